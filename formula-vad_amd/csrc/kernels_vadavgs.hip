// kernels_vadavgs.hip -- the short-term and channel-ratio averages of a part's frames, frame-parallel (context option vad_avgs
// "table"): what every machine's two short rings (kernels_vad.hip: Ring::push) would give in each frame, computed once per key
// -- (band, short_len) and (size, ratio_len) -- instead of once per (stream, config) machine, since neither the inputs nor the
// rings depend on what a machine decides.  The arithmetic is vad_avgs.h's: the reference's chain over the ring's slots in slot
// order, with the reference's bits.
//
// vad_minvol_kernel: the min_volume row of every (band, stream): the minimum over the stream's channels in channel order from
// 999.0f (VADMachine.zig:153-158, as min_vol in kernels_vad.hip).
// vad_avgs_kernel: one lane per (key, stream, frame of the part).  A ring slot that was last written inside the part is read
// from the part's input row (min_volume or the frame ratios); one written before the part's first frame from the rings' home of
// a machine with that key, which holds the ring as it was when the part began (the launches of the part change the homes only
// after the table has been filled).  Neighbouring lanes read overlapping windows of one row: the caches serve them, there is no
// LDS.  Every loop is bounded by the key's ring length or the channel count; every index is below the counts the host checked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "vad_avgs.h"

__global__ __launch_bounds__(kAvgsTile) void vad_minvol_kernel(VadAvgsArgs a)
{
    const long k = (long)blockIdx.x * kAvgsTile + threadIdx.x;
    const long s = blockIdx.y;
    const long j = blockIdx.z; // band
    const long g = a.size_of_band ? (long)a.size_of_band[j] : 0;
    if (k >= a.n_frames[g * a.n_streams + s]) return;
    const int C = a.n_channels;
    const float* band = a.band + (j * a.n_lanes + s * C) * a.band_stride + k;
    float mn = 999;
    for (int ch = 0; ch < C; ++ch) {
        const float v = band[(long)ch * a.band_stride];
        if (v < mn) mn = v;
    }
    a.minvol[(j * a.n_streams + s) * a.minvol_stride + k] = mn;
}

__global__ __launch_bounds__(kAvgsTile) void vad_avgs_kernel(VadAvgsArgs a)
{
    const long k = (long)blockIdx.x * kAvgsTile + threadIdx.x;
    const long s = blockIdx.y;
    const bool is_st = (int)blockIdx.z < a.n_st_keys;
    const VadAvgKey key = is_st ? a.st_keys[blockIdx.z] : a.cr_keys[(int)blockIdx.z - a.n_st_keys];
    const long g = key.size;
    if (k >= a.n_frames[g * a.n_streams + s]) return;
    const uint64_t ff = a.first_frame[g], n = ff + (uint64_t)k;
    const float* row = is_st ? a.minvol + ((long)key.src * a.n_streams + s) * a.minvol_stride
                             : a.ratio + ((long)key.src * a.n_streams + s) * a.ratio_stride;
    double avg;
    if (ff == 0 || (uint64_t)k + 1 >= key.len) { // every slot was last written inside the part
        avg = fvad::ring_avg_at(n, key.len, key.scalar, [&](uint32_t, uint64_t f) { return row[f - ff]; });
    } else {
        const long place = a.by_config ? key.rep * a.n_streams + s : s * a.n_configs + key.rep;
        const float* home = a.rings + (is_st ? 0 : (long)a.st_max * a.n_machines) + place;
        avg = fvad::ring_avg_at(n, key.len, key.scalar,
                                [&](uint32_t i, uint64_t f) { return f >= ff ? row[f - ff] : home[(long)i * a.n_machines]; });
    }
    double* tab = is_st ? a.st_tab : a.cr_tab;
    tab[key.base + (s * a.tab_frames[g] + k) * (long)key.nk] = avg;
}

int fvad_launch_vad_minvol(const VadAvgsArgs& a, hipStream_t stream)
{
    if (a.max_frames <= 0 || a.n_streams <= 0 || a.n_bands <= 0) return (int)hipSuccess;
    const unsigned tiles = (unsigned)((a.max_frames + kAvgsTile - 1) / kAvgsTile);
    hipLaunchKernelGGL(vad_minvol_kernel, dim3(tiles, (unsigned)a.n_streams, (unsigned)a.n_bands), dim3(kAvgsTile), 0, stream, a);
    return (int)hipGetLastError();
}

int fvad_launch_vad_avgs(const VadAvgsArgs& a, hipStream_t stream)
{
    if (a.max_frames <= 0 || a.n_streams <= 0 || a.n_st_keys + a.n_cr_keys <= 0) return (int)hipSuccess;
    const unsigned tiles = (unsigned)((a.max_frames + kAvgsTile - 1) / kAvgsTile);
    hipLaunchKernelGGL(vad_avgs_kernel, dim3(tiles, (unsigned)a.n_streams, (unsigned)(a.n_st_keys + a.n_cr_keys)), dim3(kAvgsTile), 0,
                       stream, a);
    return (int)hipGetLastError();
}
