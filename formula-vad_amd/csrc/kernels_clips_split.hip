// kernels_clips_split.hip -- the batch Recorder over a split source (fvad_clips_export_split*): a clip's channel is a head piece
// in buffer A followed by a body piece in buffer B, as MRBRecorder reads a recording from its ring as a SplitSlice
// (MRBRecorder.zig:160-192).  A run sliced in time keeps only the tail of earlier slices (A) beside the current slice's lanes (B);
// a clip may lie in either or across the seam, and the carry of the tail itself is a split export of one mono clip per lane.
//
// The work unit, the prefix tables, the partials and the pick are kernels_clips.hip's: a tile of kClipTile samples of one (clip,
// channel), tiles counted from the clip's first sample -- never from the seam --, one f64 partial per unit in rms_tile's sum order,
// clip_pick_kernel as it is.  A split clip's samples, pick and RMS values are therefore the bits fvad_clips_export_device gives for
// the same samples laid out contiguously, wherever the seam is.
//
// A tile is staged by stage_split (clip_split_device.h): one run where it lies wholly in one piece, two where it holds the seam.
// Every later read is by sample index within the tile (Staged::at).
#include <hip/hip_runtime.h>

#include "clip_device.h"
#include "clip_split_device.h"
#include "kernels.h"
#include "stage_tile.h"

namespace {

constexpr int kThreads = kStageThreads;

} // namespace

template <typename S>
__global__ __launch_bounds__(kThreads) void clip_rms_split_kernel(ClipSplitArgs a)
{
    __shared__ __attribute__((aligned(16))) S lds[lds_elems<S>()];
    __shared__ double wsum[kThreads / 64];
    const uint32_t u = blockIdx.x;
    const uint32_t c = find_clip(a.c.unit_prefix, a.c.n_clips, u);
    const ClipJob j = a.c.jobs[c];
    const uint32_t r = u - j.first_unit;
    const uint32_t ch = r / j.n_tiles, k = r % j.n_tiles;
    const uint64_t e0 = (uint64_t)k * kClipTile;
    const int n = (int)min((uint64_t)kClipTile, j.len - e0);
    const Staged st = stage_split<S>(a, a.splits[c], ch, e0, n, lds);
    // rms_tile's order (kernels_clips.hip): a thread adds its samples t, t + 256, ... one after the other, then the tree below
    const int t = threadIdx.x;
    double s = 0.0;
    for (int e = t; e < n; e += kThreads) {
        const double x = (double)to_f32(lds[st.at(e)]); // the product of two f32 is exact in f64
        s += x * x;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((t & 63) == 0) wsum[t >> 6] = s;
    __syncthreads();
    if (t == 0) a.c.partials[u] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

template <typename D, typename S>
__global__ __launch_bounds__(kThreads) void clip_gather_split_kernel(ClipSplitArgs a)
{
    __shared__ __attribute__((aligned(16))) S lds[lds_elems<S>()];
    constexpr int G = 8; // samples per thread and step: one 16-byte store of PCM16, two of f32
    const uint32_t g = blockIdx.x;
    const uint32_t c = find_clip(a.c.tile_prefix, a.c.n_clips, g);
    const ClipJob j = a.c.jobs[c];
    const uint32_t k = g - a.c.tile_prefix[c];
    const uint32_t ch = (uint32_t)a.c.infos[c].best_channel;
    const uint64_t e0 = (uint64_t)k * kClipTile;
    const int n = (int)min((uint64_t)kClipTile, j.len - e0);
    const Staged st = stage_split<S>(a, a.splits[c], ch, e0, n, lds);
    D* out = static_cast<D*>(a.c.out) + j.out_off + e0; // 16-byte aligned: the slot is, and kClipTile is a multiple of G
    for (int q = threadIdx.x * G; q < n; q += kThreads * G) {
        if (q + G <= n) {
            alignas(16) D v[G];
#pragma unroll
            for (int i = 0; i < G; ++i) v[i] = Convert<D, S>::run(lds[st.at(q + i)]);
            constexpr int NV = G * (int)sizeof(D) / 16;
#pragma unroll
            for (int i = 0; i < NV; ++i) reinterpret_cast<uint4*>(out + q)[i] = reinterpret_cast<const uint4*>(v)[i];
        } else { // the clip's last samples: nothing is written past the clip
            for (int i = q; i < n; ++i) out[i] = Convert<D, S>::run(lds[st.at(i)]);
        }
    }
}

int fvad_launch_clip_rms_split(const ClipSplitArgs& a, hipStream_t stream)
{
    if (a.c.src_i16) hipLaunchKernelGGL(clip_rms_split_kernel<int16_t>, dim3(a.c.n_units), dim3(kThreads), 0, stream, a);
    else hipLaunchKernelGGL(clip_rms_split_kernel<float>, dim3(a.c.n_units), dim3(kThreads), 0, stream, a);
    return (int)hipGetLastError();
}

int fvad_launch_clip_gather_split(const ClipSplitArgs& a, hipStream_t stream)
{
    const dim3 grid(a.c.n_tiles), block(kThreads);
    if (a.c.src_i16 && a.c.out_i16) hipLaunchKernelGGL((clip_gather_split_kernel<int16_t, int16_t>), grid, block, 0, stream, a);
    else if (a.c.src_i16) hipLaunchKernelGGL((clip_gather_split_kernel<float, int16_t>), grid, block, 0, stream, a);
    else if (a.c.out_i16) hipLaunchKernelGGL((clip_gather_split_kernel<int16_t, float>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((clip_gather_split_kernel<float, float>), grid, block, 0, stream, a);
    return (int)hipGetLastError();
}
