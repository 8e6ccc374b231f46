// kernels_vadretain.hip -- dropping configs from a sweep batch between device parts (fvad_vad_batch_retain_configs): the
// resume-form state of the kept machines (kernels_vad.hip) gathered out of the old batch's buffers into the new, smaller ones.
//
// Two launches on the caller's stream, no synchronisation between them:
// - places: a lane's rings.  The long-term rings are [rows][places][4] f32: row r of a place is one 16-byte column, copied as one
//   float4 per lane, so that a wavefront's store of 64 consecutive new places is one 1 KB run (its loads are 1 KB runs wherever
//   the kept places are consecutive in the old batch).  Only the rows the new allocation has are copied: every kept machine's
//   ring fits in them, and the slots past a machine's own long_len are never added (kernels_vad.hip).  The short-term and
//   channel-ratio homes [st + cr][places] are copied row by row, the channel-ratio rows moving up when the short-term rows shrink.
// - machines: VadLaneState, the segment count, the audit, the lazy statistics and the first min(count, seg_cap) segments of each
//   kept machine (the segments a part that keeps them on the device has written; a machine's row starts at its seg_base, which
//   is never more than its count).
// Every index is bounded by the new counts; the maps' entries are old indices the host checked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "vad_machine.h"

static_assert(sizeof(fvad::VadLaneState) % 8 == 0, "VadLaneState is copied as 8-byte words");
static_assert(sizeof(fvad_speech_segment) % 8 == 0, "segments are copied as 8-byte words");

// x: new places (grid-stride), y: rows (grid-stride)
__global__ __launch_bounds__(256) void vad_retain_places_kernel(VadRetainArgs a)
{
    const long rows = a.lt_rows + a.st + a.cr;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < a.n_places; p += (long)gridDim.x * 256) {
        const long q = a.place_src[p];
        for (long r = blockIdx.y; r < rows; r += gridDim.y) {
            if (r < a.lt_rows) {
                a.lt_dst[r * a.n_places + p] = a.lt_src[r * a.old_places + q];
            } else {
                const long i = r - a.lt_rows;                          // row of the new short-term / channel-ratio home
                const long o = i < a.st ? i : a.old_st + (i - a.st);   // the same ring's row in the old one
                a.rings_dst[i * a.n_places + p] = a.rings_src[o * a.old_places + q];
            }
        }
    }
}

// one lane per new machine (grid-stride)
__global__ __launch_bounds__(256) void vad_retain_machines_kernel(VadRetainArgs a)
{
    constexpr int kStateWords = (int)(sizeof(fvad::VadLaneState) / 8), kSegWords = (int)(sizeof(fvad_speech_segment) / 8);
    for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < a.n_places; m += (long)gridDim.x * 256) {
        const long o = a.machine_src[m];
        const uint64_t* ss = reinterpret_cast<const uint64_t*>(a.state_src + o);
        uint64_t* sd = reinterpret_cast<uint64_t*>(a.state_dst + m);
#pragma unroll
        for (int w = 0; w < kStateWords; ++w) sd[w] = ss[w];
        const uint32_t n = a.count_src[o];
        a.count_dst[m] = n;
        a.audit_dst[m].min_rel_threshold_margin = a.audit_src[o].min_rel_threshold_margin;
        a.audit_dst[m].min_abs_ratio_margin = a.audit_src[o].min_abs_ratio_margin;
        a.audit_dst[m].n_frames = a.audit_src[o].n_frames;
        a.stats_dst[2 * m] = a.stats_src[2 * o];
        a.stats_dst[2 * m + 1] = a.stats_src[2 * o + 1];
        const uint32_t k = n < a.seg_cap ? n : a.seg_cap;
        const uint64_t* gs = reinterpret_cast<const uint64_t*>(a.segs_src + o * (long)a.seg_cap);
        uint64_t* gd = reinterpret_cast<uint64_t*>(a.segs_dst + m * (long)a.seg_cap);
        for (uint32_t i = 0; i < k * (uint32_t)kSegWords; ++i) gd[i] = gs[i];
    }
}

int fvad_launch_vad_retain(const VadRetainArgs& a, hipStream_t stream)
{
    if (a.n_places <= 0) return (int)hipSuccess;
    // memory-bound: about 2048 workgroups in all, the rest grid-strided
    const long rows = a.lt_rows + a.st + a.cr;
    const unsigned gx = (unsigned)std::min<long>((a.n_places + 255) / 256, 64);
    const unsigned gy = (unsigned)std::max<long>(1, std::min<long>(rows, 2048 / gx));
    hipLaunchKernelGGL(vad_retain_places_kernel, dim3(gx, gy), dim3(256), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const unsigned gm = (unsigned)std::min<long>((a.n_places + 255) / 256, 2048);
    hipLaunchKernelGGL(vad_retain_machines_kernel, dim3(gm), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}
