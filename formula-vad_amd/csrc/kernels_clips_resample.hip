// kernels_clips_resample.hip -- the batch Recorder's gathers with a rational resampler (fvad_clips_export*_resampled): output o
// of a clip of len samples, out_len = ceil(len up / down) of them, is
//     y[o] = sum_j taps[r + j up] * x[q - j],   P = K + o down = q up + r,  j = 0 .. (2 K - r) / up,  K = (n_taps - 1) / 2,
// x the picked channel of the clip as f32 (PCM16: s / 32768, exact), 0 outside [0, len), one f32 fma chain from +0 in ascending
// j, converted by Convert<D, float>.  o is counted from the CLIP's first sample: never from the lane index, the tile or the seam
// of a split clip.  RMS and pick are kernels_clips.hip's over EVERY sample of the UNRESAMPLED clip, so the pick and both RMS
// values are the full-rate export's bits.
//
// Work unit: a tile of tile_out OUTPUT samples of one clip (resampled_tile_out of clips_resample.h: the most, in eights, whose
// window fits kClipTile clip samples; 147/160 with 5121 taps: 7488, 147/640 with 20481 taps: 1848), found by a search of the
// host-built prefix table.  The tile's window [ceil((o_first down - K) / up), floor((o_last down + K) / up)], clipped to
// [0, len), is staged once by the clip source (clip_source_device.h) as it is: no byte outside the clip is read, and the seam of
// a split clip exists in staging only (the source's index functor) -- both sources run resample_run.  The zero extension is
// SKIPPED, not stored: the j range of an output is cut to the clip.  With finite taps that gives the bits multiplying the zeros
// would give (fma(t, 0, acc) is acc, and +0 for acc = +0).
//
// Lane mapping: consecutive lanes take consecutive outputs (the resampling ingest gives a lane 4 consecutive outputs, which puts
// the tap reads of neighbouring lanes 4 words apart and their window reads 4 down / up samples apart).  A pass of the workgroup
// computes 1024 outputs, lane l the outputs l, l + 256, l + 512, l + 768 of the pass, into a 4 KB LDS buffer, from which lane l
// then takes outputs 4 l .. 4 l + 3 and stores them as 16 bytes (f32) or 8 bytes (PCM16); the clip's last group is stored
// sample by sample.  Nothing is written past out_len.
// - The taps are laid out [j][o mod up] (resample_table of resample.h).  At step j the 64 lanes of a wavefront read 64
//   consecutive words (wrapping at up; up < 64: lanes with equal o mod up read one word, a broadcast): conflict-free.  The table
//   is copied into LDS beside the window when it has at most kClipResampleTableLds entries (the default designs at 147/160
//   -- 35 x 147 words, 20.1 KB --, 2/3, 1/3, 1/2, 1/6); the 140 x 147 words of 147/640 and the 70 x 147 of 147/320 stay in
//   global memory, where the same layout makes a wavefront's read two or three 128-byte lines.
// - The window reads of neighbouring lanes are down / up samples apart, and every lane steps one sample back per j, so the
//   pattern is the same at every j.  A 4-byte LDS read is banked (a / 4) mod 32 within each 32-lane half.  f32 window:
//   up >= down: a half spans at most 32 words, equal words broadcast -- conflict-free; 160/147: 32 lanes span 34.8 words --
//   2-way on at most 3 banks; 320/147: 69.7 words -- 3-way; 640/147: 139 words -- 5-way; 3/1: stride 3, odd -- conflict-free.
//   A PCM16 window halves the span in words (two samples a word, the same word a broadcast): 160/147 conflict-free, 320/147
//   2-way, 640/147 3-way.  The conflicts are left as they are: a transposed image as in kernels_clips_fir.hip needs a whole
//   number of samples between lanes.
// LDS: the staged window (32.8 KB f32, 16.4 KB PCM16), the table (24 KB, or none) and the 4 KB of a pass's outputs.
// No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "clip_device.h"
#include "clip_source_device.h"
#include "kernels.h"

namespace {

constexpr int kThreads = kStageThreads;
constexpr int kR = 4;                 // outputs per lane and pass
constexpr int kPass = kR * kThreads;  // outputs per pass

// the gather's tile of this workgroup: clip, outputs [o0, o0 + n_out) of it; the clip samples [lo, lo + n) are its window (n may
// be 0: a filter shorter than up leaves outputs without a term).  Its first output: K + o0 down = q0 up + r0, om0 = o0 mod up.
struct RsTile {
    uint32_t clip, r0, om0;
    uint64_t o0, lo, q0, len;
    int n_out, n;
};

__device__ inline RsTile rs_tile(const ClipArgs& c, uint32_t up, uint32_t down, uint32_t tile_out, uint32_t n_taps)
{
    const uint32_t g = blockIdx.x;
    RsTile t;
    t.clip = find_clip(c.tile_prefix, c.n_clips, g);
    const ClipJob j = c.jobs[t.clip];
    const uint64_t taps_last = n_taps - 1; // 2 K
    // (all below 2^63: the export refuses len * up >= 2^62)
    const uint64_t out_len = (j.len * up + down - 1) / down;
    t.len = j.len;
    t.o0 = (uint64_t)(g - c.tile_prefix[t.clip]) * tile_out;
    t.n_out = (int)min((uint64_t)tile_out, out_len - t.o0);
    const uint64_t P0 = t.o0 * down + taps_last / 2, P1 = P0 + (uint64_t)(t.n_out - 1) * down;
    t.q0 = P0 / up;
    t.r0 = (uint32_t)(P0 % up);
    t.om0 = (uint32_t)(t.o0 % up);
    t.lo = min(P0 > taps_last ? (P0 - taps_last + up - 1) / up : 0, j.len);
    const uint64_t hi = min(P1 / up + 1, j.len);
    t.n = hi > t.lo ? (int)(hi - t.lo) : 0; // <= floor(((tile_out - 1) down + 2 K) / up) + 1 <= kClipTile
    return t;
}

// the table into LDS (TL) -- the barrier of the staging that follows, or resample_run's own, orders it before the reads
template <bool TL>
__device__ inline const float* rs_table(const float* __restrict__ table, uint32_t up, uint32_t n_taps, float* tab)
{
    if constexpr (!TL) return table;
    const int n = (int)((n_taps + up - 1) / up * up);
    for (int i = threadIdx.x; i < n; i += kThreads) tab[i] = table[i];
    return tab;
}

// the tile's outputs to out (16-byte aligned) from the staged window lds, whose sample e (clip sample lo + e) is lds[at(e)]
template <typename D, typename S, typename At>
__device__ inline void resample_run(D* out, const RsTile& t, uint32_t up, uint32_t down, uint32_t n_taps, const float* tab, const S* lds,
                                    float* ybuf, At at)
{
    const int tid = threadIdx.x;
    const uint32_t taps_last = n_taps - 1;
    __syncthreads(); // the table, and a window of no samples has no staging barrier
    for (int base = 0; base < t.n_out; base += kPass) {
#pragma unroll
        for (int k = 0; k < kR; ++k) {
            const int e = base + tid + k * kThreads;
            float acc = 0.0f;
            if (e < t.n_out) {
                // 32-bit: e down + r0 <= (tile_out - 1) down + up - 1 < kClipTile * up
                const uint32_t d = (uint32_t)e * down + t.r0, qd = d / up, rr = d - qd * up;
                if (rr <= taps_last) {
                    const uint64_t q = t.q0 + qd;
                    // clip samples q - j, j = 0 .. (2 K - rr) / up, inside [0, len)
                    const uint64_t j_last = min((uint64_t)((taps_last - rr) / up), q);
                    const uint64_t j_first = q >= t.len ? q - t.len + 1 : 0;
                    if (j_first <= j_last) {
                        const int n_terms = (int)(j_last - j_first) + 1;
                        const uint32_t om = (t.om0 + (uint32_t)e) % up;
                        const float* tp = tab + om + (uint32_t)j_first * up;
                        int b = (int)(q - j_first - t.lo); // q - j_last >= lo and q - j_first < lo + n: within the window
#pragma unroll 4
                        for (int i = 0; i < n_terms; ++i, tp += up, --b) acc = __builtin_fmaf(*tp, to_f32(lds[at(b)]), acc);
                    }
                }
            }
            ybuf[tid + k * kThreads] = acc;
        }
        __syncthreads();
        const int q4 = base + kR * tid, valid = min(kR, t.n_out - q4);
        if (valid > 0) {
            const float4 y = *reinterpret_cast<const float4*>(ybuf + kR * tid);
            const D v0 = Convert<D, float>::run(y.x), v1 = Convert<D, float>::run(y.y), v2 = Convert<D, float>::run(y.z), v3 = Convert<D, float>::run(y.w);
            if (valid == kR) {
                if constexpr (sizeof(D) == 4) {
                    *reinterpret_cast<float4*>(out + q4) = make_float4(v0, v1, v2, v3); // q4 a multiple of 4, out 16-byte aligned
                } else {
                    *reinterpret_cast<uint2*>(out + q4) = make_uint2((uint32_t)(uint16_t)v0 | (uint32_t)(uint16_t)v1 << 16, (uint32_t)(uint16_t)v2 | (uint32_t)(uint16_t)v3 << 16);
                }
            } else { // the clip's last group
                out[q4] = v0;
                if (valid > 1) out[q4 + 1] = v1;
                if (valid > 2) out[q4 + 2] = v2;
            }
        }
        __syncthreads(); // ybuf is the next pass's
    }
}

} // namespace

template <typename D, typename S, typename B, bool TL>
__global__ __launch_bounds__(kThreads) void clip_gather_resampled_kernel(ClipResampleArgs<B> a)
{
    __shared__ __attribute__((aligned(16))) S lds[ClipSource<B>::template lds_elems<S>()];
    __shared__ __attribute__((aligned(16))) float ybuf[kPass];
    __shared__ float tab[TL ? kClipResampleTableLds : 1];
    const ClipArgs& c = clip_args(a.s);
    const RsTile t = rs_tile(c, a.up, a.down, a.tile_out, a.n_taps);
    const ClipJob j = c.jobs[t.clip]; // (read before the table copy and the staging: its load is not waited for behind the barrier)
    const uint32_t ch = (uint32_t)c.infos[t.clip].best_channel;
    const float* table = rs_table<TL>(a.table, a.up, a.n_taps, tab);
    // the window is counted from the clip's first sample (lo), so the filter runs through the seam of a split clip; a window of
    // no samples is not staged
    typename ClipSource<B>::At at{};
    if (t.n > 0) at = ClipSource<B>::template stage<S>(a.s, t.clip, ch, t.lo, t.n, lds);
    D* out = static_cast<D*>(c.out) + j.out_off + t.o0; // 16-byte aligned: the slot is, and tile_out is a multiple of 8
    // (the functor goes in behind a lambda, as each source's kernel used to pass it: handed over as it is, the compiler derives
    // ybuf's write address from its read address and not the other way round -- one instruction more in front of the loops,
    // which then lie 8 bytes further on in their 64-byte lines; measured 0.6 - 2 % slower with the table in LDS)
    resample_run<D, S>(out, t, a.up, a.down, a.n_taps, table, lds, ybuf, [at](int e) { return at(e); });
}

namespace {

template <typename B, bool TL>
int launch(const ClipResampleArgs<B>& a, hipStream_t stream)
{
    return launch_clip_formats(clip_args(a.s), [&](auto d, auto s, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((clip_gather_resampled_kernel<decltype(d), decltype(s), B, TL>), grid, block, 0, stream, a);
    });
}

template <typename B>
int launch(const ClipResampleArgs<B>& a, hipStream_t stream)
{
    const bool table_in_lds = (uint64_t)((a.n_taps + a.up - 1) / a.up) * a.up <= kClipResampleTableLds;
    return table_in_lds ? launch<B, true>(a, stream) : launch<B, false>(a, stream);
}

} // namespace

int fvad_launch_clip_gather_resampled(const ClipResampleArgs<ClipArgs>& a, hipStream_t stream) { return launch(a, stream); }
int fvad_launch_clip_gather_resampled(const ClipResampleArgs<ClipSplitArgs>& a, hipStream_t stream) { return launch(a, stream); }
