// kernels_clips_fir.hip -- the batch Recorder's gathers with a FIR filter (fvad_clips_export*_fir): output q of a clip is
//     y[q] = sum over k of taps[k] * x[c + k - H],  c = skip + q * step,  H = (n_taps - 1) / 2,
// x the picked channel of the clip as f32 (PCM16: s / 32768, exact), 0 outside [0, len), accumulated in f32 by fma and converted
// by Convert<D, float>.  The strided gathers (kernels_clips_strided.hip) keep every step-th sample and so fold everything above
// the new Nyquist frequency into the band; here only the kept, band-limited samples leave the device.  RMS and pick are
// kernels_clips.hip's over EVERY sample of the UNFILTERED clip, so the pick and both RMS values are the full-rate export's bits.
//
// Work unit: a tile of tile_out = ((kClipTile - n_taps) / step + 1) / 8 * 8 OUTPUT samples of one clip, counted from the clip's
// first kept sample (never from the seam of a split clip); step 3 with 97 taps: 2696 outputs, step 16 with 513 taps: 480.  The
// tile's window is the (n_out - 1) * step + n_taps clip samples [c_first - H, c_last + H]; the part of it inside [0, len) is
// staged by the clip source (clip_source_device.h) as they are (no byte outside the clip is read), and the zero extension is
// WRITTEN INTO LDS, not tested per read: one pass copies the staged run, converted to f32, with zeros in front of and behind it,
// into a second LDS image that the filter alone reads.  That pass also makes the two sources, the two source formats and the
// seam tile one case: whatever the source's index functor and the conversion cost is paid once per staged sample and not once
// per tap.
//
// Lane mapping: a lane computes kR = 4 consecutive outputs ("a slot": outputs 4 L .. 4 L + 3 of the tile, L = lane + 256 pass).
// Its window is n_taps + 3 step samples.  With k = j + step m the sum splits into `step` branches, y[r] += taps[j + step m] *
// x_j[r + m] with x_j[u] = window[step u + j]: per (j, m) ONE new sample is read for 4 fma, the other three are the previous
// reads, kept in registers that rotate through a loop unrolled by 4 -- n_taps + 3 step LDS reads per 4 n_taps fma (step 3, 97
// taps: 106 for 388).  Every output is one fma chain from +0 in the order j = 0 .. step - 1, m ascending: the order depends on
// step and n_taps alone, never on the lane, the tile, the seam or the form, and partial sums are never shared between outputs.
// The taps are read at a wave-uniform index from the call's table, stored branch by branch so that the walk is linear (scalar
// loads; they cost the LDS nothing).
//
// Banks: a row-major image would put lanes 4 step dwords apart (step 3: 4-way, steps 2 and 6: 8-way on the 32 banks of a 4-byte
// read).  The image is therefore stored transposed: window sample i of the tile (i = RS L + o, RS = 4 step) is at
// xf[o * P + L], P = slots + the slots a window reaches past its own, made odd.  A wave's 64 lanes read 64 consecutive dwords
// for every (j, m) -- conflict-free at every step -- and the pass that writes the image has consecutive lanes P dwords apart, P
// odd: conflict-free too.  Reads are 4 bytes wide: consecutive samples of one lane are P dwords apart, so there is nothing
// wider to read.  LDS: the staged run (32.8 KB f32, 16.4 KB PCM16; the split form 48 bytes more) plus the 33.8 KB image.
// Outputs are stored 16 bytes per lane (f32) or 8 bytes per lane (PCM16), a wave's 1024 / 512 bytes contiguous; the last slot of
// a clip is stored sample by sample.  No atomics, no scratch.  Nothing is written past a clip's last kept sample.
#include <hip/hip_runtime.h>

#include "clip_device.h"
#include "clip_source_device.h"
#include "kernels.h"

namespace {

constexpr int kThreads = kStageThreads;
constexpr int kR = 4; // outputs per lane
// the image: RS * P <= (n_out - 1) * step + n_taps + 15 step - 1 <= kClipTile + 239 (RS slots <= step (n_out + 3), the reach
// <= n_taps - 1 + 3 step, two more slots for P's rounding and its odd value)
constexpr int kImage = kClipTile + 256;
static_assert(15 * (int)kClipStepMax < 256 && kClipFirTapsMax < (uint32_t)kClipTile, "kImage holds every tile's transposed window");

// the gather's tile of this workgroup: clip, outputs [o0, o0 + n_out) of it; of its window the clip samples [lo, lo + n) are
// staged and zf zeros stand in front of them
struct FirTile {
    uint32_t clip;
    uint64_t o0, lo;
    int n_out, n, zf;
};

__device__ inline FirTile fir_tile(const ClipArgs& c, uint32_t step, uint32_t tile_out, uint32_t n_taps)
{
    const uint32_t g = blockIdx.x;
    FirTile t;
    t.clip = find_clip(c.tile_prefix, c.n_clips, g);
    const ClipJob j = c.jobs[t.clip];
    const uint64_t out_len = (j.len - j.skip + step - 1) / step, H = n_taps / 2;
    t.o0 = (uint64_t)(g - c.tile_prefix[t.clip]) * tile_out;
    t.n_out = (int)min((uint64_t)tile_out, out_len - t.o0);
    const uint64_t c_first = j.skip + t.o0 * step, c_last = c_first + (uint64_t)(t.n_out - 1) * step; // c_last < len
    t.lo = c_first >= H ? c_first - H : 0;
    t.zf = c_first >= H ? 0 : (int)(H - c_first);
    t.n = (int)(min(c_last + H + 1, j.len) - t.lo); // 1 .. (tile_out - 1) * step + n_taps <= kClipTile
    return t;
}

#define FVAD_FIR_STEP(h, a, b, c, d) \
    do {                             \
        const float h_ = (h);        \
        y0 = __builtin_fmaf(h_, a, y0); \
        y1 = __builtin_fmaf(h_, b, y1); \
        y2 = __builtin_fmaf(h_, c, y2); \
        y3 = __builtin_fmaf(h_, d, y3); \
    } while (0)

// the tile's outputs to out (16-byte aligned) from the staged run lds, whose sample e is lds[at(e)]; xf is the image
template <typename D, typename S, typename At>
__device__ inline void fir_run(D* out, const FirTile& t, int step, int n_taps, const float* __restrict__ taps, const S* lds, float* xf, At at)
{
    const int tid = threadIdx.x;
    const int RS = kR * step, slots = (t.n_out + kR - 1) / kR;
    const int P = (slots + (n_taps - 1 + (kR - 1) * step) / RS + 1) | 1;
    // the image, zeros included: every element of it is written, so that no read below meets stale LDS
    {
        int o = tid % RS, s = tid / RS; // i = s * RS + o
        const int d_o = kThreads % RS, d_s = kThreads / RS;
        for (int i = tid; i < RS * P; i += kThreads) {
            const int e = i - t.zf;
            float v = 0.0f;
            if (e >= 0 && e < t.n) v = to_f32(lds[at(e)]);
            xf[o * P + s] = v;
            o += d_o;
            s += d_s;
            if (o >= RS) { o -= RS; ++s; }
        }
    }
    __syncthreads();
    const int sP = step * P;
    for (int L = tid; L < slots; L += kThreads) {
        float y0 = 0.0f, y1 = 0.0f, y2 = 0.0f, y3 = 0.0f;
        const float* __restrict__ h = taps;
        for (int j = 0; j < step && j < n_taps; ++j) {
            const int M = (n_taps - j + step - 1) / step; // the taps of branch j: >= 1
            // x_j[4 g + a] is ra[g]: window sample step (4 g + a) + j of slot L is at xf[(step a + j) P + L + g]
            const float *r0 = xf + j * P + L, *r1 = r0 + sP, *r2 = r1 + sP, *r3 = r2 + sP;
            float w0 = r0[0], w1 = r1[0], w2 = r2[0], w3;
            int m = 0, g = 0;
            for (; m + 4 <= M; m += 4, ++g) {
                w3 = r3[g];
                FVAD_FIR_STEP(h[m], w0, w1, w2, w3);
                w0 = r0[g + 1];
                FVAD_FIR_STEP(h[m + 1], w1, w2, w3, w0);
                w1 = r1[g + 1];
                FVAD_FIR_STEP(h[m + 2], w2, w3, w0, w1);
                w2 = r2[g + 1];
                FVAD_FIR_STEP(h[m + 3], w3, w0, w1, w2);
            }
            if (m < M) {
                w3 = r3[g];
                FVAD_FIR_STEP(h[m], w0, w1, w2, w3);
            }
            if (m + 1 < M) {
                w0 = r0[g + 1];
                FVAD_FIR_STEP(h[m + 1], w1, w2, w3, w0);
            }
            if (m + 2 < M) {
                w1 = r1[g + 1];
                FVAD_FIR_STEP(h[m + 2], w2, w3, w0, w1);
            }
            h += M;
        }
        const int q = kR * L, valid = min(kR, t.n_out - q);
        const D v0 = Convert<D, float>::run(y0), v1 = Convert<D, float>::run(y1), v2 = Convert<D, float>::run(y2), v3 = Convert<D, float>::run(y3);
        if (valid == kR) {
            if constexpr (sizeof(D) == 4) {
                *reinterpret_cast<float4*>(out + q) = make_float4(v0, v1, v2, v3); // q a multiple of 4, out 16-byte aligned
            } else {
                *reinterpret_cast<uint2*>(out + q) = make_uint2((uint32_t)(uint16_t)v0 | (uint32_t)(uint16_t)v1 << 16, (uint32_t)(uint16_t)v2 | (uint32_t)(uint16_t)v3 << 16);
            }
        } else { // the clip's last slot
            out[q] = v0;
            if (valid > 1) out[q + 1] = v1;
            if (valid > 2) out[q + 2] = v2;
        }
    }
}

#undef FVAD_FIR_STEP

} // namespace

template <typename D, typename S, typename B>
__global__ __launch_bounds__(kThreads) void clip_gather_fir_kernel(ClipFirArgs<B> a)
{
    __shared__ __attribute__((aligned(16))) S lds[ClipSource<B>::template lds_elems<S>()];
    __shared__ float xf[kImage];
    const ClipArgs& c = clip_args(a.s);
    const FirTile t = fir_tile(c, a.step, a.tile_out, a.n_taps);
    const uint32_t ch = (uint32_t)c.infos[t.clip].best_channel;
    // (the job's slot is read before the staging, so that its load is not waited for behind the barrier)
    D* out = static_cast<D*>(c.out) + c.jobs[t.clip].out_off + t.o0; // 16-byte aligned: the slot is, and tile_out is a multiple of 8
    // the window is counted from the clip's first sample (lo), so the filter runs through the seam of a split clip
    const auto at = ClipSource<B>::template stage<S>(a.s, t.clip, ch, t.lo, t.n, lds);
    fir_run<D, S>(out, t, (int)a.step, (int)a.n_taps, a.taps, lds, xf, at);
}

namespace {

template <typename B>
int launch(const ClipFirArgs<B>& a, hipStream_t stream)
{
    return launch_clip_formats(clip_args(a.s), [&](auto d, auto s, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((clip_gather_fir_kernel<decltype(d), decltype(s), B>), grid, block, 0, stream, a);
    });
}

} // namespace

int fvad_launch_clip_gather_fir(const ClipFirArgs<ClipArgs>& a, hipStream_t stream) { return launch(a, stream); }
int fvad_launch_clip_gather_fir(const ClipFirArgs<ClipSplitArgs>& a, hipStream_t stream) { return launch(a, stream); }
