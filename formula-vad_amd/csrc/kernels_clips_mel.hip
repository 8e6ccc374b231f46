// kernels_clips_mel.hip -- log-mel features of speech clips (fvad_clips_export_mel*): of a clip's picked channel the strided
// stream s[i] = sample skip + i * step, cut into frames of n_fft taps every `hop`, centred with reflection (torch.stft's
// center = True without its last frame), then |rfft(frame * window)|^2 -> mel[m] = sum_k M[m][k] P[k] -> log10(max(., floor)).
// What a recogniser takes in, computed where the denoised lanes already are; only [T][n_mels] floats per clip leave the device.
// RMS and pick are kernels_clips.hip's over EVERY sample of the clip.
//
// Work unit: a tile of feat_tile_frames(n_fft, hop) <= 32 consecutive frames of one clip, found by a search of the host-built
// prefix table with the block index.  The tile's window of the stream -- (F - 1) hop + n_fft samples at most, cut to the clip --
// is staged through LDS once as f32: stage_tile (f32 lanes at step 1: 16-byte loads), stage_tile_strided (f32 lanes at a step:
// one dword per kept sample) or one converting load per kept sample (PCM16).  Taps in front of the clip's first or behind its
// last kept sample are read element by element from inside the clip, at rho(j) = -j or 2 (L - 1) - j.  Nothing outside the
// clip, and at a step > 1 no sample off the stride, is read.
//
// Two transforms, chosen by n_fft (and the context option clip_mel_fft) alone, never by the size of the call:
// - clip_mel_kernel, any even n_fft: generic_rfft (fftgen_device.h) frame after frame by the whole workgroup.
// - clip_mel400_kernel, n_fft == 400: the complex transform of N = 200 = 25 x 8 in fft_device.h's scheme, a frame on EIGHT lanes
//   with 25 points each (z[a + 8 j] in lane a), eight frames per wavefront, the tile's 32 frames in one pass:
//       Z[k1 + 25 k2] = sum_a W8^{a k2} ( W200^{a k1} sum_j z[a + 8 j] W25^{j k1} )
//   a 25-point transform in registers (5 x dft5, sixteen twiddles, 5 x dft5), one twiddle multiply, three exchange stages across
//   the frame's lanes (lane ^ 4, ^ 2, ^ 1 through the LDS crossbar, ds_swizzle), kissfft's un-mixing pass through a slab of 400
//   floats per frame, powers written over the bins they came from.  The sibling of rfft320_batch8_kernel (R = 20, L = 8).
// Both end the same way: lane m of a frame adds M[m][k] P[k] in ascending k -- one rounded product and one rounded sum per k,
// fp contraction off -- from the transposed matrix (neighbouring lanes read neighbouring floats, from L2) and the frame's
// powers in LDS (one address per frame: a broadcast).  No atomics: a tile's largest feature is a fixed tree over the workgroup
// (clip_mel_kernel / clip_mel400_kernel), a clip's the maximum of its tiles' in tile order by one lane (clip_mel_max_kernel),
// and the optional normalisation an element-wise pass of its own (clip_mel_norm_kernel).  A frame's features therefore depend on
// that frame's samples and the call's parameters alone: not on the tile, the wavefront slot, the other clips or any alignment.
//
// LDS banks (clip_mel400_kernel).  Frame loads: lane (f, a) reads floats 160 f + 2 a + 16 j (+ 1) of the window (hop 160):
// within a 32-lane half the frames f and f + 2 share their banks, 2-way.  Slab stores, 8 bytes at dword 400 f + 50 k2 + 2 k1:
// the eight lanes of a frame hit the bank pairs {0, 18, 4, 22, 8, 26, 12, 30} + {0, 1}, the next frame the other sixteen banks
// (400 = 16 mod 32): 32 lanes x 8 bytes in two cycles, the minimum.  Un-mixing reads, 8 bytes at dword 400 f + 2 a + 16 u and
// its mirror: 400 = 16 mod 64, four frames x sixteen dwords: conflict-free.
// The filter-bank export (fvad_clips_export_fbank*) is clip_mel_kernel with kFbank on: frames of `win` taps from t hop on (Kaldi's
// snip_edges: T = 1 + (L - win) / hop, every tap inside the staged window, so no element-by-element path), the frame conditioned
// in LDS by the workgroup (fbank_condition: scale at the frame load, the mean in a fixed order, pre-emphasis reading d[i - 1] from
// LDS) and zero-padded to n_fft, the same generic_rfft call and projection loop, logf; lane m also adds its features over the
// tile's frames in ascending t.  clip_fbank_mean_kernel adds the tiles' sums in tile order by one lane per (clip, band) and divides
// by f32(T); clip_fbank_sub_kernel subtracts element-wise.  The log-mel export's instances are kFbank off.
// Both families take one argument struct (ClipFeatArgs of kernels.h: the filter-bank fields behind the log-mel ones), count a
// clip's frames and a tile's by feature_frames.h's functions, which the host rules use too (clip_stream_len, mel_tile), and
// launch their tile kernels through one ladder (launch_tiles: the dynamic-LDS attribute, then the instance of the source's format).
// The split-source exports (fvad_clips_export_split_mel*, _split_fbank*) are the three tile kernels with the source as a template
// parameter (B: ClipArgs, or ClipSplitArgs -- a head piece in buffer A followed by a body piece in buffer B, kernels.h).  Stream
// sample i is clip sample e = skip + i step, in A when e < a_len, else in B at e - a_len: the stride, the tiles and the frames are
// counted from the clip's first sample, never from the seam.  Only mel_stage and MelRun::stream (the reflected taps) know the
// source.  A tile wholly in one piece is staged as the contiguous source stages it, from that piece's pointer; the one tile per
// clip that holds the seam is staged element by element into the SAME contiguous image at shift 0, so every later read, the LDS
// sizes and the bank analysis above hold for both sources.  max, norm, mean and sub read tables and features only.
// Resources (make resource-usage, gfx950): see the table in DESIGN 7.2; clip_mel400_kernel is LDS-bound at two workgroups per
// CU (73.3 KB each: 177 VGPRs, two wavefronts per SIMD); clip_mel_kernel takes 28.0 KB at 400 / 160 (80 VGPRs, five workgroups per CU).
#include <hip/hip_runtime.h>

#include "clip_device.h"
#include "fftgen_device.h"
#include "kernels.h"
#include "stage_tile_strided.h"

namespace {

constexpr int kThreads = kStageThreads;
static_assert(kThreads == 256, "generic_rfft strides by 256 lanes, and the 400-point form seats 32 frames on 256 lanes");

// the tile of this workgroup: frames [t0, t0 + nf) of `clip`, whose stream has L samples; stream samples [w0, w1) are staged
struct MelTile {
    uint32_t clip;
    int nf;
    long long t0, L, w0, w1;
};

// job j's stream: feat_stream_len's L in the form the kernels have always had (len + step cannot wrap here: the clip lies inside
// the lanes).  Its frames are feature_frames.h's feat_frames in the kernels' integer type, long long
__device__ inline long long clip_stream_len(const ClipFeatArgs& a, const ClipJob& j) { return (long long)((j.len - j.skip + a.step - 1) / a.step); }

// kSnip (the filter-bank export): frames of a.win taps from t hop on, none leaving the stream (L >= win: the plan); a.pl.n taps
// centred otherwise
template <bool kSnip = false>
__device__ inline MelTile mel_tile(const ClipFeatArgs& a, const ClipJob& j, uint32_t clip)
{
    MelTile t;
    t.clip = clip;
    t.L = clip_stream_len(a, j);
    const long long taps = kSnip ? (long long)a.win : (long long)a.pl.n;
    const long long T = fvad::feat_frames<long long>(kSnip, t.L, taps, a.hop), pad = fvad::feat_pad<int>(kSnip, a.pl.n);
    t.t0 = (long long)(blockIdx.x - a.c.tile_prefix[clip]) * a.tile_frames;
    t.nf = (int)min((long long)a.tile_frames, T - t.t0);
    const long long lo = t.t0 * a.hop - pad, hi = (t.t0 + t.nf - 1) * a.hop - pad + taps;
    t.w0 = max(lo, 0ll);
    t.w1 = min(hi, t.L); // w0 <= t0 hop < w1; w1 - w0 <= (nf - 1) hop + n_fft <= kClipTile
    return t;
}

__host__ __device__ inline const ClipFeatArgs& feat_args(const ClipFeatArgs& a) { return a; }
__host__ __device__ inline const ClipFeatArgs& feat_args(const ClipFeatSplitArgs& a) { return a.f; }

// where the picked channel's stream is, by source B: stream sample r is clip sample skip + r step, of one run or of two pieces
template <typename S, typename B> struct MelRun;
template <typename S> struct MelRun<S, ClipArgs> {
    const S* pc; // stream sample 0: the picked channel's first kept sample
    uint32_t step;
    __device__ float stream(long long r) const { return to_f32(pc[(unsigned long long)r * step]); }
};
template <typename S> struct MelRun<S, ClipSplitArgs> {
    const S *pa, *pb; // the picked channel's clip sample 0 in piece A and clip sample a_len in piece B
    uint64_t a_len;
    uint32_t skip, step;
    __device__ float stream(long long r) const
    {
        const uint64_t e = skip + (unsigned long long)r * step; // < len: the stride's phase is the clip's, on either side of the seam
        return to_f32(*(e < a_len ? pa + e : pb + (e - a_len))); // one load from the selected address
    }
};

// the stream as a frame reads it: staged samples from LDS, the reflected ends from the clip itself
template <typename S, typename B> struct MelSrc {
    MelRun<S, B> run;
    const float* lds; // stream sample w0
    long long w0, w1, L;
    __device__ float at(long long j) const
    {
        if (j >= w0 && j < w1) return lds[j - w0];
        const long long r = j < 0 ? -j : (j >= L ? 2 * (L - 1) - j : j); // 0 <= r < L: L >= n_fft / 2 + 1 (the plan)
        return run.stream(r);
    }
};

// n stream samples p[0], p[step], ... of one run into LDS; the first of them is at the returned address.  Ends with a barrier
template <typename S>
__device__ inline const float* mel_stage_run(const S* p, int n, uint32_t step, float* lds)
{
    if constexpr (sizeof(S) == 4) {
        if (step == 1) return lds + stage_tile(p, n, lds);
        stage_tile_strided(p, n, step, lds);
    } else {
        for (int i = threadIdx.x; i < n; i += kThreads) lds[i] = to_f32(p[(uint32_t)i * step]); // (n - 1) step < 2^17
        __syncthreads();
    }
    return lds;
}

template <typename S>
__device__ inline MelSrc<S, ClipArgs> mel_stage(const ClipFeatArgs& a, const ClipJob& j, const MelTile& t, float* lds)
{
    const uint32_t ch = (uint32_t)a.c.infos[t.clip].best_channel;
    const S* pc = static_cast<const S*>(a.c.src) + j.src_off + (uint64_t)ch * a.c.lane_stride + j.skip;
    const float* first = mel_stage_run(pc + (unsigned long long)t.w0 * a.step, (int)(t.w1 - t.w0), a.step, lds);
    return MelSrc<S, ClipArgs>{{pc, a.step}, first, t.w0, t.w1, t.L};
}

// A tile whose kept samples lie wholly in one piece is staged from that piece as the contiguous source stages it.  The tile that
// holds the seam (at most one per clip) is staged element by element into the same contiguous image at shift 0, one dword or one
// converting load per kept sample, the piece picked per element -- so every later read of the window is the contiguous form's.
// Nothing outside either piece is read, and at a step above 1 no sample off the stride.
template <typename S>
__device__ inline MelSrc<S, ClipSplitArgs> mel_stage(const ClipFeatSplitArgs& s, const ClipJob& j, const MelTile& t, float* lds)
{
    const ClipFeatArgs& a = s.f;
    const uint32_t ch = (uint32_t)a.c.infos[t.clip].best_channel;
    const ClipSplit sp = s.splits[t.clip];
    const S* pa = static_cast<const S*>(a.c.src) + sp.a_off + (uint64_t)ch * a.c.lane_stride;
    const S* pb = static_cast<const S*>(s.b) + sp.b_off + (uint64_t)ch * s.b_stride;
    const int n = (int)(t.w1 - t.w0);
    const uint64_t e0 = j.skip + (unsigned long long)t.w0 * a.step, e1 = e0 + (uint64_t)(n - 1) * a.step; // the first and last kept sample
    const float* first = lds;
    if (e1 < sp.a_len) first = mel_stage_run(pa + e0, n, a.step, lds);
    else if (e0 >= sp.a_len) first = mel_stage_run(pb + (e0 - sp.a_len), n, a.step, lds);
    else {
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const uint64_t e = e0 + (uint32_t)i * a.step;
            lds[i] = to_f32(*(e < sp.a_len ? pa + e : pb + (e - sp.a_len)));
        }
        __syncthreads();
    }
    return MelSrc<S, ClipSplitArgs>{{pa, pb, sp.a_len, j.skip, a.step}, first, t.w0, t.w1, t.L};
}

__device__ inline float mel_feat(float mel, float floor, float log_floor) { return mel > floor ? log10f(mel) : log_floor; }
__device__ inline float fbank_feat(float mel, float floor, float log_floor) { return mel > floor ? logf(mel) : log_floor; }

// a fixed tree: 64 lanes by shuffles, then the four wavefronts in order
__device__ inline void tile_max_store(float v, float* red, float* dst)
{
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) *dst = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// stage_tile's LDS image of a tile's window: the samples and room for the global address's offset within 16 bytes
__host__ __device__ inline uint32_t mel_stage_floats(uint32_t n_fft, uint32_t hop, uint32_t tile_frames)
{
    return ((tile_frames - 1) * hop + n_fft + 4 + 3) / 4 * 4;
}

// the dynamic LDS of clip_mel_kernel behind `stage` floats of the window: s_win, s_frame, bufA, bufB, s_pow
inline size_t mel_generic_lds(uint32_t stage, uint32_t n_fft) { return (size_t)(stage + 2 * n_fft + 4 * (n_fft / 2 + 1) + (n_fft / 2 + 1)) * sizeof(float); }

// The conditioning of one filter-bank frame by the whole workgroup (fvad.h's order, every operation rounded on its own): x the
// frame's `win` staged samples, y [n_fft] what generic_rfft windows, d [win] scratch, red one float per wavefront.
//   x_i = x[i] * scale          -- the scale is applied HERE, at the frame load, not at staging (one rounded product either way)
//   mean = S / f32(win)         -- with remove_dc.  THE SUM ORDER, fixed by win alone: lane l of the 256 adds x_l, x_{l + 256},
//                                  x_{l + 512}, ... in ascending order onto 0.0f (a lane at or past win keeps 0.0f); each wavefront
//                                  folds its 64 sums by v_l += v_{l + o} for o = 32, 16, 8, 4, 2, 1 (lane 0 holds the result);
//                                  S = ((w_0 + w_1) + w_2) + w_3 over the four wavefronts
//   d_i = x_i - mean            -- (x_i without remove_dc), written to LDS
//   y_i = d_i - preemph * d_{i - 1}, d_{-1} = d_0 (Kaldi's replicated first sample); y_i = 0 for win <= i < n_fft
// Ends with a barrier.
__device__ inline void fbank_condition(const ClipFeatArgs& a, const float* x, float* y, float* d, float* red)
{
    const int tid = threadIdx.x, win = (int)a.win, n_fft = a.pl.n;
    float mean = 0.0f;
    if (a.remove_dc) {
        float v = 0.0f;
        for (int i = tid; i < win; i += kThreads) v += x[i] * a.scale;
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        mean = (((red[0] + red[1]) + red[2]) + red[3]) / (float)win;
    }
    for (int i = tid; i < win; i += kThreads) {
        const float xi = x[i] * a.scale;
        d[i] = a.remove_dc ? xi - mean : xi;
    }
    __syncthreads();
    for (int i = tid; i < n_fft; i += kThreads) y[i] = i < win ? d[i] - a.preemph * d[i > 0 ? i - 1 : 0] : 0.0f;
    __syncthreads();
}

} // namespace

// ---------------------------------------------------------------------------- any even n_fft
// kFbank: the filter-bank export's frames (snip_edges, conditioned, win taps zero-padded to n_fft, natural log) and, in place of
// the tile's maximum, the tile's sum per band over ascending t by lane m
template <typename S, bool kFbank, typename B>
__global__ __launch_bounds__(kThreads) void clip_mel_kernel(typename ClipFeatOf<B>::type args)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float red[kThreads / 64];
    const ClipFeatArgs& a = feat_args(args);
    const int n_fft = a.pl.n, M = n_fft / 2, NB = M + 1, pad = M;
    int taps = n_fft;
    if constexpr (kFbank) taps = (int)a.win;
    float* s_stage = sm;
    float* s_win = s_stage + mel_stage_floats(taps, a.hop, a.tile_frames);
    float* s_frame = s_win + n_fft;
    cpx* bufA = reinterpret_cast<cpx*>(s_frame + n_fft);
    cpx* bufB = bufA + NB;
    float* s_pow = reinterpret_cast<float*>(bufB + NB);
    const int tid = threadIdx.x;
    const uint32_t clip = find_clip(a.c.tile_prefix, a.c.n_clips, blockIdx.x);
    const ClipJob j = a.c.jobs[clip];
    const MelTile t = mel_tile<kFbank>(a, j, clip);
    if constexpr (kFbank) {
        for (int i = tid; i < n_fft; i += kThreads) s_win[i] = i < taps ? a.window[i] : 0.0f;
    } else {
        for (int i = tid; i < n_fft; i += kThreads) s_win[i] = a.window[i];
    }
    const auto src = mel_stage<S>(args, j, t, s_stage); // (ends with a barrier)
    float* out = static_cast<float*>(a.c.out) + j.out_off + (unsigned long long)t.t0 * a.n_mels;
    float vmax = -__builtin_inff(), vsum = 0.0f;
    for (int f = 0; f < t.nf; ++f) {
        if constexpr (kFbank) {
            // every tap is staged: the tile's window starts at its first frame's first tap (w0 == t0 hop)
            fbank_condition(a, src.lds + (size_t)f * a.hop, s_frame, reinterpret_cast<float*>(bufB), red);
        } else {
            const long long j0 = (t.t0 + f) * a.hop - pad;
            for (int i = tid; i < n_fft; i += kThreads) s_frame[i] = src.at(j0 + i);
            __syncthreads();
        }
        cpx* X;
        generic_rfft(s_frame, s_win, a.pl, bufA, bufB, X); // (ends with a barrier)
        for (int k = tid; k < NB; k += kThreads) s_pow[k] = X[k].r * X[k].r + X[k].i * X[k].i;
        __syncthreads();
        if (tid < (int)a.n_mels) {
            const float* mt = a.matrix_t + tid;
            float acc = 0.0f;
            for (int k = 0; k < NB; ++k) acc += mt[(size_t)k * a.n_mels] * s_pow[k];
            const float v = kFbank ? fbank_feat(acc, a.floor, a.log_floor) : mel_feat(acc, a.floor, a.log_floor);
            out[(size_t)f * a.n_mels + tid] = v;
            if constexpr (kFbank) vsum += v;
            else vmax = fmaxf(vmax, v);
        }
        __syncthreads(); // the next frame overwrites s_frame and s_pow
    }
    if constexpr (kFbank) {
        if (tid < (int)a.n_mels) a.tile_sum[(size_t)blockIdx.x * a.n_mels + tid] = vsum;
    } else {
        tile_max_store(vmax, red, a.tile_max + blockIdx.x);
    }
}

// ---------------------------------------------------------------------------- n_fft == 400: eight frames per wavefront
namespace {

constexpr int kM4 = 200, kSlab = 400; // the complex transform's length; floats per frame of the slab

// 25 points in registers: v[j] in; position 5 ka + kb holds X[ka + 5 kb] out (j = 5 j1 + j2:
// X[ka + 5 kb] = sum_j2 W5^{j2 kb} ( W25^{j2 ka} sum_j1 v[5 j1 + j2] W5^{j1 ka} )); w25 = W200^8, read from the table
__device__ __forceinline__ void dft25(cpx (&v)[25], const float* __restrict__ tw200)
{
#pragma unroll
    for (int j2 = 0; j2 < 5; ++j2) {
        cpx t[5] = {v[j2], v[5 + j2], v[10 + j2], v[15 + j2], v[20 + j2]};
        dft5<false>(t);
#pragma unroll
        for (int ka = 0; ka < 5; ++ka) v[5 * ka + j2] = t[ka];
    }
#pragma unroll
    for (int ka = 1; ka < 5; ++ka)
#pragma unroll
        for (int j2 = 1; j2 < 5; ++j2) v[5 * ka + j2] = cmul_fma(v[5 * ka + j2], ld_tw(tw200, 8 * (j2 * ka))); // (uniform: scalar loads)
#pragma unroll
    for (int ka = 0; ka < 5; ++ka) {
        cpx t[5] = {v[5 * ka], v[5 * ka + 1], v[5 * ka + 2], v[5 * ka + 3], v[5 * ka + 4]};
        dft5<false>(t);
#pragma unroll
        for (int kb = 0; kb < 5; ++kb) v[5 * ka + kb] = t[kb];
    }
}

} // namespace

template <typename S, typename B>
__global__ __launch_bounds__(kThreads) void clip_mel400_kernel(typename ClipFeatOf<B>::type args)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float red[kThreads / 64];
    const ClipFeatArgs& a = feat_args(args);
    constexpr int n_fft = 2 * kM4, pad = kM4;
    float* s_stage = sm;
    float* s_win = s_stage + mel_stage_floats(n_fft, a.hop, a.tile_frames);
    float* s_st = s_win + n_fft;  // [100][2]: the un-mixing factors
    float* s_slab = s_st + kM4;   // [32][kSlab]
    const int tid = threadIdx.x, lane = tid & 63;
    const int slot = tid >> 3;    // the frame of the tile this lane works on (four wavefronts x eight)
    const int a8 = lane & 7;      // its row of the frame
    const uint32_t clip = find_clip(a.c.tile_prefix, a.c.n_clips, blockIdx.x);
    const ClipJob j = a.c.jobs[clip];
    const MelTile t = mel_tile(a, j, clip);
    for (int i = tid; i < n_fft; i += kThreads) s_win[i] = a.window[i];
    for (int i = tid; i < kM4; i += kThreads) s_st[i] = a.pl.st[i];
    const auto src = mel_stage<S>(args, j, t, s_stage); // (ends with a barrier)

    // ---- the transform.  Slots past the tile's last frame work on that last frame again (every lane takes part in the
    // exchanges); their slab rows are never read
    {
        const int f = slot < t.nf ? slot : t.nf - 1;
        const long long j0 = (t.t0 + f) * a.hop - pad;
        cpx v[25];
#pragma unroll
        for (int q = 0; q < 25; ++q) {
            const int n = 2 * (a8 + 8 * q);
            v[q] = {src.at(j0 + n) * s_win[n], src.at(j0 + n + 1) * s_win[n + 1]};
        }
        dft25(v, a.pl.tw);
        // position r = 5 ka + kb holds k1 = ka + 5 kb: the twiddle W200^{a k1}
#pragma unroll
        for (int r = 1; r < 25; ++r) {
            const int k1 = r / 5 + 5 * (r % 5);
            v[r] = cmul_fma(v[r], ld_tw(a.pl.tw, a8 * k1));
        }
        // three decimation-in-frequency stages across the frame's lanes, wave_fft's butterflies: the lower lane a + b, the upper
        // (a_low - a_high) w with w = W8^{a mod 4} (stride 4), W4^{a mod 2} (stride 2), 1 (stride 1)
#pragma unroll
        for (int h = 4; h >= 1; h >>= 1) {
            const float sgn = (a8 & h) ? -1.0f : 1.0f;
            cpx w = {1.0f, 0.0f};
            if (h > 1 && (a8 & h)) {
                w = ld_tw(a.pl.tw, (a8 & (h - 1)) * (kM4 / (2 * h)));
                w = {-w.r, -w.i}; // the upper lane forms mine - other
            }
#pragma unroll
            for (int r = 0; r < 25; ++r) {
                const cpx mine = v[r];
                const cpx other = {lane_xor_dyn(mine.r, h, lane), lane_xor_dyn(mine.i, h, lane)};
                if (h > 1) {
                    const cpx s = {__builtin_fmaf(other.r, sgn, mine.r), __builtin_fmaf(other.i, sgn, mine.i)};
                    v[r] = cmul_fma(s, w);
                } else {
                    v[r] = {__builtin_fmaf(sgn, mine.r, other.r), __builtin_fmaf(sgn, mine.i, other.i)};
                }
            }
        }
        const int k2 = (int)(__brev((unsigned)a8) >> 29);
        float* z = s_slab + slot * kSlab;
#pragma unroll
        for (int r = 0; r < 25; ++r) {
            const int k = (r / 5 + 5 * (r % 5)) + 25 * k2;
            *reinterpret_cast<float2*>(z + 2 * k) = make_float2(v[r].r, v[r].i);
        }
    }
    __syncthreads();
    // ---- kissfft's un-mixing, lane (frame, i) the bins k = i + 8 u <= 100 and their mirrors 200 - k; the powers go where the
    // bins were: P[k] at float 2 k of the frame's slab row (k < 200), P[200] at float 1.  A lane reads and writes its own pairs only
    if (slot < t.nf) {
        float* z = s_slab + slot * kSlab;
        for (int u = 0; u < 13; ++u) {
            const int k = a8 + 8 * u;
            if (k > kM4 / 2) break;
            if (k == 0) {
                const float2 z0 = *reinterpret_cast<const float2*>(z);
                const float x0 = z0.x + z0.y, xn = z0.x - z0.y;
                *reinterpret_cast<float2*>(z) = make_float2(x0 * x0, xn * xn);
            } else {
                const float2 zk = *reinterpret_cast<const float2*>(z + 2 * k), zn = *reinterpret_cast<const float2*>(z + 2 * (kM4 - k));
                cpx xk, xnk;
                unmix_fwd({zk.x, zk.y}, {zn.x, zn.y}, {s_st[2 * (k - 1)], s_st[2 * (k - 1) + 1]}, xk, xnk);
                if (k != kM4 - k) z[2 * k] = xk.r * xk.r + xk.i * xk.i;
                z[2 * (kM4 - k)] = xnk.r * xnk.r + xnk.i * xnk.i; // (k == 100: the X[ncfft - k] form, written last in kissfft)
            }
        }
    }
    __syncthreads();
    // ---- mel bands and the logarithm: output o = frame * n_mels + m, lanes along m
    float* out = static_cast<float*>(a.c.out) + j.out_off + (unsigned long long)t.t0 * a.n_mels;
    float vmax = -__builtin_inff();
    const int n_out = t.nf * (int)a.n_mels;
    for (int o = tid; o < n_out; o += kThreads) {
        const int f = o / (int)a.n_mels, m = o - f * (int)a.n_mels;
        const float* p = s_slab + f * kSlab;
        const float* mt = a.matrix_t + m;
        float acc = 0.0f;
        for (int k = 0; k < kM4; ++k) acc += mt[(size_t)k * a.n_mels] * p[2 * k];
        acc += mt[(size_t)kM4 * a.n_mels] * p[1];
        const float v = mel_feat(acc, a.floor, a.log_floor);
        out[o] = v;
        vmax = fmaxf(vmax, v);
    }
    tile_max_store(vmax, red, a.tile_max + blockIdx.x);
}

// one lane per clip: the maximum of its tiles' maxima, in tile order (a maximum has no rounding)
__global__ __launch_bounds__(64) void clip_mel_max_kernel(ClipFeatArgs a)
{
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c >= a.c.n_clips) return;
    float v = -__builtin_inff();
    for (uint32_t g = a.c.tile_prefix[c]; g < a.c.tile_prefix[c + 1]; ++g) v = fmaxf(v, a.tile_max[g]);
    a.feat_max[c] = v;
}

// feat' = (max(feat, feat_max - range) + offset) * scale over a tile's cells: one rounded subtraction, sum and product (fp
// contraction is off for the library)
__global__ __launch_bounds__(kThreads) void clip_mel_norm_kernel(ClipFeatArgs a)
{
    const uint32_t clip = find_clip(a.c.tile_prefix, a.c.n_clips, blockIdx.x);
    const ClipJob j = a.c.jobs[clip];
    const MelTile t = mel_tile(a, j, clip);
    float* out = static_cast<float*>(a.c.out) + j.out_off + (unsigned long long)t.t0 * a.n_mels;
    const float lo = a.feat_max[clip] - a.norm_range;
    const int n_out = t.nf * (int)a.n_mels;
    for (int o = threadIdx.x; o < n_out; o += kThreads) out[o] = (fmaxf(out[o], lo) + a.norm_offset) * a.norm_scale;
}

// ---------------------------------------------------------------------------- the filter-bank export's means
// one lane per (clip, band): the tiles' sums added in tile order onto 0.0f, over f32(T) -- one rounded division
__global__ __launch_bounds__(kThreads) void clip_fbank_mean_kernel(ClipFeatArgs a)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (unsigned long long)a.c.n_clips * a.n_mels) return;
    const uint32_t c = (uint32_t)(i / a.n_mels), m = (uint32_t)(i - (unsigned long long)c * a.n_mels);
    const ClipJob j = a.c.jobs[c];
    const long long T = fvad::feat_frames<long long>(true, clip_stream_len(a, j), a.win, a.hop);
    float s = 0.0f;
    for (uint32_t g = a.c.tile_prefix[c]; g < a.c.tile_prefix[c + 1]; ++g) s += a.tile_sum[(size_t)g * a.n_mels + m];
    a.means[i] = s / (float)T;
}

// feat' = feat - mean_m over a tile's cells: one rounded subtraction
__global__ __launch_bounds__(kThreads) void clip_fbank_sub_kernel(ClipFeatArgs a)
{
    const uint32_t clip = find_clip(a.c.tile_prefix, a.c.n_clips, blockIdx.x);
    const ClipJob j = a.c.jobs[clip];
    const MelTile t = mel_tile<true>(a, j, clip);
    float* out = static_cast<float*>(a.c.out) + j.out_off + (unsigned long long)t.t0 * a.n_mels;
    const float* mean = a.means + (size_t)clip * a.n_mels;
    const int n_out = t.nf * (int)a.n_mels;
    for (int o = threadIdx.x; o < n_out; o += kThreads) out[o] = out[o] - mean[o % (int)a.n_mels];
}

namespace {

// one workgroup per tile with `lds` bytes of dynamic LDS (which may be above the default limit), the instance by the source's format
template <typename A>
int launch_tiles(void (*f32)(A), void (*i16)(A), size_t lds, const A& a, hipStream_t stream)
{
    const ClipArgs& c = feat_args(a).c;
    void (*const k)(A) = c.src_i16 ? i16 : f32;
    const hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k, dim3(c.n_tiles), dim3(kThreads), lds, stream, a);
    return (int)hipGetLastError();
}

template <typename B>
int launch_fbank(const typename ClipFeatOf<B>::type& s, hipStream_t stream)
{
    const ClipFeatArgs& a = feat_args(s);
    const size_t lds = mel_generic_lds(mel_stage_floats(a.win, a.hop, a.tile_frames), (uint32_t)a.pl.n); // win 400, n_fft 512, hop 160: 30.0 KB
    return launch_tiles(clip_mel_kernel<float, true, B>, clip_mel_kernel<int16_t, true, B>, lds, s, stream);
}

template <typename B>
int launch_mel(const typename ClipFeatOf<B>::type& s, hipStream_t stream)
{
    const ClipFeatArgs& a = feat_args(s);
    const uint32_t n_fft = (uint32_t)a.pl.n, stage = mel_stage_floats(n_fft, a.hop, a.tile_frames);
    // the 400-point form: 73.3 KB; the generic one: 28.0 KB at n_fft 400, hop 160, at most 68.0 KB
    if (a.fft400) return launch_tiles(clip_mel400_kernel<float, B>, clip_mel400_kernel<int16_t, B>, (size_t)(stage + n_fft + kM4 + fvad::kFeatTileFrames * kSlab) * sizeof(float), s, stream);
    return launch_tiles(clip_mel_kernel<float, false, B>, clip_mel_kernel<int16_t, false, B>, mel_generic_lds(stage, n_fft), s, stream);
}

} // namespace

int fvad_launch_clip_fbank(const ClipFeatArgs& a, hipStream_t stream) { return launch_fbank<ClipArgs>(a, stream); }
int fvad_launch_clip_fbank(const ClipFeatSplitArgs& a, hipStream_t stream) { return launch_fbank<ClipSplitArgs>(a, stream); }
int fvad_launch_clip_mel(const ClipFeatArgs& a, hipStream_t stream) { return launch_mel<ClipArgs>(a, stream); }
int fvad_launch_clip_mel(const ClipFeatSplitArgs& a, hipStream_t stream) { return launch_mel<ClipSplitArgs>(a, stream); }

int fvad_launch_clip_fbank_mean(const ClipFeatArgs& a, hipStream_t stream)
{
    const unsigned long long n = (unsigned long long)a.c.n_clips * a.n_mels;
    hipLaunchKernelGGL(clip_fbank_mean_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, a);
    return (int)hipGetLastError();
}

int fvad_launch_clip_fbank_sub(const ClipFeatArgs& a, hipStream_t stream)
{
    hipLaunchKernelGGL(clip_fbank_sub_kernel, dim3(a.c.n_tiles), dim3(kThreads), 0, stream, a);
    return (int)hipGetLastError();
}

int fvad_launch_clip_mel_max(const ClipFeatArgs& a, hipStream_t stream)
{
    hipLaunchKernelGGL(clip_mel_max_kernel, dim3((a.c.n_clips + 63) / 64), dim3(64), 0, stream, a);
    return (int)hipGetLastError();
}

int fvad_launch_clip_mel_norm(const ClipFeatArgs& a, hipStream_t stream)
{
    hipLaunchKernelGGL(clip_mel_norm_kernel, dim3(a.c.n_tiles), dim3(kThreads), 0, stream, a);
    return (int)hipGetLastError();
}
