// kernels_clips.hip -- the batch Recorder (fvad_clips_export*): per clip the quietest channel over [sample_from, sample_to)
// (Recorder.findBestChannel, Recorder.zig:113-129) and that channel's samples packed into the clip's slot of one output buffer.
//
// Clips run from a fraction of a second to minutes, so the work unit is a tile of kClipTile samples of one (clip, channel): a
// workgroup finds its clip by a search of a host-built prefix table with its block index (the same in every lane: scalar loads).
// Nothing is accumulated across workgroups with atomics: clip_rms_kernel stores one f64 partial per (clip, channel, tile),
// clip_pick_kernel adds a channel's partials in tile order.  A clip's numbers therefore depend on its own samples alone, never on
// the other clips of the call.
//
// A tile is staged through LDS once, by the clip source (clip_source_device.h), and every later read of it is by sample index
// within the tile.  Each kernel is instantiated for both sources: a clip's channel as one run (fvad_clips_export*), or a head
// piece in buffer A followed by a body piece in buffer B (fvad_clips_export_split*), as MRBRecorder reads a recording from its
// ring as a SplitSlice (MRBRecorder.zig:160-192).  A run sliced in time keeps only the tail of earlier slices (A) beside the
// current slice's lanes (B); a clip may lie in either or across the seam, and the carry of the tail itself is a split export of
// one mono clip per lane.  Tiles are counted from the clip's first sample, never from the seam, and the sum order below is one
// text: a split clip's samples, pick and RMS values are the bits of the same samples laid out contiguously.
#include <hip/hip_runtime.h>

#include "clip_device.h"
#include "clip_source_device.h"
#include "kernels.h"

namespace {

constexpr int kThreads = kStageThreads;

} // namespace

// one f64 partial per (clip, channel, tile), the tiles counted from the clip's first sample
template <typename S, typename B>
__global__ __launch_bounds__(kThreads) void clip_rms_kernel(B a)
{
    __shared__ __attribute__((aligned(16))) S lds[ClipSource<B>::template lds_elems<S>()];
    __shared__ double wsum[kThreads / 64];
    const ClipArgs& c = clip_args(a);
    const uint32_t u = blockIdx.x;
    const uint32_t clip = find_clip(c.unit_prefix, c.n_clips, u);
    const ClipJob j = c.jobs[clip];
    const uint32_t r = u - j.first_unit;
    const uint32_t ch = r / j.n_tiles, k = r % j.n_tiles;
    const uint64_t e0 = (uint64_t)k * kClipTile;
    const int n = (int)min((uint64_t)kClipTile, j.len - e0);
    const auto at = ClipSource<B>::template stage<S>(a, clip, ch, e0, n, lds);
    // fixed order: a thread adds its samples t, t + 256, ... one after the other, then the tree below
    const int t = threadIdx.x;
    double s = 0.0;
    for (int e = t; e < n; e += kThreads) {
        const double x = (double)to_f32(lds[at(e)]); // the product of two f32 is exact in f64
        s += x * x;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((t & 63) == 0) wsum[t >> 6] = s;
    __syncthreads();
    if (t == 0) c.partials[u] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one lane per clip: rms = (float)sqrt(sum / n) per channel, the channel's partials added in tile order; the pick is
// Recorder.findBestChannel's (strict <, in channel order, from 9999: the lowest index wins a tie)
__global__ __launch_bounds__(64) void clip_pick_kernel(ClipArgs a)
{
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c >= a.n_clips) return;
    const ClipJob j = a.jobs[c];
    auto rms_of = [&](uint32_t ch) {
        const double* p = a.partials + j.first_unit + (uint64_t)ch * j.n_tiles;
        double s = 0.0;
        for (uint32_t k = 0; k < j.n_tiles; ++k) s += p[k];
        return (float)sqrt(s / (double)j.len);
    };
    uint32_t best = 0;
    float best_vol = 9999.0f, rms0 = 0.0f;
    for (uint32_t ch = 0; ch < j.n_channels; ++ch) {
        const float vol = rms_of(ch);
        if (ch == 0) rms0 = vol;
        if (vol < best_vol) { best = ch; best_vol = vol; }
    }
    const float best_rms = best == 0 ? rms0 : best_vol; // (channel 0 also stands when no channel is below 9999)
    float runner = best_rms;
    bool have = false;
    for (uint32_t ch = 0; ch < j.n_channels; ++ch) {
        if (ch == best) continue;
        const float vol = rms_of(ch);
        if (!have || vol < runner) { runner = vol; have = true; }
    }
    ClipInfo o;
    o.best_channel = (int32_t)best;
    o.best_rms = best_rms;
    o.runner_up_rms = runner;
    o.out_offset = j.out_off;
    a.infos[c] = o;
}

// the picked channel's samples into the clip's slot, 8 consecutive outputs per lane and pass
template <typename D, typename S, typename B>
__global__ __launch_bounds__(kThreads) void clip_gather_kernel(B a)
{
    __shared__ __attribute__((aligned(16))) S lds[ClipSource<B>::template lds_elems<S>()];
    constexpr int G = 8; // samples per thread and step: one 16-byte store of PCM16, two of f32
    const ClipArgs& c = clip_args(a);
    const uint32_t g = blockIdx.x;
    const uint32_t clip = find_clip(c.tile_prefix, c.n_clips, g);
    const ClipJob j = c.jobs[clip];
    const uint32_t k = g - c.tile_prefix[clip];
    const uint32_t ch = (uint32_t)c.infos[clip].best_channel;
    const uint64_t e0 = (uint64_t)k * kClipTile;
    const int n = (int)min((uint64_t)kClipTile, j.len - e0);
    const auto at = ClipSource<B>::template stage<S>(a, clip, ch, e0, n, lds);
    D* out = static_cast<D*>(c.out) + j.out_off + e0; // 16-byte aligned: the slot is, and kClipTile is a multiple of G
    for (int q = threadIdx.x * G; q < n; q += kThreads * G) {
        if (q + G <= n) {
            alignas(16) D v[G];
#pragma unroll
            for (int i = 0; i < G; ++i) v[i] = Convert<D, S>::run(lds[at(q + i)]);
            constexpr int NV = G * (int)sizeof(D) / 16;
#pragma unroll
            for (int i = 0; i < NV; ++i) reinterpret_cast<uint4*>(out + q)[i] = reinterpret_cast<const uint4*>(v)[i];
        } else { // the clip's last samples: nothing is written past the clip
            for (int i = q; i < n; ++i) out[i] = Convert<D, S>::run(lds[at(i)]);
        }
    }
}

namespace {

template <typename B>
int launch_rms(const B& a, hipStream_t stream)
{
    const dim3 grid(clip_args(a).n_units), block(kThreads);
    if (clip_args(a).src_i16) hipLaunchKernelGGL((clip_rms_kernel<int16_t, B>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((clip_rms_kernel<float, B>), grid, block, 0, stream, a);
    return (int)hipGetLastError();
}

template <typename B>
int launch_gather(const B& a, hipStream_t stream)
{
    return launch_clip_formats(clip_args(a), [&](auto d, auto s, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((clip_gather_kernel<decltype(d), decltype(s), B>), grid, block, 0, stream, a);
    });
}

} // namespace

int fvad_launch_clip_rms(const ClipArgs& a, hipStream_t stream) { return launch_rms(a, stream); }
int fvad_launch_clip_rms(const ClipSplitArgs& a, hipStream_t stream) { return launch_rms(a, stream); }

int fvad_launch_clip_pick(const ClipArgs& a, hipStream_t stream)
{
    hipLaunchKernelGGL(clip_pick_kernel, dim3((a.n_clips + 63) / 64), dim3(64), 0, stream, a);
    return (int)hipGetLastError();
}

int fvad_launch_clip_gather(const ClipArgs& a, hipStream_t stream) { return launch_gather(a, stream); }
int fvad_launch_clip_gather(const ClipSplitArgs& a, hipStream_t stream) { return launch_gather(a, stream); }
