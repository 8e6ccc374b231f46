// kernels_clips_strided.hip -- the batch Recorder's gathers with a stride (fvad_clips_export*_strided): of the picked channel the
// samples skip, skip + step, skip + 2 step, ... of the clip.  K3 brings NSNet2's 16 kHz output back to 48 kHz as [lerp, lerp,
// sample] per 16 kHz sample (resample.zig:32-79), so a denoised lane's samples at index = 2 (mod 3) are the network's output and
// step 3 exports exactly those; at index = 0 (mod 3) the original lane gives what downsampleAudio fed the network
// (resample.zig:9-29).  RMS and pick are kernels_clips.hip's over EVERY sample of the clip: only the gather differs, so the pick
// and both RMS values are the full-rate export's bits.
//
// Work unit: a tile of tile_out = floor(kClipTile / step) / 8 * 8 OUTPUT samples of one clip, counted from the clip's first kept
// sample (never from the seam of a split clip); step 3: 2728 outputs, 8182 source samples staged.  A tile's first output is on a
// 16-byte boundary of its slot, and the (n_out - 1) * step + 1 source samples from its first kept sample to its last are staged
// by the clip source (clip_source_device.h) as they are -- nothing behind the clip's last kept sample is read.
//
// Lane mapping: one output per lane and pass, lane t reads element t * step of the staged tile.  Banks of the 4-byte and narrower
// LDS reads are (byte / 4) mod 32 per 32-lane half: f32 lanes are `step` dwords apart, gcd(step, 32)-way (step 3: conflict-free,
// 2 and 6: 2-way); PCM16 lanes are step / 2 dwords apart (step 2 and 6: conflict-free, 3: 32 lanes over 48 dwords, 2-way).
// The full-rate gathers' 8 consecutive outputs per lane would put lanes 8 step elements apart: 16-, 8-, 16-way for f32 and
// 8-, 4-, 8-way for PCM16 at steps 2, 3, 6.  f32 outputs are stored 4 bytes per lane, a wave's 256 bytes contiguous.  PCM16
// outputs are paired through one shuffle: the even lane stores its own sample and its neighbour's as 4 bytes, a wave's 128 bytes
// contiguous; a clip's last odd sample is stored alone.  Nothing is written past a clip's last kept sample.
#include <hip/hip_runtime.h>

#include "clip_device.h"
#include "clip_source_device.h"
#include "kernels.h"

namespace {

constexpr int kThreads = kStageThreads;

// the gather's tile of this workgroup: clip, outputs [o0, o0 + n_out) of it, source samples [e0, e0 + n) of the clip
struct StridedTile {
    uint32_t clip;
    uint64_t o0, e0;
    int n_out, n;
};

__device__ inline StridedTile strided_tile(const ClipArgs& c, uint32_t step, uint32_t tile_out)
{
    const uint32_t g = blockIdx.x;
    StridedTile t;
    t.clip = find_clip(c.tile_prefix, c.n_clips, g);
    const ClipJob j = c.jobs[t.clip];
    const uint64_t out_len = (j.len - j.skip + step - 1) / step;
    t.o0 = (uint64_t)(g - c.tile_prefix[t.clip]) * tile_out;
    t.n_out = (int)min((uint64_t)tile_out, out_len - t.o0);
    t.e0 = j.skip + t.o0 * step;
    t.n = (t.n_out - 1) * (int)step + 1; // <= (tile_out - 1) * step + 1 <= kClipTile, and e0 + n <= len
    return t;
}

// outputs [0, n_out) of a tile to out (16-byte aligned): output q is the staged tile's sample q * step, read by at(q * step)
template <typename D, typename S, typename At>
__device__ inline void store_strided(D* out, int n_out, int step, const S* lds, At at)
{
    const int t = threadIdx.x;
    for (int q0 = 0; q0 < n_out; q0 += kThreads) { // (the bound is the workgroup's: every lane of a wave takes part in the shuffle)
        const int q = q0 + t;
        D v{};
        if (q < n_out) v = Convert<D, S>::run(lds[at(q * step)]);
        if constexpr (sizeof(D) == 4) {
            if (q < n_out) out[q] = v;
        } else {
            const uint32_t lo = (uint16_t)v, hi = (uint32_t)__shfl_down((int)lo, 1, 64) & 0xffffu; // (lane t + 1 is q + 1: t is even)
            if ((t & 1) == 0 && q < n_out) {
                if (q + 1 < n_out) *reinterpret_cast<uint32_t*>(out + q) = lo | hi << 16; // q even, out 16-byte aligned
                else out[q] = v;                                                           // the clip's last sample
            }
        }
    }
}

} // namespace

template <typename D, typename S, typename B>
__global__ __launch_bounds__(kThreads) void clip_gather_strided_kernel(ClipStridedArgs<B> a)
{
    __shared__ __attribute__((aligned(16))) S lds[ClipSource<B>::template lds_elems<S>()];
    const ClipArgs& c = clip_args(a.s);
    const StridedTile t = strided_tile(c, a.step, a.tile_out);
    const uint32_t ch = (uint32_t)c.infos[t.clip].best_channel;
    // (the job's slot is read before the staging, so that its load is not waited for behind the barrier)
    D* out = static_cast<D*>(c.out) + c.jobs[t.clip].out_off + t.o0; // 16-byte aligned: the slot is, and tile_out is a multiple of 8
    // the tile's samples are counted from the clip's first sample (e0), so the stride runs through the seam of a split clip
    const auto at = ClipSource<B>::template stage<S>(a.s, t.clip, ch, t.e0, t.n, lds);
    store_strided<D, S>(out, t.n_out, (int)a.step, lds, at);
}

namespace {

template <typename B>
int launch(const ClipStridedArgs<B>& a, hipStream_t stream)
{
    return launch_clip_formats(clip_args(a.s), [&](auto d, auto s, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((clip_gather_strided_kernel<decltype(d), decltype(s), B>), grid, block, 0, stream, a);
    });
}

} // namespace

int fvad_launch_clip_gather_strided(const ClipStridedArgs<ClipArgs>& a, hipStream_t stream) { return launch(a, stream); }
int fvad_launch_clip_gather_strided(const ClipStridedArgs<ClipSplitArgs>& a, hipStream_t stream) { return launch(a, stream); }
