// kernels_egress_resample.hip -- fvad_egress_resample*: planar f32 device lanes at 48 kHz resampled by up/down, converted to a
// file's sample format and interleaved into the bytes of its data chunk: kernels_egress.hip with the polyphase resampler of
// kernels_clips_resample.hip in front of its conversion.  Output o of a STREAM of stream_frames lane samples is
//     y[o] = sum_j taps[r + j up] * x[q - j],   P = K + o down = q up + r,  j = 0 .. (2 K - r) / up,  K = (n_taps - 1) / 2,
// x the stream's samples of one lane, 0 outside [0, stream_frames), one f32 fma chain from +0 in ascending j (resample_run's
// chain: the order depends on up, down, n_taps, stream_frames and o alone, never on the row, the tile or the file's format, so
// a stream's bytes do not depend on how it is cut, and a PCM file holds the conversion of the f32 file's values).  o is counted
// from the STREAM's first sample: a row names its outputs [out_from, out_from + n_out) and the stream samples its lanes hold
// [frame_base, ...) apart; the host's check has made sure the latter cover the window of the former, so a tile's window lies
// inside the given frames and nothing else of a lane is read.  The zero extension is SKIPPED, not stored: the j range of an
// output is cut to [0, stream_frames) (finite taps: the bits multiplying the zeros would give).
//
// Work unit: a tile of tile_out OUTPUT frames of one row (egress_resample_tile of egress_resample.h: a multiple of 4 whose bytes
// fit kIngestTileBytes and whose window of one channel fits kClipTile lane samples; at 147/160 with 5121 taps mono f32 and stereo
// PCM16 4096, mono PCM16 7492), found by a search of the host-built prefix table with the block index; 256 lanes.  For each
// channel in turn the tile's window [ceil((o_first down - K) / up), floor((o_last down + K) / up)], clipped to the stream, is
// staged by stage_tile as it is, the channel's outputs are computed -- consecutive lanes take consecutive outputs, lane l the
// outputs l, l + 256, ... --, converted (fvad_egress's rules for f32 lanes) and placed with Sink<F>::store at
// shift + (f C + c) B of the tile's LDS byte image, shift the destination's address modulo 16; after the last channel a barrier
// and drain_tile (16-byte stores strictly inside the tile, single bytes at its ends: no byte outside the row's range is
// written, also where another row touches it).  So LDS does not depend on the channel count: the window (32 KB), the image
// (16 KB) and the tap table (24 KB, or none).  Index arithmetic is 64-bit per tile (P0, q0, the window) and 32-bit inside it
// (e down + r0 < kClipTile * up < 2^23).  Samples not aligned to their own size and all PCM24 samples go as LDS bytes: no
// unaligned LDS access.  No atomics, no scratch.
//
// LDS cost, computed (cdna_hip_programming Guideline 4: a 4-byte access is banked (a / 4) mod 32 within each 32-lane half).
// - The taps are laid out [j][o mod up] (resample_table): at step j a wavefront reads 64 consecutive words (wrapping at up;
//   up < 64: equal words, a broadcast): conflict-free.  The table is in LDS when it has at most kClipResampleTableLds entries
//   (147/160 with 5121 taps: 35 x 147 words), else in global memory (147/320 with 10241: 70 x 147), two or three 128-byte lines
//   a wavefront and step.
// - The window reads of neighbouring lanes are down / up samples apart and every lane steps one sample back per j, the same
//   pattern at every j: up >= down conflict-free (a half spans at most 32 words, equal words broadcast); 160/147: 34.8 words,
//   2-way on at most 3 banks; 3/1: stride 3, odd, conflict-free; 320/147: 69.7 words, 3-way.  Left as they are, as in the clips.
// - The image writes are one per output against (2 K + 1) / up window reads (35 at 147/160): neighbouring lanes C B bytes
//   apart.  Mono f32 and stereo PCM16: 4 bytes, conflict-free; mono PCM16: two lanes a word, 2-way at most; PCM24: byte writes 3 C
//   bytes apart; C channels of f32: gcd(C, 32)-way (64 channels: every lane of a half on one bank, 32-way, on 1 / 35 of the
//   LDS instructions).
// Occupancy: 72.0 KB of LDS with the table (2 workgroups of 4 wavefronts on a compute unit's 160 KB), 48.0 KB without (3).
//
// fvad_egress_resample_strided* (egress_strided_kernel) is the same tile body over a STRIDED stream.  Stream sample s of channel
// c is lane sample src_off + c lane_stride + (s - frame_base) step: NSNet2's own 16 kHz output lies 3 apart in the 48 kHz lanes
// (K3 puts network sample j unchanged at lane index 3 j + 2 and lerps the two in front of it), and a recording made from that
// stream carries neither the lerp's droop nor its images.  The sum, its ascending-j f32 fma chain from +0 with the zero extension
// skipped, the conversion (Quant<F>), placement (Sink<F>::store) and drain_tile, the tile (egress_resample_tile: the window is
// 8192 STAGED samples whatever the step), the per-channel loop and the LDS-or-global tap table are one text below (polyphase_tile),
// every count in STRIDED samples.  So the bytes are fvad_egress_resample's over a compacted copy of the lanes, and with step 1
// over the lanes themselves.  What differs is the staging alone, under `if constexpr (kStrided)`: for each channel the tile's
// window of n <= kClipTile stream samples is staged COMPACTED into win[] by stage_tile_strided, from the lane span of
// (n - 1) step + 1 samples at src_off + c lane_stride + (lo - frame_base) step (64-bit; inside the span (n - 1) step < 2^17 is
// 32-bit).  Only on-stride samples are loaded: no byte outside the span is read and no off-stride sample can reach an output.
//
// The strided staging's cost, computed.  Two forms read the span: dword loads `step` apart, or 16-byte contiguous loads of which
// only the on-stride words are written to LDS.  A 128-byte line holds 32 / step on-stride samples, so at step <= 32 both touch
// every line of the span once per tile: the same (n - 1) step / 32 + 1 lines through the vector cache, the same HBM bytes -- the
// lanes' bytes, what fvad_egress_resample reads for the same recording.  They differ in instructions.  Per lane and full window
// (n = 8192):
// - dword loads: 32 loads and 32 LDS writes whatever the step; a wavefront's load spans 64 step words = 2 step lines (6 at
//   step 3); the writes are 64 consecutive words, conflict-free (Guideline 4: ds_write_b32 is banked (a / 4) mod 32 within each
//   32-lane half);
// - 16-byte loads: 8 step loads (24 at step 3, 128 at step 16), 1 KB each, and min(4, ceil(4 / step) + 1) predicated LDS writes
//   per load (4 at step 3: 96), neighbouring writers 4 words apart at step 3: 11 lanes of a half over 44 words, 2-way on 3 banks;
//   plus stage_tile's head and tail.
// The dword form is taken: no more instructions at step 3 (64 against 120), fewer from step 4 on, no conflicts, no head or tail,
// and the read bound holds by construction.  It is the one place in the egress kernels where neighbouring lanes do not load
// neighbouring addresses.  The rest of the LDS cost is the plain kernel's, unchanged; at 1/1 with one tap (a 16 kHz recording of
// the network's samples) an output is one window read, one fma and one image write.
// Occupancy of the strided kernel, from the resource-usage output: 73 744 B of LDS with the table (2 workgroups: 2 waves per
// SIMD), 49 168 B without (3); 48 VGPRs in all six instances (the staging loop's loads are unrolled and in flight together), no
// scratch.  LDS, not registers, sets the occupancy.
#include <hip/hip_runtime.h>

#include "egress_device.h"
#include "kernels.h"
#include "stage_tile_strided.h"

namespace {

constexpr int kThreads = kStageThreads;

// One tile of either kernel: win[] holds a channel's window (kClipTile samples, and stage_tile's 4 of alignment slack in the
// plain kernel), img[] the tile's byte image, tab_lds[] the tap table when TL.  `step` is read by the strided kernel alone.
template <typename F, bool TL, bool kStrided>
__device__ inline void polyphase_tile(const EgressResampleArgs& a, uint32_t step, float* win, uint8_t* img, float* tab_lds)
{
    constexpr int B = Sink<F>::kBytes;
    const uint32_t u = blockIdx.x;
    const uint32_t ji = find_job(a.unit_prefix, a.n_jobs, u);
    const EgressResampleJob j = a.jobs[ji];
    const int tid = threadIdx.x;
    const int C = (int)j.n_channels;
    const uint32_t up = a.up, down = a.down, taps_last = a.n_taps - 1; // 2 K
    // the tile's outputs [o0, o0 + n_out) of the stream; its first: K + o0 down = q0 up + r0
    // (all below 2^63: the check refuses stream_frames * up >= 2^62)
    const uint64_t e0 = (uint64_t)(u - a.unit_prefix[ji]) * j.tile_out;
    const int n_out = (int)min((uint64_t)j.tile_out, j.n_out - e0);
    const uint64_t o0 = j.out_from + e0, len = j.stream_frames;
    const uint64_t P0 = o0 * down + taps_last / 2, P1 = P0 + (uint64_t)(n_out - 1) * down;
    const uint64_t q0 = P0 / up;
    const uint32_t r0 = (uint32_t)(P0 % up), om0 = (uint32_t)(o0 % up);
    // the stream samples [lo, lo + n) are the tile's window (n may be 0: a filter shorter than up leaves outputs without a term)
    const uint64_t lo = min(P0 > taps_last ? (P0 - taps_last + up - 1) / up : 0, len);
    const uint64_t hi = min(P1 / up + 1, len);
    const int n = hi > lo ? (int)(hi - lo) : 0; // <= floor(((tile_out - 1) down + 2 K) / up) + 1 <= kClipTile
    const float* tab = a.table;
    if constexpr (TL) {
        const int nt = (int)((a.n_taps + up - 1) / up * up);
        for (int i = tid; i < nt; i += kThreads) tab_lds[i] = a.table[i];
        tab = tab_lds; // (the staging's barrier, or the one below, orders it before the reads)
    }
    uint8_t* dst = a.out + j.dst_off + e0 * (uint64_t)(C * B);
    const int shift = (int)((uintptr_t)dst & 15);
    // a frame is C * B bytes, so every sample of the tile has frame 0's alignment
    const bool aligned = B == 3 ? false : (shift % B) == 0;
    for (int c = 0; c < C; ++c) {
        if (c) __syncthreads(); // the previous channel's window is read
        // the window's first sample in its lane: the check has made sure lo >= frame_base and that the window (strided: its
        // span) lies in the lane.  ws: where stage_tile put it in win[]; the strided staging compacts it to win[0]
        int ws = 0;
        if constexpr (kStrided) {
            if (n > 0) stage_tile_strided(a.lanes + j.src_off + (uint64_t)c * a.lane_stride + (lo - j.frame_base) * step, n, step, win);
            else __syncthreads();
        } else {
            if (n > 0) ws = stage_tile(a.lanes + j.src_off + (uint64_t)c * a.lane_stride + (lo - j.frame_base), n, win);
            else __syncthreads();
        }
        uint8_t* at = img + shift + c * B;
        for (int e = tid; e < n_out; e += kThreads) {
            float acc = 0.0f;
            // 32-bit: e down + r0 <= (tile_out - 1) down + up - 1 < kClipTile * up
            const uint32_t d = (uint32_t)e * down + r0, qd = d / up, rr = d - qd * up;
            if (rr <= taps_last) {
                const uint64_t q = q0 + qd;
                // stream samples q - jj, jj = 0 .. (2 K - rr) / up, inside [0, len)
                const uint64_t j_last = min((uint64_t)((taps_last - rr) / up), q);
                const uint64_t j_first = q >= len ? q - len + 1 : 0;
                if (j_first <= j_last) {
                    const int n_terms = (int)(j_last - j_first) + 1;
                    const uint32_t om = (om0 + (uint32_t)e) % up;
                    const float* tp = tab + om + (uint32_t)j_first * up;
                    int b = ws + (int)(q - j_first - lo); // q - j_last >= lo and q - j_first < lo + n: within the window
#pragma unroll 4
                    for (int i = 0; i < n_terms; ++i, tp += up, --b) acc = __builtin_fmaf(*tp, win[b], acc);
                }
            }
            Sink<F>::store(at, e * C * B, aligned, Quant<F>::run(acc));
        }
    }
    __syncthreads();
    drain_tile(dst, n_out * C * B, shift, img);
}

} // namespace

template <typename F, bool TL>
__global__ __launch_bounds__(kThreads) void egress_resample_kernel(EgressResampleArgs a)
{
    __shared__ __attribute__((aligned(16))) float win[kClipTile + 4];
    __shared__ __attribute__((aligned(16))) uint8_t img[kIngestTileBytes + 16];
    __shared__ float tab_lds[TL ? kClipResampleTableLds : 1];
    polyphase_tile<F, TL, false>(a, 0, win, img, tab_lds);
}

template <typename F, bool TL>
__global__ __launch_bounds__(kThreads) void egress_strided_kernel(EgressStridedArgs s)
{
    __shared__ float win[kClipTile];
    __shared__ __attribute__((aligned(16))) uint8_t img[kIngestTileBytes + 16];
    __shared__ float tab_lds[TL ? kClipResampleTableLds : 1];
    polyphase_tile<F, TL, true>(s.r, s.step, win, img, tab_lds);
}

namespace {

template <typename F, bool TL> auto kernel_of(const EgressResampleArgs&) { return egress_resample_kernel<F, TL>; }
template <typename F, bool TL> auto kernel_of(const EgressStridedArgs&) { return egress_strided_kernel<F, TL>; }

// args: a kernel's argument, r: the EgressResampleArgs in it.  The tap table is staged in LDS when it fits there.
template <typename A>
int launch(const A& args, const EgressResampleArgs& r, hipStream_t stream)
{
    const dim3 grid(r.n_units), block(kThreads);
    const bool in_lds = (uint64_t)((r.n_taps + r.up - 1) / r.up) * r.up <= kClipResampleTableLds;
    return launch_file_format(r.file_format, [&](auto f) {
        using F = decltype(f);
        hipLaunchKernelGGL((in_lds ? kernel_of<F, true>(args) : kernel_of<F, false>(args)), grid, block, 0, stream, args);
    });
}

} // namespace

int fvad_launch_egress_resample(const EgressResampleArgs& a, hipStream_t stream) { return launch(a, a, stream); }
int fvad_launch_egress_strided(const EgressStridedArgs& s, hipStream_t stream) { return launch(s, s.r, stream); }
