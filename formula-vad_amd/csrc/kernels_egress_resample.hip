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
#include <hip/hip_runtime.h>

#include "egress_device.h"
#include "kernels.h"

namespace {

constexpr int kThreads = kStageThreads;

// Quant<F>: the f32 result as the file sample's integer image (fvad_egress's rules for f32 lanes)
template <typename F> struct Quant;
template <> struct Quant<float> { __device__ static uint32_t run(float y) { return __float_as_uint(y); } };
template <> struct Quant<int16_t> {
    __device__ static uint32_t run(float y) { return (uint32_t)(int32_t)__builtin_rintf(fminf(fmaxf(y * 32768.0f, -32768.0f), 32767.0f)); }
};
template <> struct Quant<Pcm24> {
    __device__ static uint32_t run(float y) { return (uint32_t)(int32_t)__builtin_rintf(fminf(fmaxf(y * 8388608.0f, -8388608.0f), 8388607.0f)); }
};

} // namespace

template <typename F, bool TL>
__global__ __launch_bounds__(kThreads) void egress_resample_kernel(EgressResampleArgs a)
{
    __shared__ __attribute__((aligned(16))) float win[kClipTile + 4];
    __shared__ __attribute__((aligned(16))) uint8_t img[kIngestTileBytes + 16];
    __shared__ float tab_lds[TL ? kClipResampleTableLds : 1];
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
        int ws = 0;
        if (n > 0) ws = stage_tile(a.lanes + j.src_off + (uint64_t)c * a.lane_stride + (lo - j.frame_base), n, win);
        else __syncthreads();
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

namespace {

template <bool TL>
int launch(const EgressResampleArgs& a, hipStream_t stream)
{
    const dim3 grid(a.n_units), block(kThreads);
    if (a.file_format == FVAD_INGEST_F32) hipLaunchKernelGGL((egress_resample_kernel<float, TL>), grid, block, 0, stream, a);
    else if (a.file_format == FVAD_INGEST_PCM16) hipLaunchKernelGGL((egress_resample_kernel<int16_t, TL>), grid, block, 0, stream, a);
    else if (a.file_format == FVAD_INGEST_PCM24) hipLaunchKernelGGL((egress_resample_kernel<Pcm24, TL>), grid, block, 0, stream, a);
    else return (int)hipErrorInvalidValue; // (the callers refuse the formats before they get here)
    return (int)hipGetLastError();
}

} // namespace

int fvad_launch_egress_resample(const EgressResampleArgs& a, hipStream_t stream)
{
    const bool in_lds = (uint64_t)((a.n_taps + a.up - 1) / a.up) * a.up <= kClipResampleTableLds;
    return in_lds ? launch<true>(a, stream) : launch<false>(a, stream);
}
