// kernels_egress_strided.hip -- fvad_egress_resample_strided*: kernels_egress_resample.hip over a STRIDED stream.  Stream sample
// s of channel c is lane sample src_off + c lane_stride + (s - frame_base) step: NSNet2's own 16 kHz output lies 3 apart in the
// 48 kHz lanes (K3 puts network sample j unchanged at lane index 3 j + 2 and lerps the two in front of it), and a recording made
// from that stream carries neither the lerp's droop nor its images.  Output o of a stream of stream_frames STRIDED samples is
//     y[o] = sum_j taps[r + j up] * x[q - j],   P = K + o down = q up + r,  j = 0 .. (2 K - r) / up,  K = (n_taps - 1) / 2,
// exactly kernels_egress_resample.hip's sum: the same ascending-j f32 fma chain from +0 with the zero extension skipped, the same
// conversion (Quant<F>), placement (Sink<F>::store) and drain_tile, the same tile (egress_resample_tile: the window is 8192
// STAGED samples whatever the step), per-channel loop and LDS-or-global tap table.  So the bytes are fvad_egress_resample's over
// a compacted copy of the lanes, and with step 1 over the lanes themselves.  What is new is the staging alone: for each channel
// the tile's window of n <= kClipTile stream samples is staged COMPACTED into win[] by stage_tile_strided, from the lane span of
// (n - 1) step + 1 samples at src_off + c lane_stride + (lo - frame_base) step (64-bit; inside the span (n - 1) step < 2^17 is
// 32-bit).  Only on-stride samples are loaded: no byte outside the span is read and no off-stride sample can reach an output.
// No atomics, no scratch.
//
// The staging's cost, computed.  Two forms read the span: dword loads `step` apart, or 16-byte contiguous loads of which only the
// on-stride words are written to LDS.  A 128-byte line holds 32 / step on-stride samples, so at step <= 32 both touch every line
// of the span once per tile: the same (n - 1) step / 32 + 1 lines through the vector cache, the same HBM bytes -- the lanes'
// bytes, what fvad_egress_resample reads for the same recording.  They differ in instructions.  Per lane and full window
// (n = 8192):
// - dword loads: 32 loads and 32 LDS writes whatever the step; a wavefront's load spans 64 step words = 2 step lines (6 at
//   step 3); the writes are 64 consecutive words, conflict-free (Guideline 4: ds_write_b32 is banked (a / 4) mod 32 within each
//   32-lane half);
// - 16-byte loads: 8 step loads (24 at step 3, 128 at step 16), 1 KB each, and min(4, ceil(4 / step) + 1) predicated LDS writes
//   per load (4 at step 3: 96), neighbouring writers 4 words apart at step 3: 11 lanes of a half over 44 words, 2-way on 3 banks;
//   plus stage_tile's head and tail.
// The dword form is taken: no more instructions at step 3 (64 against 120), fewer from step 4 on, no conflicts, no head or tail,
// and the read bound holds by construction.  It is the one place in the egress kernels where neighbouring lanes do not load
// neighbouring addresses.
//
// The rest of the LDS cost is kernels_egress_resample.hip's, unchanged (taps [j][o mod up]: conflict-free; window reads down / up
// samples apart; image writes C B bytes apart).  At 1/1 with one tap (a 16 kHz recording of the network's samples) an output
// is one window read, one fma and one image write.
// Occupancy, from the resource-usage output: 73 744 B of LDS with the table (2 workgroups of 4 wavefronts on a compute unit's
// 160 KB: 2 waves per SIMD), 49 168 B without (3); 48 VGPRs in all six instances (the staging loop's loads are unrolled and in
// flight together), no scratch.  LDS, not registers, sets the occupancy.
#include <hip/hip_runtime.h>

#include "egress_device.h"
#include "kernels.h"
#include "stage_tile_strided.h"

namespace {

constexpr int kThreads = kStageThreads;

// Quant<F>: the f32 result as the file sample's integer image (fvad_egress's rules for f32 lanes; kernels_egress_resample.hip's)
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
__global__ __launch_bounds__(kThreads) void egress_strided_kernel(EgressStridedArgs s)
{
    __shared__ float win[kClipTile];
    __shared__ __attribute__((aligned(16))) uint8_t img[kIngestTileBytes + 16];
    __shared__ float tab_lds[TL ? kClipResampleTableLds : 1];
    constexpr int B = Sink<F>::kBytes;
    const EgressResampleArgs& a = s.r;
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
        // the window's first sample in its lane: the check has made sure lo >= frame_base and that the span lies in the lane
        if (n > 0) stage_tile_strided(a.lanes + j.src_off + (uint64_t)c * a.lane_stride + (lo - j.frame_base) * s.step, n, s.step, win);
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
                    int b = (int)(q - j_first - lo); // q - j_last >= lo and q - j_first < lo + n: within the window
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
int launch(const EgressStridedArgs& s, hipStream_t stream)
{
    const dim3 grid(s.r.n_units), block(kThreads);
    if (s.r.file_format == FVAD_INGEST_F32) hipLaunchKernelGGL((egress_strided_kernel<float, TL>), grid, block, 0, stream, s);
    else if (s.r.file_format == FVAD_INGEST_PCM16) hipLaunchKernelGGL((egress_strided_kernel<int16_t, TL>), grid, block, 0, stream, s);
    else if (s.r.file_format == FVAD_INGEST_PCM24) hipLaunchKernelGGL((egress_strided_kernel<Pcm24, TL>), grid, block, 0, stream, s);
    else return (int)hipErrorInvalidValue; // (the callers refuse the formats before they get here)
    return (int)hipGetLastError();
}

} // namespace

int fvad_launch_egress_strided(const EgressStridedArgs& s, hipStream_t stream)
{
    const bool in_lds = (uint64_t)((s.r.n_taps + s.r.up - 1) / s.r.up) * s.r.up <= kClipResampleTableLds;
    return in_lds ? launch<true>(s, stream) : launch<false>(s, stream);
}
