// kernels_ingest_resample.hip -- fvad_ingest_resample*: a file at another rate decoded, de-interleaved, filtered and re-timed into
// 48 kHz f32 lanes in one pass, a rational up/down polyphase resampler inside the ingest (the definition: include/fvad.h).
//   y[o] = sum_j taps[r + j up] * x[q - j],   q = (K + o down) / up,  r = (K + o down) % up,  j = 0 .. (2 K - r) / up,
// one f32 fma chain from +0 in ascending j: the order depends on (up, down, n_taps, o mod up) alone, so an output's bits do not
// depend on the source's cut, the tile, the call form or the destination.
//
// The work unit is kernels_ingest.hip's: a workgroup of 256 lanes takes one tile of one source (tile_out consecutive outputs
// of every channel), found by a search of a host-built prefix table; no atomics.  The window of source frames the tile's
// outputs read, clipped to the file, is staged through LDS once with stage_tile (no byte outside the given frames is read:
// fvad_ingest_resample_check made them cover the window); then every lane takes groups of 4 consecutive outputs of ONE channel
// -- 16 destination bytes cut at the destination's 16-byte boundaries (store_group), consecutive lanes consecutive groups --
// decodes each sample it needs from LDS and walks its phase's taps.
// - The branch table lives in GLOBAL memory (up to 80 KB: L2-resident, the phases a tile walks mostly in the CU's 32 KB L1),
//   not in LDS, which the window has (a tile of 16 KB lets several workgroups share a CU; 80 KB of taps beside it would not).
// - Its layout is [j][o mod up] (resample_table of resample.h): the lanes of a wavefront, whose outputs are 4 apart, read
//   words 4 apart (wrapping at up) -- 64 lanes touch 1 KB, 8 lines of 128 bytes, and the group's other three outputs the same
//   lines.  A table indexed by r would scatter them with stride 4 (down mod up) over all of it.
// - The LDS reads of a lane walk backwards through its channel's samples, n_channels * bytes_per_sample apart; neighbouring
//   lanes start 4 down / up frames apart.  For mono PCM16 at 160/147 that is 7.35 bytes: the 32 lanes of a ds_read group cover
//   59 consecutive words, 2-byte reads of one word broadcast -- at most 2-way conflicts (the group spans fewer than 64 banks
//   read as 32).  For wide frames (stride a multiple of 128 bytes) every lane of a group is on one bank: correct, not fast.
// - The tile (resample_tile): the most outputs, in fours, whose window fits 16 KB of staged bytes -- the window carries
//   2 K / up frames of reach --, 4096 at most; where that leaves fewer than 64 outputs (wide frames, long filters) the most
//   that fit 64 KB.  The LDS is dynamic: a launch asks for the largest window of its jobs.
// - The file-edge zeros are SKIPPED (the j range is cut to the file).  With finite taps multiplying them gives the same bits:
//   fma(t, 0, acc) is acc, and +0 for acc = +0.
// - The zero-fill range behind a source's outputs is tiled as in kernels_ingest.hip.
#include <hip/hip_runtime.h>

#include "ingest_device.h"
#include "kernels.h"
#include "stage_tile.h"

namespace {

constexpr int kThreads = kStageThreads;

template <typename S>
__device__ inline void resample_tile(const IngestResampleArgs& a, uint8_t* lds)
{
    constexpr int G = 4;
    constexpr int B = Source<S>::kBytes;
    uint32_t r;
    const IngestResampleJob j = find_unit(a.jobs, a.unit_prefix, a.n_jobs, blockIdx.x, &r);
    float* lanes = a.lanes + j.dst_off;
    const int t = threadIdx.x;
    if (r >= j.n_data_tiles) return fill_tile(lanes, a.lane_stride, j.n_out, j.fill_len, j.n_fill_tiles, r - j.n_data_tiles);
    const int C = (int)j.n_channels, FB = C * B;
    const uint32_t up = a.up, down = a.down, taps_last = a.n_taps - 1; // taps_last = 2 K
    const uint64_t i0 = (uint64_t)r * j.tile_out;
    const int n = (int)min((uint64_t)j.tile_out, j.n_out - i0);
    // the tile's first output: P = K + o down = q up + r; o mod up (all below 2^63: file_frames * up < 2^62)
    const uint64_t o0 = j.out_from + i0;
    const uint64_t P0 = o0 * down + taps_last / 2;
    const uint64_t q0 = P0 / up;
    const uint32_t r0 = (uint32_t)(P0 % up), om0 = (uint32_t)(o0 % up);
    // its window [lo, hi) of the file's frames: the first output's first frame to the last output's last, clipped
    const uint64_t P1 = P0 + (uint64_t)(n - 1) * down;
    const uint64_t lo = min(P0 > taps_last ? (P0 - taps_last + up - 1) / up : 0, j.file_frames);
    const uint64_t hi = min(P1 / up + 1, j.file_frames);
    const uint8_t* src = a.raw + j.src_off + (lo - j.frame_base) * (uint64_t)FB; // (never dereferenced when the window is empty)
    int shift = 0;
    if (hi > lo) shift = stage_tile(src, (int)(hi - lo) * FB, lds);
    // a frame is C * B bytes, so every sample of the source has this frame's alignment
    const bool aligned = B == 3 ? false : ((uintptr_t)src % B) == 0;
    const int ng = (n + 2 * G - 2) / G;
    for (int i = t; i < C * ng; i += kThreads) {
        const int c = i / ng, g = i - c * ng;
        float* p = lanes + (uint64_t)c * a.lane_stride + i0;
        const uint8_t* at = lds + shift + c * B;
        store_group(p, n, g, [&](int e) {
            const uint64_t d = (uint64_t)e * down + r0;
            uint64_t qd;
            uint32_t rr;
            if (d <= 0xffffffffu) { qd = (uint32_t)d / up; rr = (uint32_t)d % up; } else { qd = d / up; rr = (uint32_t)(d % up); }
            if (rr > taps_last) return 0.0f; // a phase without taps (up > n_taps)
            const uint64_t q = q0 + qd;
            const uint32_t om = (om0 + (uint32_t)e) % up;
            // frames q - jj, jj = 0 .. (2 K - rr) / up, inside the file [0, file_frames)
            const uint64_t j_last = min((uint64_t)((taps_last - rr) / up), q);
            const uint64_t j_first = q >= j.file_frames ? q - j.file_frames + 1 : 0;
            float acc = 0.0f;
            if (j_first > j_last) return acc; // every frame of the phase lies outside the file
            // (32-bit from here: j_last <= 2 K / up, and frames q - j_first .. q - j_last lie within the staged window)
            const int n_terms = (int)(j_last - j_first) + 1;
            const float* tp = a.table + om + (uint32_t)j_first * up;
            int b = (int)(q - j_first - lo) * FB;
            for (int k = 0; k < n_terms; ++k, tp += up, b -= FB) acc = __builtin_fmaf(*tp, decode_f32<S>(Source<S>::load(at, b, aligned)), acc);
            return acc;
        });
    }
}

} // namespace

template <typename S>
__global__ __launch_bounds__(kThreads) void ingest_resample_kernel(IngestResampleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    resample_tile<S>(a, lds);
}

int fvad_launch_ingest_resample(const IngestResampleArgs& a, hipStream_t stream)
{
    const dim3 grid(a.n_units), block(kThreads);
    if (a.lds_bytes > 65536) return (int)hipErrorInvalidValue;
    if (a.src_format == FVAD_INGEST_PCM16) hipLaunchKernelGGL((ingest_resample_kernel<int16_t>), grid, block, a.lds_bytes, stream, a);
    else if (a.src_format == FVAD_INGEST_PCM24) hipLaunchKernelGGL((ingest_resample_kernel<Pcm24>), grid, block, a.lds_bytes, stream, a);
    else if (a.src_format == FVAD_INGEST_F32) hipLaunchKernelGGL((ingest_resample_kernel<float>), grid, block, a.lds_bytes, stream, a);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}
