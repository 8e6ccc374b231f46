// kernels_ingest.hip -- fvad_ingest*: a corpus's bytes as its files hold them (interleaved frames of little-endian PCM16, PCM24
// or IEEE float32) de-interleaved, decoded and zero-padded into the planar lanes fvad_engine_enqueue_device* and
// fvad_clips_export* take.  The four format pairs are exact: PCM16 -> f32 is s / 32768 (fvad_lane.pcm_i16's rule), PCM24 -> f32
// is s / 8388608 (|s| <= 2^23 fits the f32 significand, the scale is a power of two), PCM16 -> PCM16 and f32 -> f32 move bits
// (f32 as 32-bit integers: NaN payloads and -0 survive).
//
// The work unit follows kernels_clips.hip: a workgroup of 256 lanes takes one tile of one source, found by a search of a
// host-built prefix table with its block index (the same in every lane); no atomics, a source's output depends on its own bytes
// alone.  A data tile's bytes are staged through LDS once (stage_tile: 16-byte loads for the aligned body strictly inside the
// tile, the bytes in front of and behind it one by one, so no byte outside the source's range is read); then every lane takes
// the samples of ONE channel of a group of consecutive frames from LDS by index and stores them planar.  A group is 16 bytes of
// the DESTINATION, cut at the destination's 16-byte boundaries (a lane's start has any element alignment: lane_stride and
// dst_offset are arbitrary), so that a whole group is one 16-byte store and only a run's first and last few samples are
// element stores; consecutive lanes of the workgroup take consecutive groups of one channel (coalesced stores).  The LDS reads
// of a group are n_channels * bytes_per_sample apart and the groups of neighbouring lanes 16 destination bytes' worth of frames:
// for mono f32 that is a 4-way bank conflict on ds_read_b32 (computed, cdna_hip_programming Guideline 4), which a kernel that
// moves 8 bytes of HBM per sample has the LDS cycles for.  Samples that are not aligned to their own size (a data chunk at
// an odd offset, f32 frames at 2 modulo 4) and all PCM24 samples are assembled from LDS bytes: no unaligned LDS access.
// The zero-fill range behind a source's frames is tiled the same way, one lane's zeros per unit.
#include <hip/hip_runtime.h>

#include "ingest_device.h"
#include "kernels.h"
#include "stage_tile.h"

namespace {

constexpr int kThreads = kStageThreads;

// Decode<D, S>: the element stored (E) from the integer image.  Into f32 lanes decode_f32's value; the two pairs of one format
// move bits as integers (f32: NaN payloads and -0 survive whatever the float unit would do with them).
template <typename D, typename S> struct Decode;
template <typename S> struct Decode<float, S> { using E = float; __device__ static E run(int32_t s) { return decode_f32<S>(s); } };
template <> struct Decode<int16_t, int16_t> { using E = int16_t; __device__ static E run(int32_t s) { return (int16_t)s; } };
template <> struct Decode<float, float> { using E = uint32_t; __device__ static E run(int32_t s) { return (uint32_t)s; } }; // the bits

template <typename D, typename S>
__device__ inline void ingest_tile(const IngestArgs& a, uint8_t* lds)
{
    using E = typename Decode<D, S>::E;
    constexpr int G = 16 / (int)sizeof(E);
    constexpr int B = Source<S>::kBytes;
    uint32_t r;
    const IngestJob j = find_unit(a.jobs, a.unit_prefix, a.n_jobs, blockIdx.x, &r);
    E* lanes = static_cast<E*>(a.lanes) + j.dst_off;
    const int t = threadIdx.x;
    if (r >= j.n_data_tiles) return fill_tile(lanes, a.lane_stride, j.n_frames, j.fill_len, j.n_fill_tiles, r - j.n_data_tiles);
    const int C = (int)j.n_channels;
    const uint64_t f0 = (uint64_t)r * j.tile_frames;
    const int nfr = (int)min((uint64_t)j.tile_frames, j.n_frames - f0);
    const uint8_t* src = a.raw + j.src_off + f0 * (uint64_t)(C * B);
    const int shift = stage_tile(src, nfr * C * B, lds);
    // a frame is C * B bytes, so every sample of the source has frame 0's alignment
    const bool aligned = B == 3 ? false : ((uintptr_t)src % B) == 0;
    const int ng = (nfr + 2 * G - 2) / G;
    for (int i = t; i < C * ng; i += kThreads) {
        const int c = i / ng, g = i - c * ng;
        E* p = lanes + (uint64_t)c * a.lane_stride + f0;
        const uint8_t* at = lds + shift + c * B;
        store_group(p, nfr, g, [&](int f) { return Decode<D, S>::run(Source<S>::load(at, f * C * B, aligned)); });
    }
}

} // namespace

template <typename D, typename S>
__global__ __launch_bounds__(kThreads) void ingest_kernel(IngestArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kIngestTileBytes + 16];
    ingest_tile<D, S>(a, lds);
}

int fvad_launch_ingest(const IngestArgs& a, hipStream_t stream)
{
    const dim3 grid(a.n_units), block(kThreads);
    if (a.src_format == FVAD_INGEST_PCM16 && a.out_i16) hipLaunchKernelGGL((ingest_kernel<int16_t, int16_t>), grid, block, 0, stream, a);
    else if (a.src_format == FVAD_INGEST_PCM16) hipLaunchKernelGGL((ingest_kernel<float, int16_t>), grid, block, 0, stream, a);
    else if (a.src_format == FVAD_INGEST_PCM24 && !a.out_i16) hipLaunchKernelGGL((ingest_kernel<float, Pcm24>), grid, block, 0, stream, a);
    else if (a.src_format == FVAD_INGEST_F32 && !a.out_i16) hipLaunchKernelGGL((ingest_kernel<float, float>), grid, block, 0, stream, a);
    else return (int)hipErrorInvalidValue; // (the callers refuse the conversions before they get here)
    return (int)hipGetLastError();
}
