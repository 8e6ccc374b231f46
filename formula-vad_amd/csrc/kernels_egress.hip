// kernels_egress.hip -- fvad_egress*: planar device lanes (f32 or PCM16) converted to a file's sample format and interleaved
// into the bytes of its data chunk -- little-endian PCM16, PCM24 or IEEE float32 frames -- the inverse of kernels_ingest.hip.
// The four format pairs: f32 -> f32 and PCM16 -> PCM16 move bits (f32 as 32-bit integers: NaN payloads and -0 survive);
// f32 -> PCM16 and f32 -> PCM24 are Quant<F> of egress_device.h.
//
// The work unit follows kernels_ingest.hip: a workgroup of 256 lanes takes one tile of one sink, found by a search of a
// host-built prefix table with its block index (the same in every lane); no atomics, a sink's bytes depend on its lanes alone.
// Every lane takes the samples of ONE channel of a group of consecutive frames: a group is 16 bytes of the SOURCE, cut at the
// source's 16-byte boundaries (a lane run's start has any element alignment: lane_stride and src_offset are arbitrary), so that
// a whole group is one 16-byte load and only a run's first and last few samples are element loads; consecutive lanes of the
// workgroup take consecutive groups of one channel (coalesced loads), and no sample outside the sink's lane range is read.
// Each sample is converted and placed into LDS at shift + (f * C + c) * B, shift the destination's address modulo 16, so that
// the tile's bytes lie in LDS as they will lie in memory; after a barrier they are drained (drain_tile: 16-byte stores for the
// aligned body strictly inside the tile, the bytes in front of and behind it one by one, so no byte outside the sink's range
// is written even where a neighbouring sink touches it).  Samples that are not aligned to their own size (a data chunk at an
// odd offset, f32 frames at 2 modulo 4) and all PCM24 samples are written as LDS bytes: no unaligned LDS access.
//
// LDS cost, computed (cdna_hip_programming Guideline 4; every ds_write banks by (a / 4) mod 32 within a half-wave): the writes
// of a lane's group are C * B bytes apart and the groups of neighbouring lanes G * C * B (G = 4 samples of an f32 lane, 8 of a
// PCM16 lane).  Mono f32 -> f32: a lane's four ds_write_b32 are 4 bytes apart, neighbouring lanes 16 bytes = 4 banks, so the
// 32 lanes of a half-wave fall on 8 banks: a 4-way conflict.  Stereo f32 -> PCM16: a lane's four ds_write_b16 are 4 bytes
// apart, neighbouring lanes again 16 bytes: 4-way as well (the two channels of a frame share a dword, but they are written by
// lanes ng groups apart, hardly ever by one instruction).  Does a kernel that moves 6 to 8 bytes of HBM per sample have the
// cycles?  A mono f32 tile is 4096 samples: 64 wave-level ds_write_b32 at 4 cycles, 4-way: about 1000 LDS cycles, plus 16
// ds_read_b128 of the drain; its 32 KB of HBM traffic take a compute unit's share of 6.29 TB/s (10 bytes per clock at 2.4 GHz)
// some 3200 cycles.  A stereo PCM16 tile is 8192 samples: 128 ds_write_b16, about 2000 cycles against 4800 for its 48 KB.
// PCM24 writes three bytes per sample (mono: neighbouring lanes 12 bytes = 3 banks apart, conflict-free; a tile of 5460 samples
// is 256 wave-level ds_write_b8, some 1000 cycles against 3800 for its 38 KB).  So the LDS work fits under the memory time in
// every pair, with several workgroups per compute unit to overlap the two -- a computed statement until measured
// (tools/egress_time.py reports the kernel's rate).
#include <hip/hip_runtime.h>

#include "egress_device.h"
#include "kernels.h"

namespace {

constexpr int kThreads = kStageThreads;

// Encode<F, S>: the lane element loaded (E, an integer image) and the file sample's integer image made from it: PCM16 lanes as
// they are, f32 lanes by Quant<F> (f32 -> f32: the bits go through two casts and no arithmetic)
template <typename F, typename S> struct Encode;
template <> struct Encode<int16_t, int16_t> { using E = uint16_t; __device__ static uint32_t run(E s) { return s; } };
template <typename F> struct Encode<F, float> { using E = uint32_t; __device__ static uint32_t run(E s) { return Quant<F>::run(__uint_as_float(s)); } };

template <typename F, typename S>
__device__ inline void egress_tile(const EgressArgs& a, uint8_t* lds)
{
    using E = typename Encode<F, S>::E;
    constexpr int G = 16 / (int)sizeof(E);
    constexpr int B = Sink<F>::kBytes;
    const uint32_t u = blockIdx.x;
    const uint32_t ji = find_job(a.unit_prefix, a.n_jobs, u);
    const EgressJob j = a.jobs[ji];
    const uint32_t r = u - a.unit_prefix[ji];
    const int t = threadIdx.x;
    const int C = (int)j.n_channels;
    const uint64_t f0 = (uint64_t)r * j.tile_frames;
    const int nfr = (int)min((uint64_t)j.tile_frames, j.n_frames - f0);
    uint8_t* dst = a.out + j.dst_off + f0 * (uint64_t)(C * B);
    const int shift = (int)((uintptr_t)dst & 15);
    // a frame is C * B bytes, so every sample of the tile has frame 0's alignment
    const bool aligned = B == 3 ? false : (shift % B) == 0;
    const E* lanes = static_cast<const E*>(a.lanes) + j.src_off + f0;
    const int ng = (nfr + 2 * G - 2) / G; // groups a run of nfr can touch, whatever its alignment
    for (int i = t; i < C * ng; i += kThreads) {
        const int c = i / ng, g = i - c * ng;
        uint8_t* at = lds + shift + c * B;
        load_group(lanes + (uint64_t)c * a.lane_stride, nfr, g, [&](int f, E s) { Sink<F>::store(at, f * C * B, aligned, Encode<F, S>::run(s)); });
    }
    __syncthreads();
    drain_tile(dst, nfr * C * B, shift, lds);
}

} // namespace

template <typename F, typename S>
__global__ __launch_bounds__(kThreads) void egress_kernel(EgressArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kIngestTileBytes + 16];
    egress_tile<F, S>(a, lds);
}

int fvad_launch_egress(const EgressArgs& a, hipStream_t stream)
{
    const dim3 grid(a.n_units), block(kThreads);
    if (a.src_format == FVAD_INGEST_F32)
        return launch_file_format(a.file_format, [&](auto f) { hipLaunchKernelGGL((egress_kernel<decltype(f), float>), grid, block, 0, stream, a); });
    if (a.src_format != FVAD_INGEST_PCM16 || a.file_format != FVAD_INGEST_PCM16) return (int)hipErrorInvalidValue; // (the callers refuse the conversions before they get here)
    hipLaunchKernelGGL((egress_kernel<int16_t, int16_t>), grid, block, 0, stream, a);
    return (int)hipGetLastError();
}
