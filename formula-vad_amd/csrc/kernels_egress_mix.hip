// kernels_egress_mix.hip -- fvad_egress_mix*: TWO sets of planar f32 device lanes, the original and the denoised, weighted,
// summed, converted to a file's sample format and interleaved into the bytes of its data chunk: kernels_egress.hip with a second
// source.  For frame f and channel c of a sink
//     y = den[first_lane + c][src_offset + f],   x = f < orig_zeros ? +0.0f : orig[first_lane + c][orig_offset + (f - orig_zeros)],
//     v = w_den * y             (w_orig == 0: the original lanes are never dereferenced)
//     v = w_orig * x            (w_den == 0: the denoised lanes are never dereferenced)
//     v = w_orig * x + w_den * y   otherwise: two f32 products and one f32 sum, each rounded (__fmul_rn / __fadd_rn: no fma),
// and v goes out as fvad_egress writes an f32 lane sample: its bits, or rint(fminf(fmaxf(v * scale, -scale), scale - 1)).  The
// kernel knows nothing of NSNet2's delay: the row states the pairing, so a time slice pairs its own buffers.
//
// The work unit is kernels_egress.hip's: a workgroup of 256 lanes takes one 16 KB destination tile of one sink, found with
// find_job; every lane takes ONE channel of a group of four consecutive frames; each sample goes to LDS at shift + (f C + c) B,
// then a barrier and drain_tile.  Three instantiations per file format, chosen by the weights on the host, so that an absent
// source has no load in the code at all:
//   kDen   the groups are load_group's over the denoised run (16 bytes of the source cut at its 16-byte boundaries);
//   kOrig  the same over the original run, which starts at the tile's first frame at or after orig_zeros; the frames in front
//          of it are w_orig * +0.0f, written by a loop of their own (consecutive lanes consecutive frames of one channel);
//   kBoth  the groups are cut on the DENOISED run's 16-byte boundaries.  The two runs do not share an alignment (in the harness
//          they are 482 = 2 mod 4 samples apart, so at most one of them is on a 16-byte boundary), so the original's four
//          samples of a whole group are taken with the widest loads their address allows: one 16-byte load at 0 modulo 16, two
//          8-byte loads at 8 modulo 16, four 4-byte loads otherwise -- never a 16-byte load at an address that is not a multiple
//          of 16.  The address steps by 16 bytes from group to group, so the choice is the same for every whole group of a
//          channel: no divergence inside a wavefront but where two channels meet.  A group that holds a leading zero, and the
//          run's first and last group, go element by element.  No sample outside either run is read.
// LDS cost: the stores of kDen and kBoth are kernels_egress.hip's for f32 lanes, address for address (a lane's four samples
// C B bytes apart, neighbouring lanes 4 C B): its bank arithmetic holds as it stands (mono f32: 4-way on 64 ds_write_b32 per
// tile, about 1000 LDS cycles against some 4800 for the 48 KB of HBM traffic of a two-source tile).  kOrig's zero loop is the one
// new pattern: neighbouring lanes C B bytes apart, one store each; mono f32 and stereo PCM16 4 bytes = 1 bank, conflict-free;
// mono PCM16 two lanes a dword, 2-way; at most orig_zeros frames of a sink, 482 in the harness.  No scratch; no atomic
// read-modify-write and nothing that orders threads (load_b32 / load_b64 below are plain loads the compiler may not fuse).
// The assembly of each kBoth kernel holds two global_load_dwordx4 (the denoised group; the original at 0 modulo 16), two
// global_load_dwordx2 (at 8 modulo 16) and six global_load_dword (four at 4 and 12 modulo 16, two of the element path).
#include <hip/hip_runtime.h>

#include "egress_device.h"
#include "egress_mix.h"
#include "kernels.h"

namespace {

constexpr int kThreads = kStageThreads;
enum Mode { kDen = 0, kOrig = 1, kBoth = 2 };

// One 4-byte / 8-byte load that stays one: written as `*p`, four neighbouring 4-byte loads are fused by the compiler's load
// vectoriser into ONE 16-byte load at an address that is only 4-byte aligned (the target reports such a load as legal), and
// the branches of load_four then fold into that single load.  A relaxed load at single-thread scope is an ordinary
// global_load_dword / global_load_dwordx2 -- no cache-control bits, no ordering, nothing another thread could observe -- that
// the compiler may not fuse with its neighbours.  (`make resource-usage` cannot show this: the widths are read off the assembly.)
__device__ inline uint32_t load_b32(const float* p) { return __hip_atomic_load(reinterpret_cast<const uint32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SINGLETHREAD); }
__device__ inline uint64_t load_b64(const float* p) { return __hip_atomic_load(reinterpret_cast<const uint64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SINGLETHREAD); }

// four consecutive samples at p with the widest loads p's alignment allows (p is 4-byte aligned): one 16-byte load at 0 modulo
// 16, two 8-byte loads at 8, four 4-byte loads at 4 and 12
__device__ inline void load_four(const float* __restrict__ p, float (&x)[4])
{
    const uint32_t low = (uint32_t)(uintptr_t)p & 15;
    if (low == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        x[0] = __uint_as_float(v.x); x[1] = __uint_as_float(v.y); x[2] = __uint_as_float(v.z); x[3] = __uint_as_float(v.w);
    } else if (low == 8) {
        const uint64_t v = load_b64(p), w = load_b64(p + 2);
        x[0] = __uint_as_float((uint32_t)v); x[1] = __uint_as_float((uint32_t)(v >> 32));
        x[2] = __uint_as_float((uint32_t)w); x[3] = __uint_as_float((uint32_t)(w >> 32));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = __uint_as_float(load_b32(p + k));
    }
}

template <typename F, int M>
__device__ inline void mix_tile(const EgressMixArgs& a, uint8_t* lds)
{
    constexpr int G = 4; // f32 samples in 16 source bytes
    constexpr int B = Sink<F>::kBytes;
    const uint32_t u = blockIdx.x;
    const uint32_t ji = find_job(a.unit_prefix, a.n_jobs, u);
    const EgressMixJob j = a.jobs[ji];
    const uint32_t r = u - a.unit_prefix[ji];
    const int t = threadIdx.x;
    const int C = (int)j.n_channels;
    const uint64_t f0 = (uint64_t)r * j.tile_frames;
    const int nfr = (int)min((uint64_t)j.tile_frames, j.n_frames - f0);
    uint8_t* dst = a.out + j.dst_off + f0 * (uint64_t)(C * B);
    const int shift = (int)((uintptr_t)dst & 15);
    // a frame is C * B bytes, so every sample of the tile has frame 0's alignment
    const bool aligned = B == 3 ? false : (shift % B) == 0;
    const float wo = a.w_orig, wd = a.w_den;
    // the tile's frames [0, zt) have no original sample; frame zt + e is element e of the original run po[0, nfr - zt)
    const int zt = M == kDen ? 0 : j.orig_zeros > f0 ? (int)min(j.orig_zeros - f0, (uint64_t)nfr) : 0;
    const float* po = nullptr;
    const float* pd = nullptr;
    if constexpr (M != kDen) po = a.orig + j.orig_off + (zt < nfr ? f0 + (uint64_t)zt - j.orig_zeros : 0); // (f0 + zt >= orig_zeros there; an empty run is not read)
    if constexpr (M != kOrig) pd = a.den + j.den_off + f0;
    const int ng = (nfr + 2 * G - 2) / G; // groups a run of at most nfr can touch, whatever its alignment
    if constexpr (M == kOrig) {
        const uint32_t zero = Quant<F>::run(__fmul_rn(wo, 0.0f));
        for (int i = t; i < C * zt; i += kThreads) {
            const int c = i / zt, f = i - c * zt;
            Sink<F>::store(lds + shift + c * B, f * C * B, aligned, zero);
        }
    }
    for (int i = t; i < C * ng; i += kThreads) {
        const int c = i / ng, g = i - c * ng;
        uint8_t* at = lds + shift + c * B;
        if constexpr (M == kDen) {
            load_group(reinterpret_cast<const uint32_t*>(pd + (uint64_t)c * a.den_stride), nfr, g,
                       [&](int f, uint32_t s) { Sink<F>::store(at, f * C * B, aligned, Quant<F>::run(__fmul_rn(wd, __uint_as_float(s)))); });
        } else if constexpr (M == kOrig) {
            if (zt < nfr)
                load_group(reinterpret_cast<const uint32_t*>(po + (uint64_t)c * a.orig_stride), nfr - zt, g,
                           [&](int e, uint32_t s) { Sink<F>::store(at, (zt + e) * C * B, aligned, Quant<F>::run(__fmul_rn(wo, __uint_as_float(s)))); });
        } else {
            const float* d = pd + (uint64_t)c * a.den_stride;
            const float* o = po + (uint64_t)c * a.orig_stride;
            auto put = [&](int f, float x, float y) {
                Sink<F>::store(at, f * C * B, aligned, Quant<F>::run(__fadd_rn(__fmul_rn(wo, x), __fmul_rn(wd, y))));
            };
            const int mis = (int)(((uintptr_t)d & 15) / sizeof(float));
            const int lo = g * G - mis, hi = lo + G;
            if (lo >= zt && hi <= nfr) { // (zt >= 0) a whole group of both runs: original elements [lo - zt, hi - zt) of nfr - zt
                const uint4 yv = *reinterpret_cast<const uint4*>(d + lo); // 16-byte aligned: the group is cut there
                float x[4];
                load_four(o + (lo - zt), x);
                put(lo, x[0], __uint_as_float(yv.x));
                put(lo + 1, x[1], __uint_as_float(yv.y));
                put(lo + 2, x[2], __uint_as_float(yv.z));
                put(lo + 3, x[3], __uint_as_float(yv.w));
            } else {
                for (int f = max(lo, 0); f < min(hi, nfr); ++f) put(f, f >= zt ? o[f - zt] : 0.0f, d[f]);
            }
        }
    }
    __syncthreads();
    drain_tile(dst, nfr * C * B, shift, lds);
}

} // namespace

template <typename F, int M>
__global__ __launch_bounds__(kThreads) void egress_mix_kernel(EgressMixArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kIngestTileBytes + 16];
    mix_tile<F, M>(a, lds);
}

namespace {

template <int M>
int launch(const EgressMixArgs& a, hipStream_t stream)
{
    const dim3 grid(a.n_units), block(kThreads);
    return launch_file_format(a.file_format, [&](auto f) { hipLaunchKernelGGL((egress_mix_kernel<decltype(f), M>), grid, block, 0, stream, a); });
}

} // namespace

int fvad_launch_egress_mix(const EgressMixArgs& a, hipStream_t stream)
{
    if (a.w_orig == 0.0f && a.w_den == 0.0f) return (int)hipErrorInvalidValue; // (refused by the check)
    if (a.w_orig == 0.0f) return launch<kDen>(a, stream);
    if (a.w_den == 0.0f) return launch<kOrig>(a, stream);
    return launch<kBoth>(a, stream);
}
