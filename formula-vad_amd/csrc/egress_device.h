// egress_device.h -- device helpers of the egress kernels (kernels_egress.hip, kernels_egress_resample.hip,
// kernels_egress_mix.hip), the mirror of ingest_device.h and stage_tile.h: the 16-byte source groups of a lane run, an f32 value
// as a file format's sample, the file formats' samples written into staged LDS bytes, a tile of
// bytes with an arbitrary destination drained from LDS, and the launch of a file format's instantiation.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/fvad.h"
#include "ingest_device.h" // find_job, Pcm24
#include "stage_tile.h"    // kStageThreads

// Group g of the run p[0, n): the elements of the g-th 16 source bytes counted from the 16-byte boundary at or below p.  A
// group wholly inside the run is one 16-byte load, the others (the run's first and last) element loads; a group past the run
// loads nothing: no element outside the run is read.  put(i, v) takes element i of the run.
template <typename E, typename F>
__device__ inline void load_group(const E* __restrict__ p, int n, int g, F put)
{
    constexpr int G = 16 / (int)sizeof(E);
    const int a = (int)(((uintptr_t)p & 15) / sizeof(E));
    const int lo = g * G - a, hi = lo + G;
    if (lo >= 0 && hi <= n) {
        alignas(16) E v[G];
        *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(p + lo);
#pragma unroll
        for (int i = 0; i < G; ++i) put(lo + i, v[i]);
    } else {
        for (int i = max(lo, 0); i < min(hi, n); ++i) put(i, p[i]);
    }
}

// Quant<F>: an f32 value as the file sample's integer image.  f32: its bits (NaN payloads and -0 survive); PCM16:
// rint(fminf(fmaxf(y * 32768, -32768), 32767)), Convert<int16_t, float> of clip_device.h; PCM24 the same with 8388608 and 8388607,
// its low three bytes written.  (y * scale quiets a signalling NaN, fmaxf then gives the lower bound.)
template <typename F> struct Quant;
template <> struct Quant<float> { __device__ static uint32_t run(float y) { return __float_as_uint(y); } };
template <> struct Quant<int16_t> {
    __device__ static uint32_t run(float y) { return (uint32_t)(int32_t)__builtin_rintf(fminf(fmaxf(y * 32768.0f, -32768.0f), 32767.0f)); }
};
template <> struct Quant<Pcm24> {
    __device__ static uint32_t run(float y) { return (uint32_t)(int32_t)__builtin_rintf(fminf(fmaxf(y * 8388608.0f, -8388608.0f), 8388607.0f)); }
};

// Sink<F>: bytes per sample of the file format and the sample's integer image stored at LDS byte b, little-endian (aligned: b is
// a multiple of the sample's size)
template <typename F> struct Sink;
template <> struct Sink<int16_t> {
    static constexpr int kBytes = 2;
    __device__ static void store(uint8_t* lds, int b, bool aligned, uint32_t s)
    {
        if (aligned) { *reinterpret_cast<uint16_t*>(lds + b) = (uint16_t)s; return; }
        lds[b] = (uint8_t)s;
        lds[b + 1] = (uint8_t)(s >> 8);
    }
};
template <> struct Sink<Pcm24> {
    static constexpr int kBytes = 3;
    __device__ static void store(uint8_t* lds, int b, bool, uint32_t s)
    {
        lds[b] = (uint8_t)s;
        lds[b + 1] = (uint8_t)(s >> 8);
        lds[b + 2] = (uint8_t)(s >> 16);
    }
};
template <> struct Sink<float> {
    static constexpr int kBytes = 4;
    __device__ static void store(uint8_t* lds, int b, bool aligned, uint32_t s)
    {
        if (aligned) { *reinterpret_cast<uint32_t*>(lds + b) = s; return; }
        lds[b] = (uint8_t)s;
        lds[b + 1] = (uint8_t)(s >> 8);
        lds[b + 2] = (uint8_t)(s >> 16);
        lds[b + 3] = (uint8_t)(s >> 24);
    }
};

// stage_tile's inverse: the n (1 .. the tile) bytes lds[shift ..), shift = dst's offset within 16 bytes, to dst.  The 16-byte
// aligned body strictly inside [dst, dst + n) is written with 16-byte stores, the bytes in front of and behind it one by one:
// no byte outside the run is written.  The caller's barrier stands between the LDS writes and this.
__device__ inline void drain_tile(uint8_t* __restrict__ dst, int n, int shift, const uint8_t* lds)
{
    const int t = threadIdx.x;
    const int head = min(n, (16 - shift) % 16);
    const int nvec = (n - head) / 16;
    uint4* dv = reinterpret_cast<uint4*>(dst + head);
    const uint4* lv = reinterpret_cast<const uint4*>(lds + shift + head); // shift + head is 0 or 16 whenever nvec > 0
    for (int v = t; v < nvec; v += kStageThreads) dv[v] = lv[v];
    const int tail0 = head + nvec * 16;
    if (t < head) dst[t] = lds[shift + t];
    if (t < n - tail0) dst[tail0 + t] = lds[shift + tail0 + t];
}

// The instantiation of a file format: launch(F{}) queues the kernel whose file sample type is F; the result is the launch's
// hipError_t as int.
template <typename L>
inline int launch_file_format(int file_format, L launch)
{
    if (file_format == FVAD_INGEST_F32) launch(float{});
    else if (file_format == FVAD_INGEST_PCM16) launch(int16_t{});
    else if (file_format == FVAD_INGEST_PCM24) launch(Pcm24{});
    else return (int)hipErrorInvalidValue; // (the callers refuse the formats before they get here)
    return (int)hipGetLastError();
}
