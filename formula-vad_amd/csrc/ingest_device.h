// ingest_device.h -- device helpers shared by the ingest kernels (kernels_ingest.hip, kernels_ingest_resample.hip): the search of
// a prefix table, the samples of the three source formats read from staged LDS bytes, and the 16-byte destination groups.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// the job whose units [prefix[j], prefix[j + 1]) hold unit u (prefix[0] = 0, prefix[n] > u; every job has at least one unit)
__device__ inline uint32_t find_job(const uint32_t* __restrict__ prefix, uint32_t n, uint32_t u)
{
    uint32_t lo = 0, hi = n; // invariant: prefix[lo] <= u < prefix[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (prefix[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

struct Pcm24 {}; // 3 bytes, little-endian, two's complement

// Source<S>: bytes per sample and the sample at LDS byte b as its integer image (aligned: b is a multiple of the sample's size)
template <typename S> struct Source;
template <> struct Source<int16_t> {
    static constexpr int kBytes = 2;
    __device__ static int32_t load(const uint8_t* lds, int b, bool aligned)
    {
        if (aligned) return *reinterpret_cast<const int16_t*>(lds + b);
        return (int16_t)(uint16_t)(lds[b] | (lds[b + 1] << 8));
    }
};
template <> struct Source<Pcm24> {
    static constexpr int kBytes = 3;
    __device__ static int32_t load(const uint8_t* lds, int b, bool)
    {
        const uint32_t u = (uint32_t)lds[b] | ((uint32_t)lds[b + 1] << 8) | ((uint32_t)lds[b + 2] << 16);
        return (int32_t)(u << 8) >> 8; // sign-extended
    }
};
template <> struct Source<float> {
    static constexpr int kBytes = 4;
    __device__ static int32_t load(const uint8_t* lds, int b, bool aligned)
    {
        if (aligned) return (int32_t)*reinterpret_cast<const uint32_t*>(lds + b);
        return (int32_t)((uint32_t)lds[b] | ((uint32_t)lds[b + 1] << 8) | ((uint32_t)lds[b + 2] << 16) | ((uint32_t)lds[b + 3] << 24));
    }
};

// Group g of the run p[0, n): the elements of the g-th 16 destination bytes counted from the 16-byte boundary at or below p.
// A group wholly inside the run is one 16-byte store, the others (the run's first and last) element stores; a group past the
// run stores nothing.  sample(i) gives element i of the run.
template <typename E, typename F>
__device__ inline void store_group(E* p, int n, int g, F sample)
{
    constexpr int G = 16 / (int)sizeof(E);
    const int a = (int)(((uintptr_t)p & 15) / sizeof(E));
    const int lo = g * G - a, hi = lo + G;
    if (lo >= 0 && hi <= n) {
        alignas(16) E v[G];
#pragma unroll
        for (int i = 0; i < G; ++i) v[i] = sample(lo + i);
        *reinterpret_cast<uint4*>(p + lo) = *reinterpret_cast<const uint4*>(v);
    } else {
        for (int i = max(lo, 0); i < min(hi, n); ++i) p[i] = sample(i);
    }
}
