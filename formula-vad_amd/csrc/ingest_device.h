// ingest_device.h -- device helpers shared by the ingest kernels (kernels_ingest.hip, kernels_ingest_resample.hip): the search of
// a prefix table, the samples of the three source formats read from staged LDS bytes, and the 16-byte destination groups; then
// what a workgroup of either kernel begins with -- its unit, the fill tile -- and the source formats' samples as f32.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"    // kIngestFillTile
#include "stage_tile.h" // kStageThreads

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

// The unit of workgroup u: the job whose units hold it (find_job), returned as a copy, and *r, its number within the job --
// data tile r for r < n_data_tiles, else a fill tile (kernels.h).  (The job is read before the prefix entry: both scalar loads
// are then in flight together.)
template <typename Job>
__device__ inline Job find_unit(const Job* __restrict__ jobs, const uint32_t* __restrict__ prefix, uint32_t n_jobs, uint32_t u, uint32_t* r)
{
    const uint32_t ji = find_job(prefix, n_jobs, u);
    const Job j = jobs[ji];
    *r = u - prefix[ji];
    return j;
}

// Fill tile q (= r - n_data_tiles) of a job: kIngestFillTile zeros, or what is left of fill_len, of ONE lane behind the `count`
// samples the job writes there, as store_group runs of E.  lanes: the job's sample 0 of channel 0.
template <typename E>
__device__ inline void fill_tile(E* lanes, uint64_t lane_stride, uint64_t count, uint64_t fill_len, uint32_t n_fill_tiles, uint32_t q)
{
    constexpr int G = 16 / (int)sizeof(E);
    const uint32_t ch = q / n_fill_tiles, k = q % n_fill_tiles;
    const uint64_t e0 = (uint64_t)k * kIngestFillTile;
    const int n = (int)min((uint64_t)kIngestFillTile, fill_len - e0);
    E* p = lanes + (uint64_t)ch * lane_stride + count + e0;
    const int ng = (n + 2 * G - 2) / G; // groups a run of n can touch, whatever its alignment
    for (int g = threadIdx.x; g < ng; g += kStageThreads) store_group(p, n, g, [](int) { return (E)0; });
}

// decode_f32<S>: a source sample's integer image (Source<S>::load) as the f32 the lanes hold: PCM16 s / 32768, PCM24
// s / 8388608 (both exact), f32 its bits
template <typename S> __device__ inline float decode_f32(int32_t s);
template <> __device__ inline float decode_f32<int16_t>(int32_t s) { return (float)s * (1.0f / 32768.0f); }
template <> __device__ inline float decode_f32<Pcm24>(int32_t s) { return (float)s * (1.0f / 8388608.0f); }
template <> __device__ inline float decode_f32<float>(int32_t s) { return __int_as_float(s); }
