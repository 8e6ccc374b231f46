// clip_device.h -- device helpers shared by the batch Recorder's kernels (kernels_clips*.hip): the search of a prefix
// table and the sample conversions.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// the clip whose units [prefix[c], prefix[c + 1]) hold unit u (prefix[0] = 0, prefix[n] > u; every clip has at least one unit)
__device__ inline uint32_t find_clip(const uint32_t* __restrict__ prefix, uint32_t n, uint32_t u)
{
    uint32_t lo = 0, hi = n; // invariant: prefix[lo] <= u < prefix[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (prefix[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ inline float to_f32(float x) { return x; }
__device__ inline float to_f32(int16_t s) { return (float)s * (1.0f / 32768.0f); } // s / 32768, exact

template <typename D, typename S> struct Convert;
template <typename T> struct Convert<T, T> { __device__ static T run(T x) { return x; } }; // equal formats: the bits
template <> struct Convert<float, int16_t> { __device__ static float run(int16_t s) { return to_f32(s); } };
template <> struct Convert<int16_t, float> { // fvad_lane.denoised_i16's rule (k3_istft_ola_kernel)
    __device__ static int16_t run(float y) { return (int16_t)__builtin_rintf(fminf(fmaxf(y * 32768.0f, -32768.0f), 32767.0f)); }
};
