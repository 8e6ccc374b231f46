// kernels_eval.hip -- the Evaluator statistics of every (stream, config) machine of a VAD batch on the GPU, next to the segments
// the machine kernel (kernels_vad.hip) left in device memory: one lane per machine, machine = stream * n_configs + config, so a
// wavefront holds configs of one stream (the machine kernel's default lane mapping) and its reads of that stream's labels are
// shared.  The walk is eval_walk.h's, the one the host scorer runs (host_eval.cpp): the same f32 operations in the same order,
// each segment converted as fvad_segment_to_sec does ((float)u64 / (float)sample_rate, correctly rounded on both sides).
// Not a hot path next to the machines: the simple form, binary searches per segment and per label.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eval_walk.h"
#include "kernels.h"

__global__ __launch_bounds__(64) void vad_score_kernel(VadScoreArgs a)
{
    const long m = (long)blockIdx.x * 64 + threadIdx.x;
    if (m >= a.n_machines) return;
    const long s = m / a.n_configs;
    const int c = (int)(m - s * a.n_configs);
    const uint32_t n = a.seg_count[m] < a.seg_cap ? a.seg_count[m] : a.seg_cap;
    const fvad_speech_segment* seg = a.segs + m * (long)a.seg_cap;
    const float sr = a.sample_rate_f;
    auto vad = [&](uint32_t i) {
        fvad_segment_sec r;
        r.from_sec = (float)seg[i].sample_from / sr;
        r.to_sec = (float)seg[i].sample_to / sr;
        return r;
    };
    const unsigned long long r0 = a.ref_off[s], r1 = a.ref_off[s + 1];
    a.out[m] = fvad_eval::score_walk(vad, n, a.refs + r0, a.ref_pmax + r0, (uint32_t)(r1 - r0), a.stat_cfgs[c]);
}

int fvad_launch_vad_score(const VadScoreArgs& a, hipStream_t stream)
{
    if (a.n_machines <= 0) return (int)hipSuccess;
    const dim3 grid((unsigned)((a.n_machines + 63) / 64));
    hipLaunchKernelGGL(vad_score_kernel, grid, dim3(64), 0, stream, a);
    return (int)hipGetLastError();
}
