// kernels_vadfinish.hip -- the second stage of a shared-trigger sweep (context option vad_trigger "shared"): one lane per
// (stream, config) walks the bits its trigger machine emitted for the part (kernels_vad.hip's EMIT form) through the state
// machine, trackSpeechStats and onSpeechEnd.  The walk is vad_finish.h's, the step vad_machine.h's finish_step: the code the host
// runs (fvad_vad_finish_bits), so both give the same bits.
//
// Lanes: a wavefront holds configs of one stream, configs of one trigger machine side by side (VadMachinesArgs.lane_config), so
// the load of a word is one address for all lanes of a key and a few lines for the wavefront, and the ratio row is one row.
// Segments go to the machine's room by the resume form's protocol: a lane whose room is full stops before its next frame and
// sets *paused; the host grows the room and launches this kernel alone again, over the same bits.
// Every loop is bounded by the part's word and frame counts; no LDS, no waiting between lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "vad_finish.h"

__global__ __launch_bounds__(64) void vad_finish_kernel(VadMachinesArgs a)
{
    const long m = (long)blockIdx.x * 64 + threadIdx.x;
    if (m >= a.n_machines) return;
    const long s = m / a.n_configs;
    int c = (int)(m - s * a.n_configs);
    if (a.lane_config) c = a.lane_config[c];
    const long id = s * a.n_configs + c;
    const fvad::VadMachineCfg cf = a.cfgs[c];
    uint64_t F = a.fft_size, first_frame = a.first_frame, first_sample = a.first_frame * a.fft_size;
    long row = s;
    if (a.sized) {
        const uint32_t g = a.size_of[c];
        F = a.sizes[g];
        first_sample = a.first_sample;
        first_frame = first_sample / F;
        row = (long)g * a.n_streams + s;
    }
    fvad::VadMachineState st;
    uint32_t n_segs = 0, seg_base = 0;
    uint64_t k0 = 0;
    fvad::VadLaneState& ls = a.state[id];
    if (!a.fresh) {
        st.state = ls.m.state;
        st.speech_start = ls.m.speech_start;
        st.speech_end = ls.m.speech_end;
        st.ratio_sum = ls.m.ratio_sum;
        st.ratio_count = ls.m.ratio_count;
        st.met_cum = ls.m.met_cum;
        n_segs = ls.n_segs;
        seg_base = a.rebase ? n_segs : ls.seg_base;
        k0 = ls.next_frame > first_frame ? ls.next_frame - first_frame : 0;
    }
    const uint64_t nf = (uint64_t)a.n_frames[row];
    const VadTrigKey tk = a.trig_keys[a.trig_of[c]];
    const unsigned long long* words = a.bits + tk.base + s * (long)tk.words * (long)tk.nk;
    const float* ratio = a.ratio + row * a.ratio_stride;
    fvad_speech_segment* seg = a.segs + id * (long)a.seg_cap;
    const uint32_t cap = a.seg_cap;
    uint64_t k_end = nf;
    if (k0 < nf) {
        k_end = fvad::finish_walk(
            st, cf, k0, nf, first_sample, F, [&](uint64_t w) { return (uint64_t)words[(long)w * (long)tk.nk]; },
            [&](uint64_t k) { return ratio[k]; }, [&] { return n_segs - seg_base < cap; },
            [&](const fvad_speech_segment& sg) {
                if (n_segs - seg_base < cap) seg[n_segs - seg_base] = sg;
                ++n_segs;
            });
        if (k_end < nf) *a.paused = 1;
    }
    ls.m.state = st.state;
    ls.m.speech_start = st.speech_start;
    ls.m.speech_end = st.speech_end;
    ls.m.ratio_sum = st.ratio_sum;
    ls.m.ratio_count = st.ratio_count;
    ls.m.met_cum = st.met_cum;
    ls.n_segs = n_segs;
    ls.seg_base = seg_base;
    ls.next_frame = first_frame + k_end;
    a.seg_count[id] = n_segs;
}

int fvad_launch_vad_finish(const VadMachinesArgs& a, hipStream_t stream)
{
    if (a.n_machines <= 0) return (int)hipSuccess;
    hipLaunchKernelGGL(vad_finish_kernel, dim3((unsigned)((a.n_machines + 63) / 64)), dim3(64), 0, stream, a);
    return (int)hipGetLastError();
}
