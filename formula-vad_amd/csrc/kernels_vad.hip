// kernels_vad.hip -- the VAD state machines of a parameter sweep on the GPU: one lane per (stream, config) machine.
//
// A port of host_vad.cpp's VadMachine::run (VADMachine.zig:138-239) that gives the same bits: f64 rolling averages summed in
// index order (RollingAverage.zig:45-56), the lazily exact long-term average with host_vad.cpp's error bound and its exact
// re-evaluations, the four-state machine, the segment statistics and the margin audit, every operation in the host's order
// (the library is built with -ffp-contract=off: no fused multiply-adds; f32 division and u64 -> f32 conversion are correctly
// rounded on both sides).  What only depends on the stream -- the volume ratio of each frame -- comes from the host.
//
// Storage per machine.  Pushed samples are f32, so every ring holds f32 and the f64 term fl(data[i] * scalar) is recomputed
// inside the chain with the bits the host's cached product has (data[i] = (double)sample there).  The long-term ring also
// needs "slot still holds initial_long_term_avg": slot i holds a pushed value iff i < lt_filled (pushes fill it from slot 0).
// The long-term rings (8437 slots at the defaults) are in global memory, four slots of a machine side by side and those groups
// slot-major over the machines, so that a wavefront's load of four slots is one 1 KB run and the exact chain keeps 64 slots in
// flight; the short-term and channel-ratio rings (9 and 23 at the defaults) are in LDS when
// the workgroup's rings fit, else in global memory (one template, instantiated for either address space: the LDS form must
// not go through flat pointers, whose loads take a global load's latency).
//
// Lane mapping (one wavefront per workgroup, 64 machines): by stream, the lanes of a wavefront are configs of one stream (or of a
// few), so the per-frame ratio load is one address and every lane runs as many frames; by config, they are streams of one config,
// so every lane has the same ring lengths.  The work is latency-bound scalar f64 per lane; a wavefront runs the union of its
// lanes' exact long-term chains.
// Every loop is bounded by the machine's frame count or a ring length; no workgroup waits on another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "kernels.h"

namespace {

constexpr double kU = 1.1102230246251565e-16; // 2^-53, as host_vad.cpp

template <class P> // float* (global) or an LDS float pointer: the address space is known, so LDS slots are ds_read / ds_write
struct Ring { // a rolling average without initial value (RollingAverage.zig:11-56) over f32 slots base[i * stride]
    P base;
    long stride;
    uint32_t len, w, wc;
    double scalar, pref;

    // RollingAverage.push: before the ring is full the chain over the written slots with 1 / written_count; once full
    // host_vad.cpp's prefix form (the chain resumed from the sum below the write index: the same additions in the same order)
    __device__ double push(float x)
    {
        base[(long)w * stride] = x;
        if (wc == len) {
            double acc = (w == 0) ? 0.0 : pref;
            acc += (double)x * scalar;
            const double new_pref = acc;
#pragma unroll 8
            for (uint32_t i = w + 1; i < len; ++i) acc += (double)base[(long)i * stride] * scalar;
            w = (w + 1 == len) ? 0 : w + 1;
            pref = (w == 0) ? 0.0 : new_pref;
            return acc;
        }
        w = (w + 1 == len) ? 0 : w + 1;
        wc += 1;
        const double sc = 1.0 / (double)wc;
        double acc = 0.0;
#pragma unroll 8
        for (uint32_t i = 0; i < wc; ++i) acc += (double)base[(long)i * stride] * sc;
        if (wc == len) pref = 0.0; // steady from here on (the write index is back at 0)
        return acc;
    }
};

template <class P>
struct Machine {
    VadMachineCfg cf; // in registers: read through a pointer, every field would be loaded again after each ring store (may alias)
    // long-term ring and its lazily exact average (host_vad.cpp: long_term_push, long_term_exact, decide).  Slot i of this
    // machine at lt[(i / 4) * lt_stride + i % 4]: four consecutive slots are one 16-byte load of the lane.
    float* lt;
    long lt_stride;
    float lt_next = 0; // slot lt_w, loaded one push ahead (the next lazy push overwrites it and needs its old value at once)
    uint32_t lt_w = 0, lt_wc = 0, lt_filled = 0, lt_updates = 0;
    bool lt_steady = false, lt_has_last = false, lt_stale = false, lt_anchored = false;
    double lt_last = 0, lt_approx = 0, lt_err = 0, lt_abs = 0, lt_abs_anchor = 0;
    uint64_t exact_evals = 0, lazy_pushes = 0;
    Ring<P> st, cr;
    // VADMachine state
    int state = 0; // CLOSED, OPENING, OPEN, CLOSING
    uint64_t speech_start = 0, speech_end = 0;
    float ratio_sum = 0;
    uint64_t ratio_count = 0;
    float met_cum = 0;
    double a_rel = __builtin_inf(), a_abs = __builtin_inf();
    uint64_t a_frames = 0;
    uint32_t n_segs = 0;

    __device__ float& slot(uint32_t i) const { return lt[(long)(i >> 2) * lt_stride + (i & 3)]; }
    __device__ double lt_q(uint32_t i, float x) const { return i < lt_filled ? (double)x * cf.lt_scalar : cf.lt_q_init; }

    // The reference's chain over the whole ring.  The chain's adds depend on each other, its loads do not: blocks of kLtBlock
    // slots are loaded (16 bytes per lane and instruction) one block ahead of the adds, so that 2 kLtBlock slots are in flight
    // (the ring is allocated in whole blocks plus one: the loads past long_len stay inside it, their terms are not added)
    static constexpr int kLtBlock = 64;
    __device__ void load_block(uint32_t i0, float4 (&x)[kLtBlock / 4]) const
    {
#pragma unroll
        for (int g = 0; g < kLtBlock / 4; ++g) x[g] = *reinterpret_cast<const float4*>(lt + (long)((i0 >> 2) + g) * lt_stride);
    }
    __device__ void lt_exact()
    {
        double acc = 0.0, abs_sum = 0.0;
        const uint32_t n = cf.long_len;
        float4 cur[kLtBlock / 4], nxt[kLtBlock / 4];
        load_block(0, cur);
        for (uint32_t i0 = 0; i0 < n; i0 += kLtBlock) {
            load_block(i0 + kLtBlock, nxt); // (unconditional: a branch here would make the adds below wait for these loads too)
#pragma unroll
            for (int j = 0; j < kLtBlock; ++j) {
                const float4 v = cur[j / 4];
                const float x = (j & 3) == 0 ? v.x : (j & 3) == 1 ? v.y : (j & 3) == 2 ? v.z : v.w;
                const uint32_t i = i0 + (uint32_t)j;
                const double q = lt_q(i, x);
                acc = i < n ? acc + q : acc; // (a skipped term: the chain as if it were not there)
                abs_sum = i < n ? abs_sum + fabs(q) : abs_sum;
            }
#pragma unroll
            for (int g = 0; g < kLtBlock / 4; ++g) cur[g] = nxt[g];
        }
        lt_last = acc;
        lt_has_last = true;
        lt_approx = acc;
        lt_abs = abs_sum;
        lt_abs_anchor = abs_sum;
        lt_anchored = true;
        lt_err = 0.0;
        lt_stale = false;
        lt_updates = 0;
        ++exact_evals;
    }

    __device__ void lt_push(float mv)
    {
        const uint32_t len = cf.long_len;
        if (!lt_steady) { // ring not full yet: RollingAverage.push as the reference runs it
            slot(lt_w) = mv;
            lt_w = (lt_w + 1 == len) ? 0 : lt_w + 1;
            lt_wc += 1;
            lt_filled = lt_wc;
            const double sc = 1.0 / (double)lt_wc;
            double acc = 0.0;
#pragma unroll 8
            for (uint32_t i = 0; i < lt_wc; ++i) acc += (double)slot(i) * sc;
            lt_last = acc;
            lt_has_last = true;
            if (lt_wc == len) { lt_steady = true; lt_next = slot(0); lt_exact(); }
            return;
        }
        if (!lt_anchored) lt_exact();
        const uint32_t w = lt_w;
        const double qn = (double)mv * cf.lt_scalar, qo = lt_q(w, lt_next);
        slot(w) = mv;
        if (lt_filled < len) lt_filled += 1; // (only with an initial value: slot w == lt_filled is the one written now)
        lt_w = (w + 1 == len) ? 0 : w + 1;
        lt_next = slot(lt_w); // (w + 1 == len == 1: the slot just written, read back after the store)
        const double s1 = lt_approx + qn, s2 = s1 - qo;
        lt_err += 2.0 * kU * (fabs(s1) + fabs(s2));
        lt_abs += fabs(qn) - fabs(qo);
        lt_approx = s2;
        lt_stale = true;
        lt_has_last = true;
        ++lazy_pushes;
        if (++lt_updates >= 4096) lt_exact();
    }

    __device__ bool decide(double st_avg, double cr_avg)
    {
        const double f = cf.factor;
        const double thr_r = cf.ratio_threshold;
        if (lt_steady && lt_stale) {
            const double gamma = cf.gamma;
            const double abs_now = fabs(lt_abs) * (1.0 + 1e-9) + 8192.0 * 2.0 * kU * (fabs(lt_abs) + lt_abs_anchor);
            const double delta = lt_err + 2.0 * gamma * (abs_now + lt_abs_anchor);
            double t0 = (lt_approx - delta) * f, t1 = (lt_approx + delta) * f;
            if (t0 > t1) { const double t = t0; t0 = t1; t1 = t; }
            const double lo = t0 - fabs(t0) * 4.0 * kU - 1e-300, hi = t1 + fabs(t1) * 4.0 * kU + 1e-300;
            const bool sure_true = st_avg > hi, sure_false = st_avg <= lo;
            bool need_exact = !(sure_true || sure_false);
            if (!need_exact && hi > 0) {
                const double gap = sure_true ? st_avg - hi : lo - st_avg;
                const double m_lb = gap / (sure_true ? hi : (lo < hi ? hi : lo));
                if (!(m_lb * (1.0 - 1e-9) > a_rel)) need_exact = true;
            }
            if (!need_exact) {
                const double rm = fabs(cr_avg - thr_r);
                if (rm < a_abs) a_abs = rm;
                a_frames++;
                return sure_true && cr_avg > thr_r;
            }
            lt_exact();
        }
        double base;
        if (lt_has_last) base = lt_last;
        else if (cf.has_init) base = cf.initial;
        else base = st_avg;
        const double threshold = base * f;
        const bool met = st_avg > threshold && cr_avg > thr_r;
        if (threshold > 0) {
            const double m = fabs(st_avg - threshold) / threshold;
            if (m < a_rel) a_rel = m;
        }
        const double rm = fabs(cr_avg - thr_r);
        if (rm < a_abs) a_abs = rm;
        a_frames++;
        return met;
    }

    __device__ void speech_end_event(VadSegmentDev* seg, uint32_t cap)
    {
        const uint64_t length_samples = speech_end - speech_start;
        const float length_sec = (float)length_samples / cf.sample_rate_f;
        const float avg_ratio = ratio_sum / (float)ratio_count;
        if (length_sec >= cf.min_vad_duration_sec) {
            if (n_segs < cap) {
                VadSegmentDev s;
                s.sample_from = speech_start - (cf.start_buffer < speech_start ? cf.start_buffer : speech_start);
                s.sample_to = speech_end + cf.end_buffer;
                s.avg_channel_vol_ratio = avg_ratio;
                s.vad_met_sec = met_cum;
                seg[n_segs] = s;
            }
            ++n_segs; // counted past the capacity: the caller sees the overflow and runs again with room for all
        }
    }

    __device__ void finish_step(uint64_t index, bool met, bool has_ratio, float ratio, VadSegmentDev* seg, uint32_t cap)
    {
        const int from_state = state;
        switch (state) {
        case 0:
            if (met) { state = 1; speech_start = index; }
            break;
        case 1:
            if (met && index - speech_start >= cf.min_open) state = 2;
            else if (!met) state = 0;
            break;
        case 2:
            if (!met) { state = 3; speech_end = index; }
            break;
        default:
            if (met) state = 2;
            else if (index - speech_end >= cf.max_gap) { state = 0; speech_end_event(seg, cap); }
            break;
        }
        const float r = has_ratio ? ratio : 0;
        if (from_state == 0 && state == 1) {
            ratio_sum = r;
            ratio_count = 1;
            met_cum = cf.input_len_sec;
        } else if (from_state == 2) {
            ratio_sum += r;
            ratio_count += 1;
            if (met) met_cum += cf.input_len_sec;
        }
    }
};

} // namespace

typedef __attribute__((address_space(3))) float lds_float;

// RINGS_LDS: the short-term and channel-ratio rings in LDS ([st_max + cr_max][64]), else in global memory
template <bool RINGS_LDS>
__global__ __launch_bounds__(64) void vad_machines_kernel(VadMachinesArgs a)
{
    extern __shared__ float vad_rings[];
    using P = typename std::conditional<RINGS_LDS, lds_float*, float*>::type;
    const int lane = threadIdx.x;
    const long m = (long)blockIdx.x * 64 + lane; // this lane's place: its rings
    if (m >= a.n_machines) return;
    // which machine the lane runs: by stream, lane m is machine m (the configs of a stream side by side); by config, the streams of
    // a config side by side (every lane of a wavefront has that config's ring lengths)
    long s;
    int c;
    if (a.by_config) { c = (int)(m / a.n_streams); s = m - (long)c * a.n_streams; }
    else { s = m / a.n_configs; c = (int)(m - s * a.n_configs); }
    const long id = s * a.n_configs + c; // machine index of the outputs
    const VadMachineCfg* cfg = a.cfgs + c;

    Machine<P> mc;
    mc.cf = *cfg;
    mc.lt = a.lt_rings + 4 * m;
    mc.lt_stride = 4 * a.n_machines;
    P rb;
    long rs;
    if constexpr (RINGS_LDS) { rb = (lds_float*)vad_rings + lane; rs = 64; }
    else { rb = a.rings + m; rs = a.n_machines; }
    mc.st = Ring<P>{rb, rs, cfg->short_len, 0, 0, cfg->st_scalar, 0.0};
    mc.cr = Ring<P>{rb + (long)a.st_max * rs, rs, cfg->ratio_len, 0, 0, cfg->cr_scalar, 0.0};
    if (cfg->has_init) { // RollingAverage.init with an initial value (RollingAverage.zig:20-26): full, steady, its average evaluated
        double acc = 0.0;
        for (uint32_t i = 0; i < cfg->long_len; ++i) acc += cfg->lt_q_init;
        mc.lt_last = acc;
        mc.lt_has_last = true;
        mc.lt_steady = true;
        mc.lt_wc = cfg->long_len;
        mc.lt_next = mc.slot(0);
    }

    const long nf = a.n_frames[s];
    const int C = a.n_channels;
    const float* band = a.band + ((long)cfg->band * a.n_lanes + s * C) * a.band_stride;
    const float* ratio = a.ratio + s * a.ratio_stride;
    VadSegmentDev* seg = a.segs + id * (long)a.seg_cap;
    // the next frame's band values (up to kPre channels) and ratio are loaded while this frame runs; the minimum is taken when the
    // frame is run, so that the loads are waited for a frame later (more channels: loaded and reduced at once)
    constexpr int kPre = 4;
    float nv[kPre], nr = 0.0f;
    auto fetch = [&](long k) {
#pragma unroll
        for (int ch = 0; ch < kPre; ++ch) nv[ch] = ch < C ? band[(long)ch * a.band_stride + k] : 999.0f;
        nr = ratio[k];
    };
    auto min_vol = [&](long k) { // VADMachine.zig:153-158, channels in order
        float mn = 999;
#pragma unroll
        for (int ch = 0; ch < kPre; ++ch) if (ch < C && nv[ch] < mn) mn = nv[ch];
        for (int ch = kPre; ch < C; ++ch) {
            const float v = band[(long)ch * a.band_stride + k];
            if (v < mn) mn = v;
        }
        return mn;
    };
    if (nf > 0) fetch(0);
    for (long k = 0; k < nf; ++k) {
        const float mv = min_vol(k), rt = nr;
        if (k + 1 < nf) fetch(k + 1);
        // every frame overlaps a chunk, so its metadata always has a ratio (BufferedFFT.zig:137-140): has_ratio is true, and a
        // NaN ratio (from NaN audio) goes into the ring as it is, as on the host
        const double st = mc.st.push(mv);
        const double cr = mc.cr.push(rt);
        const bool met = mc.decide(st, cr);
        if (!met) mc.lt_push(mv);
        mc.finish_step((uint64_t)k * a.fft_size, met, true, rt, seg, a.seg_cap);
    }
    a.seg_count[id] = mc.n_segs;
    VadAuditDev au;
    au.min_rel_threshold_margin = mc.a_rel;
    au.min_abs_ratio_margin = mc.a_abs;
    au.n_frames = mc.a_frames;
    a.audits[id] = au;
    a.stats[2 * id] = mc.exact_evals;
    a.stats[2 * id + 1] = mc.lazy_pushes;
}

int fvad_launch_vad_machines(const VadMachinesArgs& a, hipStream_t stream)
{
    if (a.n_machines <= 0) return (int)hipSuccess;
    const size_t lds = a.rings_in_lds ? (size_t)(a.st_max + a.cr_max) * 64 * sizeof(float) : 0;
    const dim3 grid((unsigned)((a.n_machines + 63) / 64));
    if (a.rings_in_lds) hipLaunchKernelGGL(vad_machines_kernel<true>, grid, dim3(64), lds, stream, a);
    else hipLaunchKernelGGL(vad_machines_kernel<false>, grid, dim3(64), 0, stream, a);
    return (int)hipGetLastError();
}
