// vad_machine.h -- one step of a VAD machine (VADMachine.zig:138-239) once its rolling averages have been pushed: the decision
// with the lazily exact long-term average (host_vad.cpp explains the bound), the four-state machine, trackSpeechStats, the
// closing of a segment and the margin audit.  Shared by the host machine (host_vad.cpp, plain C++) and the sweep kernel
// (kernels_vad.hip): the same operations in the same order on both sides, so both give the same bits (the library is built with
// -ffp-contract=off; f32 division and u64 -> f32 conversion are correctly rounded on both sides).  The rings, the exact
// long-term chain and the segment storage are each side's own.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/fvad.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define FVAD_HD __host__ __device__
#else
#define FVAD_HD
#endif

namespace fvad {

constexpr double kU = 1.1102230246251565e-16; // 2^-53

// per config: what a machine derives from its VADMachine.Config (vad_machine_cfg, host_vad.cpp)
struct VadMachineCfg {
    double lt_scalar, st_scalar, cr_scalar; // 1 / ring length (RollingAverage.zig:45-56 once full)
    double lt_q_init;        // fl(initial_long_term_avg * lt_scalar): the term of a slot still holding the initial value
    double initial;          // initial_long_term_avg
    double factor;           // (double)speech_threshold_factor
    double ratio_threshold;  // (double)channel_vol_ratio_threshold
    double gamma;            // n u / (1 - n u), n = long_len
    uint64_t min_open, max_gap, start_buffer, end_buffer; // VADMachine.zig:161,163,312-325 in samples
    float input_len_sec, sample_rate_f, min_vad_duration_sec;
    uint32_t long_len, short_len, ratio_len;
    int32_t has_init;
    uint32_t band;           // band block of the sweep's band sums this config reads (kernels_vad.hip)
};

FVAD_HD inline uint64_t offset_start(const VadMachineCfg& cf, uint64_t vad_from) // VADMachine.zig:312-317
{
    return vad_from - (cf.start_buffer < vad_from ? cf.start_buffer : vad_from);
}

struct VadMachineState {
    enum { CLOSED, OPENING, OPEN, CLOSING };
    int state = CLOSED;
    uint64_t speech_start = 0, speech_end = 0;
    float ratio_sum = 0;
    uint64_t ratio_count = 0;
    float met_cum = 0; // vad_threshold_met_cumulative_sec
    fvad_vad_audit audit = {__builtin_inf(), __builtin_inf(), 0};
    // The long-term average: lt_last is the chain's last value (current only while !lt_stale); between exact evaluations
    // lt_approx is updated push by push, lt_err bounds the rounding of those updates, lt_abs follows sum |q_i| (lt_abs_anchor:
    // its exact value at the last exact evaluation).
    double lt_last = 0;
    bool has_last = false;
    double lt_approx = 0, lt_err = 0, lt_abs = 0, lt_abs_anchor = 0;
    bool lt_stale = false, lt_anchored = false;
    uint32_t lt_updates = 0;
    uint64_t exact_evals = 0, lazy_pushes = 0; // statistics

    // the exact chain over the ring gave acc, with sum |q_i| = abs_sum
    FVAD_HD void anchor(double acc, double abs_sum)
    {
        lt_last = acc;
        has_last = true;
        lt_approx = acc;
        lt_abs = abs_sum;
        lt_abs_anchor = abs_sum;
        lt_anchored = true;
        lt_err = 0.0;
        lt_stale = false;
        lt_updates = 0;
        ++exact_evals;
    }

    // a push on the full ring replaced the term qo with qn; true when the caller is to re-anchor (keeps the bound tight)
    FVAD_HD bool lazy_update(double qn, double qo)
    {
        const double s1 = lt_approx + qn, s2 = s1 - qo;
        lt_err += 2.0 * kU * (fabs(s1) + fabs(s2)); // each rounding <= u |result|; doubled
        lt_abs += fabs(qn) - fabs(qo);
        lt_approx = s2;
        lt_stale = true;
        has_last = true;
        ++lazy_pushes;
        return ++lt_updates >= 4096;
    }

    // `short_term > long_term * factor && ratio > ratio_threshold` (VADMachine.zig:166-171) and the margin audit.  A stale
    // long-term average (only a lazy push, on a full ring, makes it stale) settles it when the interval its bound gives leaves
    // no doubt and the frame cannot lower the audit's minimum margin; otherwise exact() runs the chain (and anchors on it).
    template <class Exact>
    FVAD_HD bool decide(const VadMachineCfg& cf, double st_avg, double cr_avg, Exact&& exact)
    {
        const double f = cf.factor;
        const double thr_r = cf.ratio_threshold;
        if (lt_stale) {
            // lt_abs is itself updated in floating point: widen it by its own drift
            const double abs_now = fabs(lt_abs) * (1.0 + 1e-9) + 8192.0 * 2.0 * kU * (fabs(lt_abs) + lt_abs_anchor);
            const double delta = lt_err + 2.0 * cf.gamma * (abs_now + lt_abs_anchor);
            double t0 = (lt_approx - delta) * f, t1 = (lt_approx + delta) * f;
            if (t0 > t1) { const double t = t0; t0 = t1; t1 = t; }
            const double lo = t0 - fabs(t0) * 4.0 * kU - 1e-300, hi = t1 + fabs(t1) * 4.0 * kU + 1e-300;
            const bool sure_true = st_avg > hi, sure_false = st_avg <= lo;
            bool need_exact = !(sure_true || sure_false);
            if (!need_exact && hi > 0) {
                // smallest relative margin |st - thr| / thr any threshold in [lo, hi] could give
                const double gap = sure_true ? st_avg - hi : lo - st_avg;
                const double m_lb = gap / (sure_true ? hi : (lo < hi ? hi : lo));
                if (!(m_lb * (1.0 - 1e-9) > audit.min_rel_threshold_margin)) need_exact = true;
            }
            if (!need_exact) {
                const double rm = fabs(cr_avg - thr_r);
                if (rm < audit.min_abs_ratio_margin) audit.min_abs_ratio_margin = rm;
                audit.n_frames++;
                return sure_true && cr_avg > thr_r;
            }
            exact();
        }
        double base; // :169  last_avg orelse initial_long_term_avg orelse short_term
        if (has_last) base = lt_last;
        else if (cf.has_init) base = cf.initial;
        else base = st_avg;
        const double threshold = base * f; // :170
        const bool met = st_avg > threshold && cr_avg > thr_r; // :171
        // margin audit: how close was this frame to flipping?
        if (threshold > 0) {
            const double m = fabs(st_avg - threshold) / threshold;
            if (m < audit.min_rel_threshold_margin) audit.min_rel_threshold_margin = m;
        }
        const double rm = fabs(cr_avg - thr_r);
        if (rm < audit.min_abs_ratio_margin) audit.min_abs_ratio_margin = rm;
        audit.n_frames++;
        return met;
    }

    // the state transitions (:189-233) and trackSpeechStats (:241-263) of the frame at sample `index`; a segment that closes
    // (onSpeechEnd, :265-309) goes to sink(const fvad_speech_segment&)
    template <class Sink>
    FVAD_HD fvad_vad_result finish_step(const VadMachineCfg& cf, uint64_t index, bool met, bool has_ratio, float ratio, Sink&& sink)
    {
        fvad_vad_result result = {FVAD_REC_NONE, 0};
        const int from_state = state;
        switch (state) {
        case CLOSED:
            if (met) { state = OPENING; speech_start = index; }
            break;
        case OPENING:
            if (met && index - speech_start >= cf.min_open) { state = OPEN; result = {FVAD_REC_STARTED, offset_start(cf, speech_start)}; }
            else if (!met) state = CLOSED;
            break;
        case OPEN:
            if (!met) { state = CLOSING; speech_end = index; }
            break;
        default: // CLOSING
            if (met) state = OPEN;
            else if (index - speech_end >= cf.max_gap) {
                state = CLOSED;
                const float length_sec = (float)(speech_end - speech_start) / cf.sample_rate_f;
                const float avg_ratio = ratio_sum / (float)ratio_count;
                result = {FVAD_REC_ABORTED, 0};
                if (length_sec >= cf.min_vad_duration_sec) {
                    fvad_speech_segment s;
                    s.sample_from = offset_start(cf, speech_start);
                    s.sample_to = speech_end + cf.end_buffer; // :320-325
                    s.avg_channel_vol_ratio = avg_ratio;
                    s.vad_met_sec = met_cum;
                    sink(s);
                    result = {FVAD_REC_COMPLETED, s.sample_to};
                }
            }
            break;
        }
        const float r = has_ratio ? ratio : 0;
        if (from_state == CLOSED && state == OPENING) {
            ratio_sum = r;
            ratio_count = 1;
            met_cum = cf.input_len_sec;
        } else if (from_state == OPEN) {
            ratio_sum += r;
            ratio_count += 1;
            if (met) met_cum += cf.input_len_sec;
        }
        return result;
    }
};

// A sweep machine between two launches of the kernel's resume form (kernels_vad.hip): the step's state, the cursors of its rings
// (the rings themselves stay in device memory), its segment count and where its current part has got to
struct VadLaneState {
    VadMachineState m;
    double st_pref, cr_pref;
    uint32_t st_w, st_wc, cr_w, cr_wc;
    uint32_t lt_w, lt_wc, lt_filled, lt_steady;
    uint32_t n_segs, seg_base; // segments closed so far; the first of them in the segment buffer
    uint64_t next_frame;       // the next frame the machine runs
};

} // namespace fvad
