// eval_walk.h -- the Evaluator statistics of one VAD machine against its stream's labels, as a walk over sorted lists.
// Shared by the host scorer (host_eval.cpp, plain C++) and the scoring kernel (kernels_eval.hip): the same operations in the
// same order on both sides, and the same bits as host_stats.cpp's fvad_stats_from_segments (Evaluator.zig:90-156,
// statistics.zig:88-114,175-256) -- all f32, the library built with -ffp-contract=off, f32 division and sqrt correctly rounded,
// subnormals kept.
//
// What the walk relies on instead of fvad_stats_from_segments' scan of every pair:
//   * the machine's segments in the order the machine closes them, which is the stable sort by start of fvad_stats_from_segments:
//     sample_from = max(speech_start - start_buffer, 0) and sample_to = speech_end + end_buffer grow with every segment (speech
//     start and end grow), so after the monotone u64 -> f32 conversion both ends are non-decreasing;
//   * the labels stably sorted by start (fvad_vad_batch_set_references), with pmax[j] = the largest end of labels 0..j.
// Overlap is strictly positive (SpeechSegment.findOverlapping), min(ends) - max(starts) > 0, so with subnormals kept it needs
// a.end > b.start and b.end > a.start: the labels that can overlap a segment are those from the first with pmax > segment start
// up to the last with start < segment end (binary searches), and likewise the segments that can overlap a label.  Inside those
// ranges every candidate is tested with the reference's own expression, so the matched lists -- in sorted order -- are exactly
// fvad_stats_from_segments'.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/fvad.h"
#include "vad_machine.h" // FVAD_HD

namespace fvad_eval {

// std::max / std::min as <algorithm> defines them (the argument order matters for signed zeros)
FVAD_HD inline float smax(float a, float b) { return (a < b) ? b : a; }
FVAD_HD inline float smin(float a, float b) { return (b < a) ? b : a; }

FVAD_HD inline float overlap_with(float af, float at, float bf, float bt) // SpeechSegment.zig:22-27
{
    return smin(at, bt) - smax(af, bf);
}

// first index in [0, n) whose key(i) is > x (keys non-decreasing), n if none
template <class Key> FVAD_HD inline uint32_t first_above(Key key, uint32_t n, float x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key(mid) > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
// first index in [0, n) whose key(i) is >= x (keys non-decreasing), n if none
template <class Key> FVAD_HD inline uint32_t first_not_below(Key key, uint32_t n, float x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (!(key(mid) < x)) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// vad(i) -> fvad_segment_sec of the machine's segment i (time order); ref / pmax: the stream's sorted labels and prefix max of
// their ends.  Labels are never NaN (fvad_vad_batch_set_references refuses them), so the searches see ordered keys.
template <class Vad>
FVAD_HD inline fvad_single_stats score_walk(Vad vad, uint32_t n_vad, const fvad_segment_sec* ref, const float* pmax, uint32_t n_ref,
                                            const fvad_stat_config& cfg)
{
    fvad_single_stats st;
    st.total_positives_sec = 0; st.true_positives_sec = 0; st.false_positives_sec = 0; st.false_negatives_sec = 0;
    st.true_positive_rate = 0; st.false_negative_rate = 0; st.false_discovery_rate = 0; st.precision = 0;
    st.fm_index = 0; st.f_score = 0; st.f_score_beta = 0;
    for (uint32_t i = 0; i < n_vad; ++i) { // statistics.zig:88-94
        const fvad_segment_sec s = vad(i);
        const uint32_t j0 = first_above([&](uint32_t j) { return pmax[j]; }, n_ref, s.from_sec);
        const uint32_t j1 = first_not_below([&](uint32_t j) { return ref[j].from_sec; }, n_ref, s.to_sec);
        // calcFalsePositiveSec on the extruded clone of the matched labels (statistics.zig:191-203,229-256), one matched label
        // of look-ahead: a matched label's end is final once the next one is known (fill_gaps) or the list has ended (extrude_end)
        float overlap = 0.0f;
        bool have = false, first = true;
        float pf = 0, pt = 0; // the pending matched label: start (already extruded if it is the first), end
        for (uint32_t j = j0; j < j1; ++j) {
            const fvad_segment_sec r = ref[j];
            if (!(overlap_with(s.from_sec, s.to_sec, r.from_sec, r.to_sec) > 0.0f)) continue;
            if (have) {
                const float to = (r.from_sec - pt <= cfg.fill_gaps) ? r.from_sec : pt;
                overlap += smax(0.0f, overlap_with(s.from_sec, s.to_sec, pf, to));
            }
            pf = first ? r.from_sec - cfg.extrude_start : r.from_sec;
            pt = r.to_sec;
            have = true;
            first = false;
        }
        if (have) overlap += smax(0.0f, overlap_with(s.from_sec, s.to_sec, pf, pt + cfg.extrude_end));
        const float dur = s.to_sec - s.from_sec;
        const float fp = smax(0.0f, dur - overlap);
        st.false_positives_sec += fp;
        const float tp = smax(0.0f, dur - fp); // calcTruePositiveSec :205-214
        st.true_positives_sec += tp;
        st.total_positives_sec += tp;
    }
    for (uint32_t j = 0; j < n_ref; ++j) { // :96-102
        const fvad_segment_sec r = ref[j];
        const float dur = r.to_sec - r.from_sec;
        if (dur < cfg.ignore_shorter_than_sec) continue;
        const uint32_t i0 = first_above([&](uint32_t i) { return vad(i).to_sec; }, n_vad, r.from_sec);
        const uint32_t i1 = first_not_below([&](uint32_t i) { return vad(i).from_sec; }, n_vad, r.to_sec);
        float overlap = 0.0f; // calcOverlapWithMatches :274-278
        for (uint32_t i = i0; i < i1; ++i) {
            const fvad_segment_sec s = vad(i);
            const float o = overlap_with(r.from_sec, r.to_sec, s.from_sec, s.to_sec);
            if (o > 0.0f) overlap += smax(0.0f, o);
        }
        const float fn = smax(0.0f, dur - overlap);
        st.false_negatives_sec += fn;
        st.total_positives_sec += fn;
    }
    st.true_positive_rate = st.true_positives_sec / st.total_positives_sec;
    st.false_negative_rate = st.false_negatives_sec / st.total_positives_sec;
    st.false_discovery_rate = st.false_positives_sec / (st.false_positives_sec + st.true_positives_sec);
    st.precision = st.true_positives_sec / (st.true_positives_sec + st.false_positives_sec);
    st.f_score_beta = 0.7f;
    const float b2 = st.f_score_beta * st.f_score_beta; // :175-182
    st.f_score = (1 + b2) * (st.precision * st.true_positive_rate) / (b2 * st.precision + st.true_positive_rate);
    st.fm_index = sqrtf(st.precision * st.true_positive_rate);
    return st;
}

} // namespace fvad_eval
