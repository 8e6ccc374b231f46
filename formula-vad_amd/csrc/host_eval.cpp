// host_eval.cpp -- scoring a VAD batch against reference labels on the host: fvad_vad_batch_set_references, the host scorer
// fvad_vad_batch_score (the yardstick of the device scorer in kernels_eval.hip: both run eval_walk.h) and the score accessors.
// Evaluator.initAndRun (Evaluator.zig:90-111) per machine: the machine's segments converted to seconds as
// SimulationInstance.storeResult does (fvad_segment_to_sec), the stream's labels sorted once, statistics.fromEvaluator.
#include <algorithm>
#include <cmath>
#include <vector>

#include "eval_walk.h"
#include "host_vad.h"

extern "C" {

int fvad_vad_batch_set_references(fvad_vad_batch* b, const fvad_segment_sec* refs, const size_t* ref_offsets,
                                  const fvad_stat_config* stat_cfgs)
{
    if (!b || !ref_offsets || !stat_cfgs) return FVAD_ERR_INVALID_ARGUMENT;
    if (b->part_in_flight) return FVAD_ERR_INVALID_ARGUMENT; // (a device part in flight: fvad_vad_batch_part_wait first)
    const size_t S = b->n_streams, NC = b->cfgs.size();
    if (ref_offsets[0] != 0) return FVAD_ERR_INVALID_ARGUMENT;
    for (size_t s = 0; s < S; ++s)
        if (ref_offsets[s + 1] < ref_offsets[s]) return FVAD_ERR_INVALID_ARGUMENT;
    const size_t n = ref_offsets[S];
    if (n && !refs) return FVAD_ERR_INVALID_ARGUMENT;
    if (n > 0xFFFFFFFFu) return FVAD_ERR_INVALID_ARGUMENT; // (the walk indexes a stream's labels with 32 bits)
    for (size_t i = 0; i < n; ++i) // the walk's binary searches need ordered keys
        if (std::isnan(refs[i].from_sec) || std::isnan(refs[i].to_sec)) return FVAD_ERR_INVALID_ARGUMENT;
    std::vector<fvad_segment_sec> sorted(refs, refs + n);
    std::vector<float> pmax(n);
    auto by_start = [](const fvad_segment_sec& x, const fvad_segment_sec& y) { return x.from_sec < y.from_sec; };
    for (size_t s = 0; s < S; ++s) {
        // Evaluator.zig:95-111: std.mem.sort (stable) by start
        std::stable_sort(sorted.begin() + (long)ref_offsets[s], sorted.begin() + (long)ref_offsets[s + 1], by_start);
        float m = -INFINITY;
        for (size_t j = ref_offsets[s]; j < ref_offsets[s + 1]; ++j) pmax[j] = m = fvad_eval::smax(m, sorted[j].to_sec);
    }
    b->refs = std::move(sorted);
    b->ref_pmax = std::move(pmax);
    b->ref_off.assign(ref_offsets, ref_offsets + S + 1);
    b->stat_cfgs.assign(stat_cfgs, stat_cfgs + NC);
    b->has_refs = true;
    b->scored = false;
    return FVAD_OK;
}

int fvad_vad_batch_set_keep_segments(fvad_vad_batch* b, int keep)
{
    if (!b || b->part_in_flight) return FVAD_ERR_INVALID_ARGUMENT;
    b->keep_segments = keep != 0;
    return FVAD_OK;
}

int fvad_vad_batch_score(fvad_vad_batch* b, int n_threads)
{
    if (!b || !b->has_refs || !b->segs_kept || b->part_in_flight) return FVAD_ERR_INVALID_ARGUMENT;
    const size_t NC = b->cfgs.size(), M = b->n_streams * NC;
    const float sr = (float)b->sample_rate;
    std::vector<fvad_single_stats> out(M);
    auto score = [&](size_t m) {
        const size_t s = m / NC, c = m % NC;
        const std::vector<fvad_speech_segment>& v = b->segs[m];
        const size_t r0 = b->ref_off[s];
        // fvad_segment_to_sec's expression, (float)u64 / (float)sample_rate
        auto vad = [&](uint32_t i) { return fvad_segment_sec{(float)v[i].sample_from / sr, (float)v[i].sample_to / sr}; };
        out[m] = fvad_eval::score_walk(vad, (uint32_t)v.size(), b->refs.data() + r0, b->ref_pmax.data() + r0,
                                       (uint32_t)(b->ref_off[s + 1] - r0), b->stat_cfgs[c]);
    };
    fvad::deal(M, n_threads, score);
    b->scores = std::move(out);
    b->scored = true;
    return FVAD_OK;
}

int fvad_vad_batch_config_stats(const fvad_vad_batch* b, size_t config, fvad_single_stats* out)
{
    if (!b || !out || config >= b->cfgs.size() || !b->scored || b->part_in_flight) return FVAD_ERR_INVALID_ARGUMENT;
    const size_t NC = b->cfgs.size();
    for (size_t s = 0; s < b->n_streams; ++s) out[s] = b->scores[s * NC + config];
    return FVAD_OK;
}

} // extern "C"
