// Sanitizer driver for the host scorer of a VAD batch (no GPU): built by tests/test_sanitizers_eval.py with
// -fsanitize=address,undefined from host_vad.cpp, host_stats.cpp and host_eval.cpp.
//   eval_san <seed>   a sweep batch of ragged random streams run on the host, scored against random labels (ragged offsets,
//                     empty streams, overlapping, unsorted and zero-length labels) on 1 and 7 threads: every machine bit for bit
//                     fvad_stats_from_segments, both thread counts alike; then the argument checks.  Prints "ok segments=N machines=M".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "fvad.h"

#define CHECK(x)                                                                   \
    do {                                                                           \
        if (!(x)) { fprintf(stderr, "check failed: %s (line %d)\n", #x, __LINE__); return 1; } \
    } while (0)

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    std::mt19937_64 rng(strtoull(argv[1], nullptr, 10));
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    const size_t S = 6, NC = 5, C = 2, F = 1024, FS = 48000, CHUNK = 24000, n_chunks = 120, nf = n_chunks * CHUNK / F;
    std::vector<fvad_vad_config> cfgs(NC);
    for (size_t c = 0; c < NC; ++c) {
        fvad_vad_config_default(&cfgs[c]);
        cfgs[c].long_term_speech_avg_sec = (float)uni(3.0, 20.0);
        cfgs[c].has_initial_long_term_avg = c % 2;
        cfgs[c].speech_threshold_factor = (float)uni(1.5, 4.0);
        cfgs[c].max_speech_gap_sec = (float)uni(0.0, 2.0);
        cfgs[c].min_vad_duration_sec = (float)uni(0.0, 1.0);
    }
    cfgs[NC - 1].speech_threshold_factor = 1e9f; // never opens: machines without segments
    fvad_vad_batch* b = nullptr;
    CHECK(fvad_vad_batch_create_sweep(cfgs.data(), NC, FS, C, F, S, &b) == FVAD_OK);
    size_t n_bands = 0;
    fvad_vad_batch_bands(b, nullptr, 0, &n_bands, nullptr);
    // band sums: a floor with bursts, per stream; chunk RMS following them
    std::vector<float> band(n_bands * S * C * nf), rms(S * C * n_chunks);
    for (size_t s = 0; s < S; ++s) {
        std::vector<char> on(nf, 0);
        for (double t = uni(0, 3); t < nf * (double)F / FS; t += uni(1, 8)) {
            const double d = uni(0.3, 4.0);
            for (size_t k = (size_t)(t * FS / F); k < nf && k < (size_t)((t + d) * FS / F); ++k) on[k] = 1;
            t += d;
        }
        for (size_t j = 0; j < n_bands; ++j)
            for (size_t ch = 0; ch < C; ++ch)
                for (size_t k = 0; k < nf; ++k)
                    band[((j * S + s) * C + ch) * nf + k] = (float)(0.01 * uni(0.5, 2.0) + (on[k] ? uni(0.2, 2.0) : 0.0));
        for (size_t ch = 0; ch < C; ++ch)
            for (size_t k = 0; k < n_chunks; ++k) rms[(s * C + ch) * n_chunks + k] = (float)uni(0.01, 0.2);
    }
    CHECK(fvad_vad_batch_run(b, band.data(), nf, nf, rms.data(), n_chunks, n_chunks, CHUNK, 4) == FVAD_OK);
    // labels: ragged offsets, stream 1 and the last stream without any
    std::vector<fvad_segment_sec> refs;
    std::vector<size_t> offs(S + 1, 0);
    const double dur = nf * (double)F / FS;
    for (size_t s = 0; s < S; ++s) {
        const size_t n = (s == 1 || s == S - 1) ? 0 : (size_t)uni(1, 40);
        for (size_t i = 0; i < n; ++i) {
            const float a = (float)uni(0, dur);
            const int kind = (int)uni(0, 4);
            const float len = kind == 0 ? 0.0f : kind == 1 ? (float)uni(0, 0.2) : kind == 2 ? (float)uni(10, 40) : (float)uni(0.2, 8);
            refs.push_back({a, a + len});
        }
        offs[s + 1] = refs.size();
    }
    std::vector<fvad_stat_config> scs(NC);
    for (size_t c = 0; c < NC; ++c) scs[c] = {cfgs[c].min_vad_duration_sec, (float)uni(0, 6), (float)uni(0, 12), (float)uni(0, 6)};
    CHECK(fvad_vad_batch_config_stats(b, 0, nullptr) == FVAD_ERR_INVALID_ARGUMENT);
    CHECK(fvad_vad_batch_set_references(b, refs.data(), offs.data(), scs.data()) == FVAD_OK);
    std::vector<fvad_single_stats> one(S), many(S);
    size_t machines = 0, n_segs = 0;
    for (size_t c = 0; c < NC; ++c) {
        CHECK(fvad_vad_batch_score(b, 1) == FVAD_OK);
        CHECK(fvad_vad_batch_config_stats(b, c, one.data()) == FVAD_OK);
        CHECK(fvad_vad_batch_score(b, 7) == FVAD_OK);
        CHECK(fvad_vad_batch_config_stats(b, c, many.data()) == FVAD_OK);
        CHECK(memcmp(one.data(), many.data(), S * sizeof(fvad_single_stats)) == 0);
        std::vector<size_t> so(S + 1);
        fvad_vad_batch_config_segments(b, c, nullptr, 0, so.data());
        std::vector<fvad_speech_segment> segs(so[S] + 1);
        CHECK(fvad_vad_batch_config_segments(b, c, segs.data(), segs.size(), so.data()) == FVAD_OK);
        n_segs += so[S];
        for (size_t s = 0; s < S; ++s) {
            std::vector<fvad_segment_sec> secs;
            for (size_t i = so[s]; i < so[s + 1]; ++i) secs.push_back(fvad_segment_to_sec(&segs[i], FS));
            fvad_single_stats want;
            CHECK(fvad_stats_from_segments(secs.data(), secs.size(), refs.data() + offs[s], offs[s + 1] - offs[s], &scs[c], &want) == FVAD_OK);
            CHECK(memcmp(&want, &one[s], sizeof want) == 0);
            ++machines;
        }
    }
    CHECK(n_segs > 50); // (the machines open and close)
    // argument checks
    std::vector<size_t> bad = offs;
    bad[2] = bad[3] + 1; // not monotone
    CHECK(fvad_vad_batch_set_references(b, refs.data(), bad.data(), scs.data()) == FVAD_ERR_INVALID_ARGUMENT);
    bad = offs;
    bad[0] = 1;
    CHECK(fvad_vad_batch_set_references(b, refs.data(), bad.data(), scs.data()) == FVAD_ERR_INVALID_ARGUMENT);
    CHECK(fvad_vad_batch_config_stats(b, NC, one.data()) == FVAD_ERR_INVALID_ARGUMENT);
    fvad_vad_batch_destroy(b);
    printf("ok segments=%zu machines=%zu\n", n_segs, machines);
    return 0;
}
