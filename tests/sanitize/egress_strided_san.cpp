// egress_strided_san.cpp -- the host-only half of the strided resampling egress (csrc/host_egress_strided.cpp, with
// csrc/host_egress_resample.cpp and the ratio and window rules of csrc/host_resample.cpp) under AddressSanitizer + UBSan:
// fvad_egress_resample_strided_check over seeded random row tables with random steps -- half of them built to be acceptable, the
// others wild, with values near UINT64_MAX -- checking that whatever is accepted lies inside its lanes, counted `step` apart and
// without wrapping, and inside its bytes, and is given the window it reads; and that with step 1 the status is
// fvad_egress_resample_check's.  Built by tests/test_sanitizers_egress_strided.py; never loaded into Python.
//   usage: egress_strided_san <seed>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fvad.h"

typedef unsigned __int128 u128;

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: egress_strided_san <seed>\n"); return 2; }
    std::mt19937_64 rng((uint64_t)atoll(argv[1]));
    auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    auto near_max = [&]() -> uint64_t {
        switch (pick(6)) {
        case 0: return UINT64_MAX - pick(4);
        case 1: return (UINT64_MAX >> pick(4)) + pick(3);
        case 2: return (1ull << 63) + pick(5) - 2;
        case 3: return (1ull << 62) / (1 + pick(640)) + pick(5) - 2;
        default: return pick(200);
        }
    };
    auto sample_bytes = [](uint64_t f) -> uint64_t { return f == FVAD_INGEST_PCM16 ? 2 : f == FVAD_INGEST_PCM24 ? 3 : 4; };
    long tables = 0, ok_tables = 0, bad_steps = 0, step1 = 0;

    for (int round = 0; round < 6000; ++round) {
        const size_t n = (size_t)pick(7);
        const bool wild = pick(2) == 0;
        const uint32_t up = wild && pick(6) == 0 ? (uint32_t)near_max() : 1 + (uint32_t)pick(pick(2) ? 4 : 160);
        const uint32_t down = wild && pick(6) == 0 ? (uint32_t)near_max() : 1 + (uint32_t)pick(pick(2) ? 4 : 160);
        const uint32_t n_taps = wild && pick(6) == 0 ? (uint32_t)near_max() : 1 + 2 * (uint32_t)pick(60);
        const uint32_t step = wild && pick(5) == 0 ? (uint32_t)(pick(2) ? near_max() : pick(20)) : 1 + (uint32_t)pick(FVAD_EGRESS_STEP_MAX);
        std::vector<float> taps(n_taps >= 1 && n_taps <= 30000 ? n_taps : 1, 0.25f);
        if (wild && pick(10) == 0) taps[pick(taps.size())] = 1.0f / 0.0f;
        const size_t n_lanes = wild && pick(4) == 0 ? (size_t)near_max() : 1 + (size_t)pick(12);
        const size_t n_samples = wild && pick(4) == 0 ? (size_t)near_max() : 200 + (size_t)pick(300) * (step >= 1 && step <= 16 ? step : 1);
        const size_t lane_stride = wild && pick(4) == 0 ? (size_t)near_max() : n_samples + (size_t)pick(3);
        const uint64_t out_bytes = pick(3) == 0 ? UINT64_MAX : wild ? near_max() : 40000 + pick(20000);
        std::vector<uint64_t> rows(n * FVAD_EGRESS_RESAMPLE_FIELDS + 1);
        uint64_t at = pick(50);
        for (size_t i = 0; i < n; ++i) {
            uint64_t* r = &rows[i * FVAD_EGRESS_RESAMPLE_FIELDS];
            // a row that would pass: a stream, a range of its outputs, their window (the library's own) widened a little
            const uint64_t sf = pick(400), of = fvad_resample_out_frames(sf, up ? up : 1, down ? down : 1);
            r[8] = sf;
            r[9] = of ? pick(of + 1) : 0;
            r[1] = of > r[9] ? pick(std::min<uint64_t>(of - r[9], 40) + 1) : 0;
            uint64_t lo = 0, hi = 0;
            (void)fvad_resample_window(up, down, n_taps, sf, r[9], r[1], &lo, &hi); // (refused for a ratio that is none: 0, 0)
            r[6] = lo - std::min<uint64_t>(lo, pick(3));
            r[7] = std::min<uint64_t>(hi + pick(3), sf) - r[6];
            r[2] = 1 + pick(pick(8) ? 4 : 64);
            r[3] = pick(3);
            r[4] = pick(12);
            r[5] = pick(60);
            r[0] = pick(4) == 0 ? pick(4000) : at;
            if (wild) { // ... and then anything anywhere
                for (int f = 0; f < FVAD_EGRESS_RESAMPLE_FIELDS; ++f)
                    if (pick(8) == 0) r[f] = pick(3) ? near_max() : r[f] + pick(3) - 1;
            }
            at = r[0] + r[1] * r[2] * 4 + pick(3); // (wraps with wild values: unsigned, and then just another offset)
        }
        const int src_format = pick(20) == 0 ? (int)pick(5) - 1 : FVAD_INGEST_F32;
        const bool null_taps = wild && pick(30) == 0;
        const uint64_t* table = n ? rows.data() : (pick(2) ? rows.data() : nullptr);
        const uint32_t nt = n_taps <= 30000 ? n_taps : n_taps % 2 ? 30001 : 30000;
        const int rc = fvad_egress_resample_strided_check(table, n, out_bytes, up, down, null_taps ? nullptr : taps.data(), nt, step, src_format, n_lanes,
                                                          lane_stride, n_samples);
        ++tables;
        const bool step_ok = step >= 1 && step <= FVAD_EGRESS_STEP_MAX;
        if (!step_ok) ++bad_steps;
        if (rc == FVAD_OK) ++ok_tables;
        else if (rc != FVAD_ERR_INVALID_ARGUMENT && rc != FVAD_ERR_OUT_OF_RANGE) { fprintf(stderr, "an unexpected status %d\n", rc); return 6; }
        if (step == 1) { // the parent's rules: the same status, but for a row without frames whose src_offset lies past the lane
            const int parent = fvad_egress_resample_check(table, n, out_bytes, up, down, null_taps ? nullptr : taps.data(), nt, src_format, n_lanes, lane_stride, n_samples);
            ++step1;
            bool empty_past = false;
            for (size_t i = 0; i < n; ++i) empty_past |= rows[i * FVAD_EGRESS_RESAMPLE_FIELDS + 7] == 0 && rows[i * FVAD_EGRESS_RESAMPLE_FIELDS + 5] > n_samples;
            if (parent != rc && !empty_past) { fprintf(stderr, "step 1 is not the parent's check: %d, %d (round %d)\n", rc, parent, round); return 9; }
        }
        if (rc != FVAD_OK) continue;
        // what is accepted has a ratio, a step and taps, stays inside the lanes and the output bytes without wrapping, is given the
        // window it reads, and no two rows share a byte
        if (src_format != FVAD_INGEST_F32 || up < 1 || up > FVAD_RESAMPLE_UP_MAX || down < 1 || !step_ok || n_taps % 2 == 0 ||
            n_taps > FVAD_RESAMPLE_TAPS_MAX || null_taps) {
            fprintf(stderr, "accepted without a ratio, a step or taps (round %d)\n", round); return 7;
        }
        for (size_t i = 0; i < n; ++i) {
            const uint64_t* r = &rows[i * FVAD_EGRESS_RESAMPLE_FIELDS];
            const uint64_t fb = r[2] * sample_bytes(r[3]);
            uint64_t lo = 0, hi = 0;
            // the last strided sample of the given frames, in 128 bits: below n_samples
            const bool in_lane = r[7] == 0 || (u128)r[5] + (u128)(r[7] - 1) * step < (u128)n_samples;
            if (r[2] < 1 || r[2] > 64 || r[3] > 2 || r[4] >= n_lanes || r[2] > n_lanes - r[4] || !in_lane ||
                r[0] > out_bytes || r[1] > (out_bytes - r[0]) / fb || (n_lanes > 1 && lane_stride < n_samples) ||
                (u128)r[8] * up >= ((u128)1 << 62) || (u128)r[9] + r[1] > fvad_resample_out_frames(r[8], up, down) || (u128)r[6] + r[7] > r[8] ||
                fvad_egress_resample_tile(up, down, n_taps, (uint32_t)r[2], (uint32_t)r[3]) == 0 ||
                fvad_resample_window(up, down, n_taps, r[8], r[9], r[1], &lo, &hi) != FVAD_OK || (hi > lo && (r[6] > lo || r[6] + r[7] < hi))) {
                fprintf(stderr, "an accepted table is out of range (round %d)\n", round); return 7;
            }
            for (size_t k = 0; k < i; ++k) {
                const uint64_t* q = &rows[k * FVAD_EGRESS_RESAMPLE_FIELDS];
                const uint64_t qb = q[1] * q[2] * sample_bytes(q[3]);
                if (r[1] && q[1] && r[0] < q[0] + qb && q[0] < r[0] + r[1] * fb) { fprintf(stderr, "two accepted rows overlap (round %d)\n", round); return 7; }
            }
        }
    }
    if (ok_tables * 10 < tables || ok_tables == tables || bad_steps == 0 || step1 == 0) {
        fprintf(stderr, "the driver is one-sided: %ld of %ld tables, %ld bad steps, %ld at step 1\n", ok_tables, tables, bad_steps, step1); return 8;
    }
    printf("tables=%ld ok=%ld bad_steps=%ld step1=%ld\n", tables, ok_tables, bad_steps, step1);
    return 0;
}
