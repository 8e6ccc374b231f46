// resample_san.cpp -- the host-only half of the resampling ingest (csrc/host_resample.cpp) under AddressSanitizer + UBSan:
// fvad_resample_ratio / _out_frames / _window / _design and fvad_ingest_resample_tile over seeded random arguments, and
// fvad_ingest_resample_check over seeded random source tables and ratios with values near UINT64_MAX for the overflow paths.
// Whatever the check accepts must lie inside its bytes, its file and its lanes, and its given frames must hold every frame its
// outputs read (recomputed here in 128-bit arithmetic).  Built by tests/test_sanitizers_resample.py; never loaded into Python.
//   usage: resample_san <seed>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fvad.h"

typedef unsigned __int128 u128;

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: resample_san <seed>\n"); return 2; }
    std::mt19937_64 rng((uint64_t)atoll(argv[1]));
    auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    auto near_max = [&]() -> uint64_t {
        switch (pick(6)) {
        case 0: return UINT64_MAX - pick(4);
        case 1: return (UINT64_MAX >> pick(4)) + pick(3);
        case 2: return (1ull << 63) + pick(5) - 2;
        case 3: return (1ull << (40 + pick(23))) + pick(5) - 2;
        default: return pick(200);
        }
    };
    auto any_u32 = [&]() -> uint32_t {
        switch (pick(5)) {
        case 0: return UINT32_MAX - (uint32_t)pick(3);
        case 1: return (uint32_t)pick(3);
        case 2: return 638 + (uint32_t)pick(5);
        default: return 1 + (uint32_t)pick(700);
        }
    };
    long ratios = 0, windows = 0, designs = 0, tables = 0, ok_tables = 0, ok_rows = 0;

    // ---- the ratio, the output count, the window, the tile
    for (int round = 0; round < 3000; ++round) {
        uint32_t up = 77, down = 77;
        const uint32_t rin = pick(4) ? (uint32_t)pick(200000) : any_u32(), rout = pick(4) ? 48000 : any_u32();
        const int rc = fvad_resample_ratio(rin, rout, pick(40) ? &up : nullptr, &down);
        ++ratios;
        if (rc == FVAD_OK) {
            if (up < 1 || up > FVAD_RESAMPLE_UP_MAX || down < 1 || (u128)rin * up != (u128)rout * down) { fprintf(stderr, "a wrong ratio %u/%u for %u -> %u\n", up, down, rin, rout); return 4; }
        } else if (rc != FVAD_ERR_INVALID_ARGUMENT || up != 77 || down != 77) { fprintf(stderr, "a refused ratio wrote its outputs\n"); return 4; }
        const uint32_t u = pick(3) ? 1 + (uint32_t)pick(640) : any_u32(), d = pick(3) ? 1 + (uint32_t)pick(700) : any_u32();
        const uint32_t n_taps = pick(6) ? 2 * (uint32_t)pick(10241) + 1 : any_u32();
        const uint64_t ff = pick(2) ? pick(100000) : near_max(), from = pick(2) ? pick(100000) : near_max(), n = pick(2) ? pick(5000) : near_max();
        (void)fvad_resample_out_frames(ff, u, d);
        (void)fvad_ingest_resample_tile(u, d, n_taps, (uint32_t)pick(70), (uint32_t)pick(5));
        uint64_t lo = 1, hi = 0;
        const int rw = fvad_resample_window(u, d, n_taps, ff, from, n, pick(40) ? &lo : nullptr, &hi);
        ++windows;
        if (rw == FVAD_OK && !(lo <= hi && hi <= ff)) { fprintf(stderr, "a window outside its file\n"); return 5; }
    }
    // ---- the design (a few: the largest is 20481 taps)
    std::vector<float> taps(FVAD_RESAMPLE_TAPS_MAX + 1, -7.0f);
    for (int round = 0; round < 60; ++round) {
        const uint32_t u = pick(3) ? 1 + (uint32_t)pick(640) : any_u32(), d = pick(3) ? 1 + (uint32_t)pick(200) : any_u32();
        const uint32_t half = pick(4) ? (uint32_t)pick(40) : any_u32();
        const double cutoff = pick(4) ? 0.0 : pick(2) ? 0.6 * (double)pick(1000) / 1000.0 : NAN;
        const double beta = pick(4) ? 0.0 : pick(2) ? (double)pick(2000) - 10.0 : INFINITY;
        uint32_t n = 0;
        taps[FVAD_RESAMPLE_TAPS_MAX] = -7.0f;
        const int rc = fvad_resample_design(u, d, half, cutoff, beta, taps.data(), &n);
        ++designs;
        if (taps[FVAD_RESAMPLE_TAPS_MAX] != -7.0f) { fprintf(stderr, "the design wrote past FVAD_RESAMPLE_TAPS_MAX\n"); return 6; }
        if (rc == FVAD_OK) {
            double sum = 0;
            if (n % 2 == 0 || n > FVAD_RESAMPLE_TAPS_MAX) { fprintf(stderr, "a design of %u taps\n", n); return 6; }
            for (uint32_t k = 0; k < n; ++k) { if (!std::isfinite(taps[k])) { fprintf(stderr, "a design with a tap that is not finite\n"); return 6; } sum += taps[k]; }
            if (std::fabs(sum - u) > 1e-3 * u) { fprintf(stderr, "a design that sums to %g, not %u\n", sum, u); return 6; }
        } else if (rc != FVAD_ERR_INVALID_ARGUMENT) { fprintf(stderr, "an unexpected status %d\n", rc); return 6; }
    }

    // ---- fvad_ingest_resample_check
    std::vector<float> some(4097);
    for (float& t : some) t = (float)pick(2001) / 1000.0f - 1.0f;
    for (int round = 0; round < 4000; ++round) {
        const size_t n = (size_t)pick(6);
        const bool wild = pick(3) == 0;
        const uint32_t up = wild && pick(3) == 0 ? any_u32() : 1 + (uint32_t)pick(12), down = wild && pick(3) == 0 ? any_u32() : 1 + (uint32_t)pick(12);
        const uint32_t n_taps = pick(15) == 0 ? any_u32() : 2 * (uint32_t)pick(40) + 1;
        const size_t n_lanes = wild && pick(4) == 0 ? (size_t)near_max() : 6 + (size_t)pick(12);
        const size_t n_samples = wild && pick(4) == 0 ? (size_t)near_max() : 200 + (size_t)pick(300);
        const size_t lane_stride = wild && pick(4) == 0 ? (size_t)near_max() : n_samples + (size_t)pick(3);
        const uint64_t raw_bytes = pick(3) == 0 ? UINT64_MAX : wild ? near_max() : pick(20000);
        std::vector<uint64_t> rows(n * FVAD_RESAMPLE_FIELDS + 1);
        for (size_t i = 0; i < n; ++i) {
            uint64_t* r = &rows[i * FVAD_RESAMPLE_FIELDS];
            const bool w = wild && pick(2) == 0;
            r[2] = w && pick(5) == 0 ? near_max() : 1 + pick(pick(8) ? 4 : 70);
            r[3] = pick(12) == 0 ? near_max() : pick(3);
            r[8] = w && pick(3) == 0 ? near_max() : pick(120);                                     // file_frames
            const u128 of = ((u128)r[8] * up + down - 1) / (down ? down : 1);
            r[9] = w && pick(3) == 0 ? near_max() : pick((uint64_t)(of < 400 ? of : 400) + 2);     // out_from
            r[10] = w && pick(3) == 0 ? near_max() : pick(40);                                     // n_out
            // mostly the whole file or the window with a frame more or fewer, so that a good share passes
            uint64_t lo = 0, hi = 0;
            if (pick(2)) (void)fvad_resample_window(up, down, n_taps, r[8], r[9], r[10], &lo, &hi);
            else hi = r[8];
            r[7] = w && pick(3) == 0 ? near_max() : lo + (pick(8) == 0) - (pick(8) == 0 && lo > 0);
            r[1] = w && pick(3) == 0 ? near_max() : (hi >= r[7] ? hi - r[7] : 0) + (pick(8) == 0) - (pick(8) == 0 && hi > r[7]);
            r[0] = w && pick(3) == 0 ? near_max() : pick(4000);
            r[4] = w && pick(4) == 0 ? near_max() : pick(8);
            r[5] = w && pick(3) == 0 ? near_max() : 50 * i + pick(4); // (rows that do not overlap, mostly)
            r[6] = w && pick(3) == 0 ? near_max() : r[5] + r[10] + pick(6) - (pick(12) == 0);
        }
        const int out_format = pick(20) == 0 ? (int)pick(5) - 1 : 0;
        const float* tp = pick(40) ? some.data() : nullptr;
        const int rc = fvad_ingest_resample_check(n ? rows.data() : (pick(2) ? rows.data() : nullptr), n, raw_bytes, up, down, tp, n_taps, out_format,
                                                  n_lanes, lane_stride, n_samples);
        ++tables;
        if (rc == FVAD_OK) { ++ok_tables; ok_rows += (long)n; }
        else if (rc != FVAD_ERR_INVALID_ARGUMENT && rc != FVAD_ERR_OUT_OF_RANGE) { fprintf(stderr, "an unexpected status %d\n", rc); return 7; }
        if (rc != FVAD_OK) continue;
        if (out_format != FVAD_INGEST_F32 || up < 1 || up > FVAD_RESAMPLE_UP_MAX || down < 1 || !tp || n_taps % 2 == 0 || n_taps > 4097) { fprintf(stderr, "accepted arguments that are none (round %d)\n", round); return 8; }
        const u128 K = (n_taps - 1) / 2;
        for (size_t i = 0; i < n; ++i) {
            const uint64_t* r = &rows[i * FVAD_RESAMPLE_FIELDS];
            const uint64_t fb = r[2] * (r[3] == FVAD_INGEST_PCM16 ? 2 : r[3] == FVAD_INGEST_PCM24 ? 3 : 4);
            const u128 of = ((u128)r[8] * up + down - 1) / down;
            bool good = r[2] >= 1 && r[2] <= 64 && r[3] <= 2 && (u128)r[4] + r[2] <= n_lanes && r[6] <= n_samples && (u128)r[5] + r[10] <= r[6] &&
                        (u128)r[7] + r[1] <= r[8] && (u128)r[9] + r[10] <= of && r[0] <= raw_bytes && (u128)r[1] * fb <= (u128)(raw_bytes - r[0]) &&
                        (u128)r[8] * up < ((u128)1 << 62);
            // every frame an output reads is a given frame
            for (uint64_t o = r[9]; good && o < r[9] + r[10]; ++o) {
                const u128 p = (u128)o * down;
                u128 first = p > K ? (p - K + up - 1) / up : 0, last = (p + K) / up; // frames first .. last, clipped to the file
                if (last >= r[8]) { if (r[8] == 0) continue; last = r[8] - 1; }
                if (first > last) continue;
                good = first >= r[7] && last < (u128)r[7] + r[1];
            }
            if (!good) { fprintf(stderr, "an accepted table is out of range (round %d, row %zu)\n", round, i); return 9; }
        }
    }
    if (ok_rows < 200 || ok_tables * 2 > tables) { fprintf(stderr, "the driver is one-sided: %ld of %ld tables, %ld accepted rows\n", ok_tables, tables, ok_rows); return 10; }
    printf("ratios=%ld windows=%ld designs=%ld tables=%ld ok=%ld rows=%ld\n", ratios, windows, designs, tables, ok_tables, ok_rows);
    return 0;
}
