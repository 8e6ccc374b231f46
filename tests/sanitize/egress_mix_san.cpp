// egress_mix_san.cpp -- the host-only half of the two-source egress (csrc/host_egress_mix.cpp) under AddressSanitizer + UBSan:
// fvad_nsnet2_delay over seeded random rates and fvad_egress_mix_check over seeded random row tables and weights, with values
// near UINT64_MAX for the overflow paths; whatever is accepted must lie inside both lane sets and the output bytes.  Built by
// tests/test_sanitizers_egress_mix.py; never loaded into Python.
//   usage: egress_mix_san <seed>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "fvad.h"

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: egress_mix_san <seed>\n"); return 2; }
    std::mt19937_64 rng((uint64_t)atoll(argv[1]));
    auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    auto near_max = [&]() -> uint64_t {
        switch (pick(6)) {
        case 0: return UINT64_MAX - pick(4);
        case 1: return (UINT64_MAX >> pick(4)) + pick(3);
        case 2: return (1ull << 63) + pick(5) - 2;
        default: return pick(200);
        }
    };
    auto weight = [&]() -> float {
        switch (pick(10)) {
        case 0: return 0.0f;
        case 1: return -0.0f;
        case 2: return std::numeric_limits<float>::quiet_NaN();
        case 3: return pick(2) ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity();
        case 4: return std::numeric_limits<float>::denorm_min();
        default: return (float)((double)pick(4001) / 1000.0 - 2.0);
        }
    };
    long delays = 0, ok_delays = 0, tables = 0, ok_tables = 0;

    // ---- fvad_nsnet2_delay
    for (int round = 0; round < 2000; ++round) {
        const size_t rate = pick(3) == 0 ? (size_t)near_max() : pick(2) ? 16000 * (size_t)pick(8) : (size_t)pick(200000);
        uint64_t d = 12345;
        const int rc = fvad_nsnet2_delay(rate, pick(50) == 0 ? nullptr : &d);
        ++delays;
        if (rc == FVAD_OK) {
            ++ok_delays;
            if (rate == 0 || rate % 16000 != 0 || d != 161 * (uint64_t)(rate / 16000) - 1) { fprintf(stderr, "a wrong delay (round %d)\n", round); return 4; }
        } else if (rc != FVAD_ERR_INVALID_SAMPLE_RATE && rc != FVAD_ERR_INVALID_ARGUMENT) { fprintf(stderr, "an unexpected status %d\n", rc); return 6; }
    }

    // ---- fvad_egress_mix_check
    for (int round = 0; round < 4000; ++round) {
        const size_t n = (size_t)pick(7);
        const bool wild = pick(3) == 0;
        const size_t n_lanes = wild && pick(4) == 0 ? (size_t)near_max() : 1 + (size_t)pick(12);
        const size_t den_samples = wild && pick(4) == 0 ? (size_t)near_max() : (size_t)pick(300);
        const size_t den_stride = wild && pick(4) == 0 ? (size_t)near_max() : den_samples + (size_t)pick(3);
        const size_t orig_samples = wild && pick(4) == 0 ? (size_t)near_max() : (size_t)pick(300);
        const size_t orig_stride = wild && pick(4) == 0 ? (size_t)near_max() : orig_samples + (size_t)pick(3);
        const uint64_t out_bytes = pick(3) == 0 ? UINT64_MAX : wild ? near_max() : pick(20000);
        const float w_orig = weight(), w_den = weight();
        std::vector<uint64_t> rows(n * FVAD_EGRESS_MIX_FIELDS + 1);
        uint64_t at = pick(50);
        for (size_t i = 0; i < n; ++i) {
            uint64_t* r = &rows[i * FVAD_EGRESS_MIX_FIELDS];
            r[1] = wild && pick(3) == 0 ? near_max() : pick(40);
            r[2] = wild && pick(5) == 0 ? near_max() : 1 + pick(pick(8) ? 4 : 70);
            r[3] = pick(12) == 0 ? near_max() : pick(3);
            r[4] = wild && pick(4) == 0 ? near_max() : pick(12);
            r[5] = wild && pick(3) == 0 ? near_max() : pick(250);
            r[6] = wild && pick(3) == 0 ? near_max() : pick(250);
            r[7] = pick(4) == 0 ? near_max() : pick(50);
            // mostly one behind the other (so that tables are accepted), sometimes anywhere
            r[0] = wild && pick(3) == 0 ? near_max() : pick(4) == 0 ? pick(4000) : at;
            at = r[0] + r[1] * r[2] * 4 + pick(3); // (wraps with wild values: unsigned, and then just another offset)
        }
        const int src_format = pick(20) == 0 ? (int)pick(5) - 1 : FVAD_INGEST_F32;
        const int rc = fvad_egress_mix_check(n ? rows.data() : (pick(2) ? rows.data() : nullptr), n, out_bytes, src_format, w_orig, w_den, n_lanes,
                                             orig_stride, orig_samples, den_stride, den_samples);
        ++tables;
        if (rc == FVAD_OK) ++ok_tables;
        else if (rc != FVAD_ERR_INVALID_ARGUMENT && rc != FVAD_ERR_OUT_OF_RANGE) { fprintf(stderr, "an unexpected status %d\n", rc); return 6; }
        if (rc == FVAD_OK) {
            if (!std::isfinite(w_orig) || !std::isfinite(w_den) || (w_orig == 0.0f && w_den == 0.0f) || src_format != FVAD_INGEST_F32) { fprintf(stderr, "bad weights or lanes accepted (round %d)\n", round); return 7; }
        }
        if (rc == FVAD_OK && n) { // what is accepted stays inside the lanes it reads and the output bytes, without wrapping, and no two sinks share a byte
            const bool uo = w_orig != 0.0f, ud = w_den != 0.0f;
            if (n_lanes > 1 && ((uo && orig_stride < orig_samples) || (ud && den_stride < den_samples))) { fprintf(stderr, "overlapping lanes accepted (round %d)\n", round); return 7; }
            for (size_t i = 0; i < n; ++i) {
                const uint64_t* r = &rows[i * FVAD_EGRESS_MIX_FIELDS];
                const uint64_t fb = r[2] * (r[3] == FVAD_INGEST_PCM16 ? 2 : r[3] == FVAD_INGEST_PCM24 ? 3 : 4);
                const uint64_t n_read = r[1] - (r[7] < r[1] ? r[7] : r[1]);
                if (r[2] < 1 || r[2] > 64 || r[3] > 2 || r[4] >= n_lanes || r[2] > n_lanes - r[4] || (ud && (r[5] > den_samples || r[1] > den_samples - r[5])) ||
                    (uo && (r[6] > orig_samples || n_read > orig_samples - r[6])) || r[0] > out_bytes || r[1] > (out_bytes - r[0]) / fb) {
                    fprintf(stderr, "an accepted table is out of range (round %d)\n", round); return 7;
                }
                for (size_t k = 0; k < i; ++k) {
                    const uint64_t* q = &rows[k * FVAD_EGRESS_MIX_FIELDS];
                    const uint64_t qb = q[1] * q[2] * (q[3] == FVAD_INGEST_PCM16 ? 2 : q[3] == FVAD_INGEST_PCM24 ? 3 : 4);
                    if (r[1] && q[1] && r[0] < q[0] + qb && q[0] < r[0] + r[1] * fb) { fprintf(stderr, "two accepted sinks overlap (round %d)\n", round); return 7; }
                }
            }
        }
    }
    if (ok_tables == 0 || ok_tables == tables || ok_delays == 0 || ok_delays == delays) { fprintf(stderr, "the driver is one-sided: %ld of %ld tables, %ld of %ld delays\n", ok_tables, tables, ok_delays, delays); return 8; }
    printf("delays=%ld accepted=%ld tables=%ld ok=%ld\n", delays, ok_delays, tables, ok_tables);
    return 0;
}
