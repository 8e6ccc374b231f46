// clips_split_san.cpp -- fvad_clips_split_check (csrc/host_clips_split.cpp, host only) under AddressSanitizer + UBSan: seeded
// random tables of split clips, buffer shapes and addresses with values near UINT64_MAX for the overflow paths.  Whatever is
// accepted must lie inside its buffers without wrapping, give the slots fvad_clips_plan's rule gives, fit the capacity and
// leave the output's bytes clear of both sources.  Built by tests/test_sanitizers_clips_split.py; never loaded into Python.
//   usage: clips_split_san <seed>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fvad.h"

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: clips_split_san <seed>\n"); return 2; }
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
    long tables = 0, ok_tables = 0, by_status[4] = {0, 0, 0, 0};
    for (int round = 0; round < 6000; ++round) {
        const size_t n = (size_t)pick(7);
        const bool wild = pick(3) == 0, tame = !wild && pick(3) != 0; // tame: most rows inside their buffers, so that the later rules are reached
        auto dim = [&](uint64_t sane) { return (size_t)(wild && pick(4) == 0 ? near_max() : sane); };
        const int src_format = pick(20) == 0 ? (int)pick(5) - 1 : (int)pick(2), out_format = pick(20) == 0 ? (int)pick(5) - 1 : (int)pick(2);
        const uint64_t sb = src_format == FVAD_CLIP_PCM16 ? 2 : 4, ob = out_format == FVAD_CLIP_PCM16 ? 2 : 4;
        const size_t a_lanes = dim(tame ? 3 + pick(4) : pick(6)), a_samples = dim(tame ? 300 : pick(300)), a_stride = dim(a_samples + pick(3) - (pick(12) == 0 && a_samples));
        const size_t b_lanes = dim(tame ? 3 + pick(4) : 1 + pick(6)), b_samples = dim(tame ? 300 : pick(300)), b_stride = dim(b_samples + pick(3));
        // addresses only: nothing is read through them
        const uintptr_t d_a = pick(tame ? 40 : 8) == 0 ? 0 : (uintptr_t)(wild && pick(5) == 0 ? near_max() : 0x100000 + pick(64) * (pick(10) ? 4 : 1));
        const uintptr_t d_b = pick(tame ? 40 : 8) == 0 ? 0 : (uintptr_t)(wild && pick(5) == 0 ? near_max() : 0x200000 + pick(64) * (pick(10) ? 4 : 1));
        const uintptr_t out = pick(12) == 0 ? 0 : (uintptr_t)(wild && pick(5) == 0 ? near_max() : (pick(4) ? 0x800000 : 0x0ff000 + pick(0x102000)) + pick(8) * (pick(10) ? 16 : 2));
        const int device_out = (int)pick(2);
        std::vector<uint64_t> rows(n * FVAD_CLIP_SPLIT_FIELDS + 1), offsets(n + 1, 77);
        for (size_t i = 0; i < n; ++i) {
            uint64_t* r = &rows[i * FVAD_CLIP_SPLIT_FIELDS];
            r[0] = wild && pick(5) == 0 ? near_max() : pick(12) == 0 ? 0 : 1 + pick(3);
            r[1] = wild && pick(4) == 0 ? near_max() : pick(6);
            r[2] = wild && pick(4) == 0 ? near_max() : pick(250);
            r[3] = wild && pick(4) == 0 ? near_max() : pick(3) == 0 ? 0 : pick(120);
            r[4] = wild && pick(4) == 0 ? near_max() : pick(6);
            r[5] = wild && pick(4) == 0 ? near_max() : pick(250);
            r[6] = wild && pick(4) == 0 ? near_max() : pick(3) == 0 ? 0 : pick(120);
            if (tame && pick(10)) { r[0] = 1 + pick(3); r[1] = pick(4 - r[0]); r[4] = pick(4 - r[0]); r[2] = pick(180); r[5] = pick(180); }
        }
        const size_t cap = pick(2) == 0 ? (size_t)pick(200) : wild ? (size_t)near_max() : 100000;
        uint64_t total = 99;
        const int rc = fvad_clips_split_check((const void*)d_a, a_lanes, a_stride, a_samples, (const void*)d_b, b_lanes, b_stride, b_samples,
                                              src_format, n ? rows.data() : (pick(2) ? rows.data() : nullptr), n, out_format, (const void*)out, cap,
                                              device_out, pick(4) ? offsets.data() : nullptr, pick(4) ? &total : nullptr);
        ++tables;
        if (rc == FVAD_OK) { ++ok_tables; ++by_status[0]; }
        else if (rc == FVAD_ERR_INVALID_ARGUMENT) ++by_status[1];
        else if (rc == FVAD_ERR_OUT_OF_RANGE) ++by_status[2];
        else if (rc == FVAD_ERR_BUFFER_TOO_SMALL) ++by_status[3];
        else { fprintf(stderr, "an unexpected status %d\n", rc); return 6; }
        if (offsets[n] != 77) { fprintf(stderr, "offsets written past n_clips (round %d)\n", round); return 9; }
        if (rc != FVAD_OK || n == 0) continue;
        // what is accepted, restated with 128-bit arithmetic
        typedef unsigned __int128 u128;
        const u128 per16 = 16 / ob;
        u128 at = 0, units = 0;
        for (size_t i = 0; i < n; ++i) {
            const uint64_t* r = &rows[i * FVAD_CLIP_SPLIT_FIELDS];
            const u128 len = (u128)r[3] + r[6];
            bool good = r[0] >= 1 && len >= 1;
            if (r[3]) good = good && d_a && (u128)r[2] + r[3] <= a_samples && (u128)r[1] + r[0] <= a_lanes;
            if (r[6]) good = good && d_b && (u128)r[5] + r[6] <= b_samples && (u128)r[4] + r[0] <= b_lanes;
            if (!good) { fprintf(stderr, "an accepted row is out of range (round %d, row %zu)\n", round, i); return 7; }
            at += (len + per16 - 1) / per16 * per16;
            units += (len + 8191) / 8192 * r[0];
        }
        auto range_end = [](uintptr_t p, u128 lanes, u128 stride, u128 samples, u128 bytes) { return (u128)p + (lanes ? ((lanes - 1) * (lanes > 1 ? stride : 0) + samples) * bytes : 0); };
        const u128 a_end = range_end(d_a, d_a ? a_lanes : 0, a_stride, a_samples, sb), b_end = range_end(d_b, d_b ? b_lanes : 0, b_stride, b_samples, sb);
        const u128 o_end = (u128)out + at * ob;
        const bool hits_a = (u128)out < a_end && (u128)d_a < o_end && a_end > d_a, hits_b = (u128)out < b_end && (u128)d_b < o_end && b_end > d_b;
        if (!out || at > cap || at > UINT64_MAX || units > 0x7fffffffull || hits_a || hits_b || (device_out && out % 16) || d_a % sb || d_b % sb ||
            src_format < 0 || src_format > 1 || out_format < 0 || out_format > 1 || (a_lanes > 1 && a_stride < a_samples) || (b_lanes > 1 && b_stride < b_samples)) {
            fprintf(stderr, "an accepted call breaks a rule (round %d)\n", round);
            return 8;
        }
    }
    if (by_status[0] < 200 || by_status[1] < 200 || by_status[2] < 200 || by_status[3] < 20) {
        fprintf(stderr, "the driver is one-sided: ok %ld, invalid %ld, out of range %ld, too small %ld\n", by_status[0], by_status[1], by_status[2], by_status[3]);
        return 10;
    }
    printf("tables=%ld ok=%ld invalid=%ld range=%ld small=%ld\n", tables, ok_tables, by_status[1], by_status[2], by_status[3]);
    return 0;
}
