// clips_resample_san.cpp -- fvad_clips_resample_check, fvad_clips_resample_tile and fvad_clips_plan_resampled
// (csrc/host_clips_resample.cpp with csrc/host_resample.cpp, host only) under AddressSanitizer + UBSan: seeded ratios, tap counts
// and tap tables with NaN and the infinities among them, and clip lengths that are random, tiny or near UINT64_MAX.  The check
// and the tile are held against their rules restated here (the tile by a search of its own in 128 bits); whatever the plan
// accepts must be ceil(len * up / down) per clip, in 128 bits, in 16-byte aligned slots one behind the other; whatever it
// refuses must break a stated rule.  Built by tests/test_sanitizers_clips_resample.py; never loaded into Python.
//   usage: clips_resample_san <seed>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "fvad.h"

typedef unsigned __int128 u128;

// the most outputs, in eights, at most 8192, whose window floor(((n - 1) down + n_taps - 1) / up) + 1 fits 8192 samples
static uint64_t tile_by_search(uint32_t up, uint32_t down, uint32_t n_taps)
{
    for (uint64_t n = 8192; n >= 8; n -= 8)
        if (((u128)(n - 1) * down + (n_taps - 1)) / up + 1 <= 8192) return n;
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: clips_resample_san <seed>\n"); return 2; }
    std::mt19937_64 rng((uint64_t)atoll(argv[1]));
    auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    auto unit = [&]() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); };
    long rounds = 0, checks_ok = 0, checks_bad = 0, tiles = 0, tiles_zero = 0, plans_ok = 0, plans_bad = 0;
    for (int round = 0; round < 4000; ++round, ++rounds) {
        // ---- a ratio and a tap count, inside and outside every limit
        const uint32_t up = pick(10) == 0 ? (uint32_t)(pick(2) ? 0 : FVAD_RESAMPLE_UP_MAX + 1 + pick(1u << 20)) : 1 + (uint32_t)pick(FVAD_RESAMPLE_UP_MAX);
        const uint32_t down = pick(12) == 0 ? 0 : pick(6) == 0 ? (uint32_t)rng() : 1 + (uint32_t)pick(2000);
        const uint32_t n_taps = pick(10) == 0 ? FVAD_RESAMPLE_TAPS_MAX + 1 + (uint32_t)pick(100000) : pick(12) == 0 ? 0 : 1 + 2 * (uint32_t)pick(pick(3) ? 600 : 10241) + (pick(9) == 0);
        const bool ratio = up >= 1 && up <= FVAD_RESAMPLE_UP_MAX && down >= 1;
        const bool count = n_taps >= 1 && n_taps % 2 == 1 && n_taps <= FVAD_RESAMPLE_TAPS_MAX;
        // ---- the tile
        const uint64_t tile = fvad_clips_resample_tile(up, down, n_taps);
        const uint64_t tile_want = ratio && count ? tile_by_search(up, down, n_taps) : 0;
        if (tile != tile_want) { fprintf(stderr, "tile %llu, want %llu (round %d: %u/%u, %u taps)\n", (unsigned long long)tile, (unsigned long long)tile_want, round, up, down, n_taps); return 3; }
        ++tiles;
        tiles_zero += tile == 0;
        // ---- the check
        std::vector<float> t(n_taps ? n_taps : 1); // exactly n_taps floats: a read past them is ASan's to find
        bool finite = true;
        for (auto& v : t) {
            const uint64_t r = pick(n_taps > 20 ? 8000 : 12);
            v = r == 0 ? std::numeric_limits<float>::quiet_NaN() : r == 1 ? std::numeric_limits<float>::infinity() : r == 2 ? -std::numeric_limits<float>::infinity() : (float)(unit() * 2 - 1);
        }
        for (uint32_t k = 0; k < n_taps; ++k) finite = finite && std::isfinite(t[k]);
        const bool null_t = pick(30) == 0;
        const int cs = fvad_clips_resample_check(up, down, null_t ? nullptr : t.data(), n_taps);
        const bool want = ratio && !null_t && count && finite && tile_want > 0;
        if (cs != (want ? FVAD_OK : FVAD_ERR_INVALID_ARGUMENT)) { fprintf(stderr, "the check gave %d (round %d: %u/%u, %u taps)\n", cs, round, up, down, n_taps); return 4; }
        (want ? checks_ok : checks_bad) += 1;
        // ---- the plan
        const size_t n_clips = pick(8) == 0 ? 0 : 1 + (size_t)pick(12);
        const int fmt = pick(15) == 0 ? 2 + (int)pick(5) : (int)pick(2);
        std::vector<uint64_t> lens(n_clips ? n_clips : 1), out_lens(n_clips + 2, 77), offsets(n_clips + 2, 77);
        bool zero = false;
        for (size_t i = 0; i < n_clips; ++i) {
            switch (pick(8)) {
            case 0: lens[i] = UINT64_MAX - pick(1000); break;
            case 1: lens[i] = UINT64_MAX / (up ? up : 1) - 500 + pick(1000); break;
            case 2: lens[i] = pick(40) == 0 ? 0 : 1 + pick(16); break;
            case 3: lens[i] = rng() >> pick(64); break;
            default: lens[i] = 1 + pick(1u << 26); break;
            }
            zero = zero || lens[i] == 0;
        }
        uint64_t total = 77;
        const bool null_total = pick(40) == 0, null_lens = n_clips && pick(40) == 0;
        const int ps = fvad_clips_plan_resampled(null_lens ? nullptr : lens.data(), n_clips, up, down, fmt, out_lens.data(), offsets.data(), null_total ? nullptr : &total);
        if (ps != FVAD_OK && ps != FVAD_ERR_INVALID_ARGUMENT) { fprintf(stderr, "the plan gave %d (round %d)\n", ps, round); return 5; }
        // the plan restated in 128 bits
        bool fits = true;
        u128 at = 0;
        const uint64_t per16 = fmt == FVAD_CLIP_PCM16 ? 8 : 4;
        std::vector<u128> want_len(n_clips), want_off(n_clips);
        if (ratio)
            for (size_t i = 0; i < n_clips; ++i) {
                want_len[i] = ((u128)lens[i] * up + down - 1) / down;
                want_off[i] = at;
                if (at + want_len[i] + per16 > (u128)UINT64_MAX) fits = false; // (the slot and its rounding fit 64 bits)
                at += (want_len[i] + per16 - 1) / per16 * per16;
            }
        const bool rules = (fmt == FVAD_CLIP_F32 || fmt == FVAD_CLIP_PCM16) && !null_total && !null_lens && ratio && !zero;
        if (ps == FVAD_OK) {
            if (!rules) { fprintf(stderr, "a plan that breaks a rule was accepted (round %d)\n", round); return 6; }
            if ((u128)total != at) { fprintf(stderr, "the total is wrong (round %d)\n", round); return 7; }
            for (size_t i = 0; i < n_clips; ++i)
                if ((u128)out_lens[i] != want_len[i] || (u128)offsets[i] != want_off[i] || offsets[i] % per16 != 0) { fprintf(stderr, "clip %zu is planned wrong (round %d)\n", i, round); return 7; }
            ++plans_ok;
        } else {
            if (rules && fits) { fprintf(stderr, "a good plan was refused (round %d: %u/%u, %zu clips)\n", round, up, down, n_clips); return 8; }
            if (total != 77) { fprintf(stderr, "a refused plan wrote the total (round %d)\n", round); return 8; }
            ++plans_bad;
        }
        for (size_t i = n_clips; i < n_clips + 2; ++i)
            if (out_lens[i] != 77 || offsets[i] != 77) { fprintf(stderr, "written past the clips (round %d)\n", round); return 9; }
        // fvad_resample_out_frames beside the plan: the same count, saturated
        if (ratio && n_clips) {
            const uint64_t got = fvad_resample_out_frames(lens[0], up, down);
            const u128 w = ((u128)lens[0] * up + down - 1) / down;
            if (got != (w > (u128)UINT64_MAX ? UINT64_MAX : (uint64_t)w)) { fprintf(stderr, "out_frames is wrong (round %d)\n", round); return 10; }
        }
    }
    if (checks_ok < 300 || checks_bad < 300 || plans_ok < 300 || plans_bad < 300 || tiles_zero < 100 || tiles - tiles_zero < 300) {
        fprintf(stderr, "the driver is one-sided: checks %ld/%ld, plans %ld/%ld, tiles %ld of %ld zero\n", checks_ok, checks_bad, plans_ok, plans_bad, tiles_zero, tiles);
        return 11;
    }
    printf("rounds=%ld checks_ok=%ld checks_bad=%ld plans_ok=%ld plans_bad=%ld tiles_zero=%ld\n", rounds, checks_ok, checks_bad, plans_ok, plans_bad, tiles_zero);
    return 0;
}
