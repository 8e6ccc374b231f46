// clips_stride_san.cpp -- fvad_clips_phase_skips and fvad_clips_plan_strided (csrc/host_clips_strided.cpp, host only) under
// AddressSanitizer + UBSan: seeded random length / skip / step tables with values near UINT64_MAX for the overflow paths.
// Whatever is accepted must keep at least one sample per clip, give out_len = ceil((len - skip) / step), slots that start on
// 16-byte boundaries in clip order without overlapping, and a total that holds them all -- restated with 128-bit arithmetic.
// Built by tests/test_sanitizers_clips_stride.py; never loaded into Python.
//   usage: clips_stride_san <seed>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fvad.h"

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: clips_stride_san <seed>\n"); return 2; }
    std::mt19937_64 rng((uint64_t)atoll(argv[1]));
    auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    auto near_max = [&]() -> uint64_t {
        switch (pick(6)) {
        case 0: return UINT64_MAX - pick(40);
        case 1: return (UINT64_MAX >> pick(5)) + pick(3);
        case 2: return (1ull << 63) + pick(5) - 2;
        default: return pick(200);
        }
    };
    typedef unsigned __int128 u128;
    long tables = 0, ok = 0, refused = 0, huge_ok = 0;
    for (int round = 0; round < 6000; ++round) {
        const size_t n = (size_t)pick(9);
        const bool wild = pick(3) == 0;
        const uint32_t step = pick(15) == 0 ? (uint32_t)(pick(3) == 0 ? 0 : FVAD_CLIP_STEP_MAX + 1 + pick(4) * 1000000) : 1 + (uint32_t)pick(FVAD_CLIP_STEP_MAX);
        const int out_format = pick(25) == 0 ? (int)pick(5) - 1 : (int)pick(2);
        std::vector<uint64_t> lens(n + 1), out_lens(n + 1, 77), offsets(n + 1, 77), starts(n + 1);
        std::vector<uint32_t> skips(n + 1, 0xdeadbeef);
        const uint32_t phase = step ? (uint32_t)pick(step + (pick(20) == 0)) : 0;
        for (size_t i = 0; i < n; ++i) {
            lens[i] = wild && pick(3) == 0 ? near_max() : pick(40) == 0 ? pick(3) : 1 + pick(30000);
            starts[i] = wild && pick(2) ? near_max() : pick(1000000);
        }
        // the skips: the phase's, sometimes one broken
        const int rs = fvad_clips_phase_skips(n ? starts.data() : nullptr, n, step, phase, n ? skips.data() : nullptr);
        const bool step_ok = step >= 1 && step <= FVAD_CLIP_STEP_MAX;
        if ((rs == FVAD_OK) != (step_ok && phase < step)) { fprintf(stderr, "phase_skips: status %d for step %u phase %u\n", rs, step, phase); return 3; }
        if (skips[n] != 0xdeadbeef) { fprintf(stderr, "skips written past n_clips (round %d)\n", round); return 9; }
        if (rs == FVAD_OK)
            for (size_t i = 0; i < n; ++i)
                if (skips[i] >= step || (uint64_t)(((u128)starts[i] + skips[i]) % step) != phase) { fprintf(stderr, "a wrong skip (round %d)\n", round); return 4; }
        if (rs != FVAD_OK) for (size_t i = 0; i < n; ++i) skips[i] = step ? (uint32_t)pick(step) : 0;
        if (n && pick(12) == 0) skips[pick(n)] = step + (uint32_t)pick(3);
        const bool null_skips = pick(6) == 0;
        uint64_t total = 99;
        const int rc = fvad_clips_plan_strided(lens.data(), null_skips ? nullptr : skips.data(), n, step, out_format, out_lens.data(), offsets.data(), &total);
        ++tables;
        if (out_lens[n] != 77 || offsets[n] != 77) { fprintf(stderr, "written past n_clips (round %d)\n", round); return 9; }
        if (rc != FVAD_OK && rc != FVAD_ERR_INVALID_ARGUMENT) { fprintf(stderr, "an unexpected status %d\n", rc); return 6; }
        // what must be refused and what accepted, restated with 128-bit arithmetic
        const u128 per16 = out_format == FVAD_CLIP_PCM16 ? 8 : 4;
        bool good = step_ok && (out_format == FVAD_CLIP_F32 || out_format == FVAD_CLIP_PCM16);
        u128 at = 0;
        bool huge = false;
        for (size_t i = 0; good && i < n; ++i) {
            const uint64_t skip = null_skips ? 0 : skips[i];
            if (skip >= step || lens[i] <= skip) { good = false; break; }
            const u128 want = ((u128)lens[i] - skip + step - 1) / step;
            if (rc == FVAD_OK) {
                if (out_lens[i] != want || want == 0) { fprintf(stderr, "a wrong out_len (round %d, clip %zu)\n", round, i); return 7; }
                if (offsets[i] != at || offsets[i] % per16 != 0) { fprintf(stderr, "a slot that overlaps or is misaligned (round %d, clip %zu)\n", round, i); return 7; }
                if ((want - 1) * step + skip >= lens[i]) { fprintf(stderr, "the last kept sample lies past the clip (round %d, clip %zu)\n", round, i); return 7; }
            }
            at += (want + per16 - 1) / per16 * per16;
            huge = huge || lens[i] > (1ull << 62);
        }
        if (rc == FVAD_OK) {
            if (!good || at > UINT64_MAX || total != (uint64_t)at) { fprintf(stderr, "an accepted table breaks a rule (round %d)\n", round); return 8; }
            ++ok;
            huge_ok += huge;
        } else {
            // a refusal needs a reason: a broken rule, or a total within one slot's rounding of what 64 bits hold
            if (good && at + per16 <= (u128)UINT64_MAX) { fprintf(stderr, "a good table was refused (round %d)\n", round); return 8; }
            if (total != 99) { fprintf(stderr, "total written by a refused call (round %d)\n", round); return 8; }
            ++refused;
        }
    }
    if (ok < 500 || refused < 500 || huge_ok < 20) { fprintf(stderr, "the driver is one-sided: ok %ld, refused %ld, huge and ok %ld\n", ok, refused, huge_ok); return 10; }
    printf("tables=%ld ok=%ld refused=%ld huge_ok=%ld\n", tables, ok, refused, huge_ok);
    return 0;
}
