// clips_mel_san.cpp -- fvad_clips_plan_mel, fvad_clips_mel_check and fvad_mel_design (csrc/host_clips_features.cpp, host only) under
// AddressSanitizer + UBSan: seeded random length / skip / frame-parameter tables with values near UINT64_MAX for the overflow
// paths.  Whatever the plan accepts must give L = ceil((len - skip) / step) >= n_fft / 2 + 1, T = floor(L / hop) >= 1 frames,
// slots of T * n_mels floats that start on 16-byte boundaries in clip order without overlapping, and a total that holds them all
// -- restated with 128-bit arithmetic; the check must agree with the plan wherever its other rules hold; the designer must write
// exactly n_mels * (n_fft / 2 + 1) finite non-negative values or nothing.
// Built by tests/test_sanitizers_clips_mel.py; never loaded into Python.
//   usage: clips_mel_san <seed>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fvad.h"

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: clips_mel_san <seed>\n"); return 2; }
    std::mt19937_64 rng((uint64_t)atoll(argv[1]));
    auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    auto near_max = [&]() -> uint64_t {
        switch (pick(6)) {
        case 0: return UINT64_MAX - pick(40);
        case 1: return (UINT64_MAX >> pick(9)) + pick(3);
        case 2: return (1ull << 63) + pick(5) - 2;
        default: return pick(200);
        }
    };
    typedef unsigned __int128 u128;
    long tables = 0, ok = 0, refused = 0, huge_ok = 0, designs = 0;
    for (int round = 0; round < 4000; ++round) {
        const size_t n = (size_t)pick(9);
        const bool wild = pick(3) == 0;
        const uint32_t step = pick(15) == 0 ? (uint32_t)(pick(3) == 0 ? 0 : FVAD_CLIP_STEP_MAX + 1 + pick(4) * 1000000) : 1 + (uint32_t)pick(FVAD_CLIP_STEP_MAX);
        uint32_t n_fft = pick(12) == 0 ? (uint32_t)pick(5000) : 2 * (2 + (uint32_t)pick(pick(2) ? 8 : FVAD_CLIP_MEL_NFFT_MAX / 2 - 1));
        const uint32_t hop = pick(15) == 0 ? (uint32_t)pick(3) * (n_fft + 1) / 2 : 1 + (uint32_t)pick(n_fft ? n_fft : 1);
        const uint32_t n_mels = pick(15) == 0 ? (uint32_t)pick(3) * 129 / 2 : 1 + (uint32_t)pick(FVAD_CLIP_MEL_BANDS_MAX);
        std::vector<uint64_t> lens(n + 1), frames(n + 1, 77), offsets(n + 1, 77);
        std::vector<uint32_t> skips(n + 1, 0);
        for (size_t i = 0; i < n; ++i) {
            lens[i] = wild && pick(3) == 0 ? near_max() : pick(40) == 0 ? pick(3) : 1 + pick(30) * (uint64_t)(n_fft + 1) * (step ? step : 1) / 4;
            skips[i] = step ? (uint32_t)pick(step) : 0;
        }
        if (n && pick(12) == 0) skips[pick(n)] = step + (uint32_t)pick(3);
        const bool null_skips = pick(6) == 0;
        uint64_t total = 99;
        const int rc = fvad_clips_plan_mel(lens.data(), null_skips ? nullptr : skips.data(), n, step, n_fft, hop, n_mels, frames.data(), offsets.data(), &total);
        ++tables;
        if (frames[n] != 77 || offsets[n] != 77) { fprintf(stderr, "written past n_clips (round %d)\n", round); return 9; }
        if (rc != FVAD_OK && rc != FVAD_ERR_INVALID_ARGUMENT) { fprintf(stderr, "an unexpected status %d\n", rc); return 6; }
        bool good = step >= 1 && step <= FVAD_CLIP_STEP_MAX && n_fft >= 4 && n_fft <= FVAD_CLIP_MEL_NFFT_MAX && n_fft % 2 == 0 && hop >= 1 &&
                    hop <= n_fft && n_mels >= 1 && n_mels <= FVAD_CLIP_MEL_BANDS_MAX;
        u128 at = 0;
        bool huge = false;
        for (size_t i = 0; good && i < n; ++i) {
            const uint64_t skip = null_skips ? 0 : skips[i];
            if (skip >= step || lens[i] <= skip) { good = false; break; }
            const u128 L = ((u128)lens[i] - skip + step - 1) / step, T = L / hop;
            if (L < n_fft / 2 + 1 || T == 0) { good = false; break; }
            if (rc == FVAD_OK) {
                if (frames[i] != T) { fprintf(stderr, "a wrong frame count (round %d, clip %zu)\n", round, i); return 7; }
                if (offsets[i] != at || offsets[i] % 4 != 0) { fprintf(stderr, "a slot that overlaps or is misaligned (round %d, clip %zu)\n", round, i); return 7; }
            }
            at += (T * n_mels + 3) / 4 * 4;
            huge = huge || lens[i] > (1ull << 56);
        }
        if (rc == FVAD_OK) {
            if (!good || at > UINT64_MAX || total != (uint64_t)at) { fprintf(stderr, "an accepted table breaks a rule (round %d)\n", round); return 8; }
            ++ok;
            huge_ok += huge;
        } else {
            if (good && at + 4 <= (u128)UINT64_MAX) { fprintf(stderr, "a good table was refused (round %d)\n", round); return 8; }
            if (total != 99) { fprintf(stderr, "total written by a refused call (round %d)\n", round); return 8; }
            ++refused;
        }
        // the check on rows of one lane that holds every clip from sample 0: it accepts what the plan accepts (its own further
        // rules hold by construction, or it says out of range / too many tiles) and gives the plan's numbers
        if (n && n_fft >= 4 && n_fft <= FVAD_CLIP_MEL_NFFT_MAX && n_fft % 2 == 0 && n_mels >= 1 && n_mels <= FVAD_CLIP_MEL_BANDS_MAX) {
            std::vector<uint64_t> rows(n * FVAD_CLIP_FIELDS), f2(n + 1, 55), o2(n + 1, 55);
            bool rows_ok = true;
            for (size_t i = 0; i < n; ++i) { rows[4 * i] = 0; rows[4 * i + 1] = 1; rows[4 * i + 2] = 0; rows[4 * i + 3] = lens[i]; rows_ok = rows_ok && lens[i] > 0; }
            std::vector<float> window(n_fft, 0.5f), matrix((size_t)n_mels * (n_fft / 2 + 1), 0.25f);
            const float norm[3] = {8.0f, 4.0f, 0.25f};
            if (pick(30) == 0) window[pick(n_fft)] = NAN;
            uint64_t t2 = 55;
            const int rk = fvad_clips_mel_check((const void*)0x1000, FVAD_CLIP_F32, 1, 0, UINT64_MAX, rows.data(), n, FVAD_CLIP_F32, (const void*)0x2000,
                                                UINT64_MAX, 1, step, null_skips ? nullptr : skips.data(), n_fft, hop, window.data(), n_mels, matrix.data(),
                                                1e-10f, pick(2) ? norm : nullptr, f2.data(), o2.data(), &t2);
            if (f2[n] != 55 || o2[n] != 55) { fprintf(stderr, "the check wrote past n_clips (round %d)\n", round); return 9; }
            if (rk == FVAD_OK) {
                if (rc != FVAD_OK || !rows_ok || t2 != total) { fprintf(stderr, "the check accepts what the plan refuses (round %d)\n", round); return 11; }
                for (size_t i = 0; i < n; ++i) if (f2[i] != frames[i] || o2[i] != offsets[i]) { fprintf(stderr, "the check's numbers are not the plan's (round %d)\n", round); return 11; }
            } else if (rk != FVAD_ERR_INVALID_ARGUMENT) { fprintf(stderr, "the check: an unexpected status %d (round %d)\n", rk, round); return 11; }
        }
        // the designer
        if (round % 8 == 0) {
            const uint32_t nb = n_fft / 2 + 1;
            std::vector<float> m((size_t)(n_mels ? n_mels : 1) * nb + 1, -7.0f);
            const double sr = pick(10) == 0 ? -1.0 : 8000.0 + (double)pick(40000), fmin = pick(8) == 0 ? -1.0 : (double)pick(300), fmax = pick(8) == 0 ? sr : sr / 2 - (double)pick(100);
            const int rd = fvad_mel_design(sr, n_fft, n_mels, fmin, fmax, m.data());
            ++designs;
            const bool dgood = sr > 0 && n_fft >= 4 && n_fft <= FVAD_CLIP_MEL_NFFT_MAX && n_fft % 2 == 0 && n_mels >= 1 && n_mels <= FVAD_CLIP_MEL_BANDS_MAX && fmin >= 0 && fmax <= sr / 2 && fmin < fmax;
            if ((rd == FVAD_OK) != dgood) { fprintf(stderr, "the designer: status %d (round %d)\n", rd, round); return 12; }
            if (m[(size_t)(n_mels ? n_mels : 1) * nb] != -7.0f) { fprintf(stderr, "the designer wrote past its matrix (round %d)\n", round); return 12; }
            if (rd == FVAD_OK) { for (size_t i = 0; i < (size_t)n_mels * nb; ++i) if (!std::isfinite(m[i]) || m[i] < 0.0f) { fprintf(stderr, "a matrix value that is not finite and >= 0 (round %d)\n", round); return 12; } }
            else if (m[0] != -7.0f) { fprintf(stderr, "a refused design wrote (round %d)\n", round); return 12; }
        }
    }
    if (ok < 300 || refused < 300 || huge_ok < 5) { fprintf(stderr, "the driver is one-sided: ok %ld, refused %ld, huge and ok %ld\n", ok, refused, huge_ok); return 10; }
    printf("tables=%ld ok=%ld refused=%ld huge_ok=%ld designs=%ld\n", tables, ok, refused, huge_ok, designs);
    return 0;
}
