// clips_fir_san.cpp -- fvad_clips_fir_design and fvad_clips_fir_check (csrc/host_clips_fir.cpp, host only) under
// AddressSanitizer + UBSan: seeded steps, halves, cutoffs, betas and tap tables, with NaN, the infinities and values past every
// limit among them.  Whatever the design accepts must be 2 half + 1 finite taps that sum to 1 (within the f32 rounding of the
// taps, 2^-23 sum |h|), pass the check, and leave the floats behind them alone; whatever it refuses must break a stated rule or
// have no finite normalised form, and must write nothing.  The check is held against its own rules restated here.
// Built by tests/test_sanitizers_clips_fir.py; never loaded into Python.
//   usage: clips_fir_san <seed>
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
    if (argc < 2) { fprintf(stderr, "usage: clips_fir_san <seed>\n"); return 2; }
    std::mt19937_64 rng((uint64_t)atoll(argv[1]));
    auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    auto unit = [&]() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); };
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    long designs = 0, ok = 0, refused = 0, checks = 0, checks_ok = 0;
    for (int round = 0; round < 4000; ++round) {
        // ---- the design
        const uint32_t step = pick(12) == 0 ? (uint32_t)(pick(2) ? 0 : FVAD_CLIP_STEP_MAX + 1 + pick(1000)) : 1 + (uint32_t)pick(FVAD_CLIP_STEP_MAX);
        const uint32_t half = pick(12) == 0 ? 257 + (uint32_t)pick(100000) : pick(4) == 0 ? 0 : 1 + (uint32_t)pick(256);
        double cutoff, beta;
        switch (pick(10)) {
        case 0: cutoff = nan; break;
        case 1: cutoff = pick(2) ? inf : -inf; break;
        case 2: cutoff = -unit(); break;
        case 3: cutoff = 0.5 + unit() * 1e-3 + 1e-12; break;
        case 4: cutoff = 0; break;
        case 5: cutoff = 0.5; break;
        case 6: cutoff = std::ldexp(unit(), -(int)pick(1070)); break;
        default: cutoff = unit() * 0.5; break;
        }
        switch (pick(10)) {
        case 0: beta = nan; break;
        case 1: beta = pick(2) ? inf : -inf; break;
        case 2: beta = -unit() * 10; break;
        case 3: beta = 0; break;
        case 4: beta = unit() * 2000; break;
        case 5: beta = std::ldexp(unit(), (int)pick(1000)); break;
        default: beta = unit() * 20; break;
        }
        const bool null_taps = pick(40) == 0;
        const uint32_t eff_half = half ? half : 16 * step;
        std::vector<float> taps(2 * (size_t)(eff_half <= 256 ? eff_half : 0) + 1 + 4, 77.0f); // exactly the room the call may use, + 4
        const int rc = fvad_clips_fir_design(step, half, cutoff, beta, null_taps ? nullptr : taps.data());
        ++designs;
        if (rc != FVAD_OK && rc != FVAD_ERR_INVALID_ARGUMENT) { fprintf(stderr, "an unexpected status %d (round %d)\n", rc, round); return 3; }
        const bool rules = step >= 1 && step <= FVAD_CLIP_STEP_MAX && half <= 256 && cutoff >= 0 && cutoff <= 0.5 && std::isfinite(beta) && beta >= 0 && !null_taps;
        if (rc == FVAD_OK) {
            if (!rules) { fprintf(stderr, "a design that breaks a rule was accepted (round %d)\n", round); return 4; }
            const size_t n = 2 * (size_t)eff_half + 1;
            double sum = 0, mag = 0;
            for (size_t k = 0; k < n; ++k) {
                if (!std::isfinite(taps[k])) { fprintf(stderr, "a tap that is not finite (round %d, tap %zu)\n", round, k); return 5; }
                sum += (double)taps[k];
                mag += std::fabs((double)taps[k]);
            }
            if (!(std::fabs(sum - 1.0) <= std::ldexp(mag, -23) + 1e-12)) { fprintf(stderr, "the taps sum to %.17g (round %d)\n", sum, round); return 5; }
            for (size_t k = n; k < taps.size(); ++k)
                if (taps[k] != 77.0f) { fprintf(stderr, "written past the taps (round %d)\n", round); return 6; }
            if (fvad_clips_fir_check(taps.data(), (uint32_t)n) != FVAD_OK) { fprintf(stderr, "the check refuses a design (round %d)\n", round); return 7; }
            ++ok;
        } else {
            for (size_t k = 0; k < taps.size(); ++k)
                if (taps[k] != 77.0f) { fprintf(stderr, "a refused design wrote taps (round %d)\n", round); return 6; }
            // within the rules only a design without a finite normalised form may be refused: I0(beta) overflows above ~713,
            // and a cutoff so small that the taps underflow has no sum to divide by
            if (rules && beta < 700 && (cutoff == 0 || cutoff > 1e-290)) { fprintf(stderr, "a good design was refused (round %d: step %u half %u cutoff %g beta %g)\n", round, step, half, cutoff, beta); return 8; }
            ++refused;
        }
        // ---- the check
        const uint32_t n_taps = pick(8) == 0 ? (uint32_t)pick(3) * 514 + (uint32_t)pick(1200) : 1 + 2 * (uint32_t)pick(257) + (pick(9) == 0);
        std::vector<float> t(n_taps ? n_taps : 1); // exactly n_taps floats: a read past them is ASan's to find
        bool finite = true;
        for (auto& v : t) {
            const uint64_t r = pick(n_taps > 20 ? 400 : 12);
            v = r == 0 ? std::numeric_limits<float>::quiet_NaN() : r == 1 ? std::numeric_limits<float>::infinity() : r == 2 ? -std::numeric_limits<float>::infinity() : (float)(unit() * 2 - 1);
        }
        for (uint32_t k = 0; k < n_taps; ++k) finite = finite && std::isfinite(t[k]);
        const bool null_t = pick(30) == 0;
        const int cs = fvad_clips_fir_check(null_t ? nullptr : t.data(), n_taps);
        ++checks;
        const bool want = !null_t && n_taps >= 1 && n_taps % 2 == 1 && n_taps <= FVAD_CLIP_FIR_TAPS_MAX && finite;
        if (cs != (want ? FVAD_OK : FVAD_ERR_INVALID_ARGUMENT)) { fprintf(stderr, "the check gave %d for n_taps %u (round %d)\n", cs, n_taps, round); return 9; }
        checks_ok += want;
    }
    if (ok < 300 || refused < 300 || checks_ok < 300 || checks - checks_ok < 300) { fprintf(stderr, "the driver is one-sided: ok %ld, refused %ld, checks ok %ld of %ld\n", ok, refused, checks_ok, checks); return 10; }
    printf("designs=%ld ok=%ld refused=%ld checks=%ld checks_ok=%ld\n", designs, ok, refused, checks, checks_ok);
    return 0;
}
