// host_clips_fir.cpp -- fvad_clips_fir_design and fvad_clips_fir_check: the taps of a filtered clip export, without a device
// (plain C++: tests/sanitize/clips_fir_san.cpp builds this file alone).
#include "clips_fir.h"
#include "clips_strided.h"

using namespace fvad;

namespace {

// the modified Bessel function of the first kind, order 0, by its power series sum_k ((x / 2)^k / k!)^2: every term is
// positive, so there is no cancellation; overflows to inf for x above ~713
double bessel_i0(double x)
{
    const double q = x * x / 4;
    double term = 1, sum = 1;
    for (int k = 1; k < (1 << 16); ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (!(term > sum * 1e-20)) break; // (also ends on inf and NaN)
    }
    return sum;
}

const double kPi = 3.14159265358979323846;

} // namespace

extern "C" {

int fvad_clips_fir_design(uint32_t step, uint32_t half, double cutoff, double beta, float* taps)
{
    if (!strided_step_ok(step) || half > (FVAD_CLIP_FIR_TAPS_MAX - 1) / 2 || !taps) return FVAD_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(beta) || beta < 0 || !(cutoff >= 0 && cutoff <= 0.5)) return FVAD_ERR_INVALID_ARGUMENT;
    if (half == 0) half = 16 * step;
    if (cutoff == 0) cutoff = 0.45 / step;
    if (beta == 0) beta = 6.0;
    const uint32_t n = 2 * half + 1;
    double h[FVAD_CLIP_FIR_TAPS_MAX];
    const double i0b = bessel_i0(beta);
    double sum = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const double d = (double)k - (double)half, r = d / (double)half, a = kPi * 2 * cutoff * d;
        const double sinc = d == 0 ? 1.0 : std::sin(a) / a;
        const double w = bessel_i0(beta * std::sqrt(std::fmax(0.0, 1 - r * r))) / i0b;
        h[k] = 2 * cutoff * sinc * w;
        sum += h[k];
    }
    // a beta whose I0 overflows or a design whose taps sum to (nearly) nothing has no normalised form in f32: refused
    float out[FVAD_CLIP_FIR_TAPS_MAX];
    for (uint32_t k = 0; k < n; ++k) {
        const double v = h[k] / sum;
        if (!std::isfinite(v) || std::fabs(v) > 3.0e38) return FVAD_ERR_INVALID_ARGUMENT;
        out[k] = (float)v;
    }
    for (uint32_t k = 0; k < n; ++k) taps[k] = out[k];
    return FVAD_OK;
}

int fvad_clips_fir_check(const float* taps, uint32_t n_taps)
{
    const char* why;
    return fir_taps_ok(Fir{taps, n_taps}, &why) ? FVAD_OK : FVAD_ERR_INVALID_ARGUMENT;
}

} // extern "C"
