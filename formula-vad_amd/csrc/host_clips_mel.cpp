// host_clips_mel.cpp -- fvad_mel_design, fvad_clips_plan_mel and fvad_clips_mel_check: the Slaney mel matrix, how many frames a
// log-mel clip export writes and where, and every argument rule of the exports, without a device (plain C++:
// tests/sanitize/clips_mel_san.cpp builds this file alone).
#include <cmath>
#include <vector>

#include "clips_mel.h"

using namespace fvad;

namespace {

// Slaney's scale: linear at 3 f / 200 below 1 kHz, 15 + ln(f / 1000) / (ln 6.4 / 27) above it
constexpr double kMelBreakHz = 1000.0, kMelBreak = 15.0;
double mel_logstep() { return std::log(6.4) / 27.0; }
double hz_to_mel(double f) { return f < kMelBreakHz ? 3.0 * f / 200.0 : kMelBreak + std::log(f / kMelBreakHz) / mel_logstep(); }
double mel_to_hz(double m) { return m < kMelBreak ? 200.0 * m / 3.0 : kMelBreakHz * std::exp(mel_logstep() * (m - kMelBreak)); }

} // namespace

extern "C" {

int fvad_mel_design(double sample_rate, uint32_t n_fft, uint32_t n_mels, double fmin, double fmax, float* matrix)
{
    if (!matrix || !(sample_rate > 0.0) || !std::isfinite(sample_rate)) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_fft < 4 || n_fft > FVAD_CLIP_MEL_NFFT_MAX || n_fft % 2 != 0 || n_mels < 1 || n_mels > FVAD_CLIP_MEL_BANDS_MAX) return FVAD_ERR_INVALID_ARGUMENT;
    if (!(fmin >= 0.0) || !(fmax <= sample_rate / 2) || !(fmin < fmax)) return FVAD_ERR_INVALID_ARGUMENT;
    const uint32_t n_bins = n_fft / 2 + 1;
    std::vector<double> f(n_mels + 2);
    const double m_lo = hz_to_mel(fmin), m_hi = hz_to_mel(fmax);
    for (uint32_t i = 0; i < n_mels + 2; ++i) f[i] = mel_to_hz(m_lo + (m_hi - m_lo) * (double)i / (double)(n_mels + 1));
    for (uint32_t m = 0; m < n_mels; ++m) {
        const double scale = 2.0 / (f[m + 2] - f[m]);
        for (uint32_t k = 0; k < n_bins; ++k) {
            const double fk = (double)k * sample_rate / (double)n_fft;
            const double up = (fk - f[m]) / (f[m + 1] - f[m]), down = (f[m + 2] - fk) / (f[m + 2] - f[m + 1]);
            const double tri = std::fmax(0.0, std::fmin(up, down));
            matrix[(size_t)m * n_bins + k] = (float)(tri * scale);
        }
    }
    return FVAD_OK;
}

int fvad_clips_plan_mel(const uint64_t* lens, const uint32_t* skips, size_t n_clips, uint32_t step, uint32_t n_fft, uint32_t hop,
                        uint32_t n_mels, uint64_t* n_frames, uint64_t* offsets, uint64_t* total)
{
    if (!total || (n_clips && (!lens || !n_frames || !offsets))) return FVAD_ERR_INVALID_ARGUMENT;
    const Mel m{step, skips, n_fft, hop, n_mels};
    const char* why;
    if (!mel_frames_ok(m, &why)) return FVAD_ERR_INVALID_ARGUMENT;
    uint64_t at = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t slot = at;
        uint64_t L;
        if (!mel_slot(m, i, lens[i], &at, &L, &n_frames[i], &why)) return FVAD_ERR_INVALID_ARGUMENT;
        offsets[i] = slot;
    }
    *total = at;
    return FVAD_OK;
}

int fvad_clips_mel_check(const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                         const uint64_t* clips, size_t n_clips, int out_format, const void* out, size_t out_capacity, int device_out, uint32_t step,
                         const uint32_t* skips, uint32_t n_fft, uint32_t hop, const float* window, uint32_t n_mels,
                         const float* matrix, float floor, const float* norm, uint64_t* n_frames, uint64_t* offsets, uint64_t* total)
{
    const Mel m{step, skips, n_fft, hop, n_mels};
    return mel_check(d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, out, out_capacity, device_out, m, window,
                     matrix, floor, norm, n_frames, offsets, total, nullptr);
}

} // extern "C"
