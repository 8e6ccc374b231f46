// host_clips_features.cpp -- what the feature clip exports offer without a device: the two band designers (fvad_mel_design:
// Slaney's scale, area-normalised; fvad_mel_design_kaldi: HTK's scale as Kaldi's MelBanks has it), how many frames an export
// writes and where (fvad_clips_plan_mel, fvad_clips_plan_fbank: one loop), and every argument rule of the exports
// (fvad_clips_mel_check, fvad_clips_fbank_check: clips_features.h's feat_check; fvad_clips_split_mel_check,
// fvad_clips_split_fbank_check: its feat_split_check).  Plain C++: tests/sanitize/clips_mel_san.cpp, clips_fbank_san.cpp and
// clips_feat_split_san.cpp build this file alone.
#include <cmath>
#include <vector>

#include "clips_features.h"

using namespace fvad;

namespace {

// Slaney's scale: linear at 3 f / 200 below 1 kHz, 15 + ln(f / 1000) / (ln 6.4 / 27) above it
constexpr double kMelBreakHz = 1000.0, kMelBreak = 15.0;
double mel_logstep() { return std::log(6.4) / 27.0; }
double hz_to_mel(double f) { return f < kMelBreakHz ? 3.0 * f / 200.0 : kMelBreak + std::log(f / kMelBreakHz) / mel_logstep(); }
double mel_to_hz(double m) { return m < kMelBreak ? 200.0 * m / 3.0 : kMelBreakHz * std::exp(mel_logstep() * (m - kMelBreak)); }

// HTK's scale, as Kaldi's MelBanks::MelScale has it
double hz_to_mel_htk(double f) { return 1127.0 * std::log(1.0 + f / 700.0); }

// the frame counts and slots of a family's clips
int plan_features(const Feat& f, const uint64_t* lens, size_t n_clips, uint64_t* n_frames, uint64_t* offsets, uint64_t* total)
{
    if (!total || (n_clips && (!lens || !n_frames || !offsets))) return FVAD_ERR_INVALID_ARGUMENT;
    const char* why;
    if (!feat_frames_ok(f, &why)) return FVAD_ERR_INVALID_ARGUMENT;
    uint64_t at = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t slot = at;
        if (!feat_slot(f, i, lens[i], &at, &n_frames[i], &why)) return FVAD_ERR_INVALID_ARGUMENT;
        offsets[i] = slot;
    }
    *total = at;
    return FVAD_OK;
}

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

int fvad_mel_design_kaldi(double sample_rate, uint32_t n_fft, uint32_t n_mels, double low_freq, double high_freq, float* matrix)
{
    if (!matrix || !(sample_rate > 0.0) || !std::isfinite(sample_rate)) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_fft < 4 || n_fft > FVAD_CLIP_MEL_NFFT_MAX || n_fft % 2 != 0 || n_mels < 1 || n_mels > FVAD_CLIP_MEL_BANDS_MAX) return FVAD_ERR_INVALID_ARGUMENT;
    const double nyquist = sample_rate / 2, high = high_freq <= 0.0 ? nyquist + high_freq : high_freq; // (NaN stays NaN: refused below)
    if (!(low_freq >= 0.0) || !(high <= nyquist) || !(low_freq < high)) return FVAD_ERR_INVALID_ARGUMENT;
    const uint32_t n_bins = n_fft / 2 + 1;
    std::vector<double> p(n_mels + 2);
    const double m_lo = hz_to_mel_htk(low_freq), m_hi = hz_to_mel_htk(high);
    for (uint32_t i = 0; i < n_mels + 2; ++i) p[i] = m_lo + (m_hi - m_lo) * (double)i / (double)(n_mels + 1);
    for (uint32_t m = 0; m < n_mels; ++m) {
        const double l = p[m], c = p[m + 1], r = p[m + 2];
        for (uint32_t k = 0; k + 1 < n_bins; ++k) {
            const double mk = hz_to_mel_htk((double)k * sample_rate / (double)n_fft);
            matrix[(size_t)m * n_bins + k] = (float)std::fmax(0.0, std::fmin((mk - l) / (c - l), (r - mk) / (r - c)));
        }
        matrix[(size_t)m * n_bins + n_bins - 1] = 0.0f; // Kaldi's banks span n_fft / 2 bins: the Nyquist bin takes no part
    }
    return FVAD_OK;
}

int fvad_clips_plan_mel(const uint64_t* lens, const uint32_t* skips, size_t n_clips, uint32_t step, uint32_t n_fft, uint32_t hop,
                        uint32_t n_mels, uint64_t* n_frames, uint64_t* offsets, uint64_t* total)
{
    return plan_features(Feat{step, skips, n_fft, n_fft, hop, n_mels, false}, lens, n_clips, n_frames, offsets, total);
}

// (the plan does not know n_fft: win_length is held to the largest one)
int fvad_clips_plan_fbank(const uint64_t* lens, const uint32_t* skips, size_t n_clips, uint32_t step, uint32_t win_length, uint32_t hop,
                          uint32_t n_mels, uint64_t* n_frames, uint64_t* offsets, uint64_t* total)
{
    return plan_features(Feat{step, skips, win_length, FVAD_CLIP_MEL_NFFT_MAX, hop, n_mels, true}, lens, n_clips, n_frames, offsets, total);
}

int fvad_clips_mel_check(const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                         const uint64_t* clips, size_t n_clips, int out_format, const void* out, size_t out_capacity, int device_out, uint32_t step,
                         const uint32_t* skips, uint32_t n_fft, uint32_t hop, const float* window, uint32_t n_mels,
                         const float* matrix, float floor, const float* norm, uint64_t* n_frames, uint64_t* offsets, uint64_t* total)
{
    return feat_check(d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, out, out_capacity, device_out,
                      Feat{step, skips, n_fft, n_fft, hop, n_mels, false}, window, matrix, FeatCond{floor, norm, 0.0f, 0.0f, 0, 0}, n_frames, offsets, total, nullptr);
}

int fvad_clips_fbank_check(const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples, const uint64_t* clips,
                           size_t n_clips, int out_format, const void* out, size_t out_capacity, int device_out, uint32_t step,
                           const uint32_t* skips, uint32_t win_length, uint32_t n_fft, uint32_t hop, const float* window, uint32_t n_mels,
                           const float* matrix, float scale, float preemph, int remove_dc, float floor, int cmn, uint64_t* n_frames,
                           uint64_t* offsets, uint64_t* total)
{
    return feat_check(d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, out, out_capacity, device_out,
                      Feat{step, skips, win_length, n_fft, hop, n_mels, true}, window, matrix, FeatCond{floor, nullptr, scale, preemph, remove_dc, cmn}, n_frames, offsets, total, nullptr);
}

int fvad_clips_split_mel_check(const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b, size_t b_lanes,
                               size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips, int out_format,
                               const void* out, size_t out_capacity, int device_out, uint32_t step, const uint32_t* skips, uint32_t n_fft,
                               uint32_t hop, const float* window, uint32_t n_mels, const float* matrix, float floor, const float* norm,
                               uint64_t* n_frames, uint64_t* offsets, uint64_t* total)
{
    return feat_split_check(d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips, out_format, out, out_capacity,
                            device_out, Feat{step, skips, n_fft, n_fft, hop, n_mels, false}, window, matrix, FeatCond{floor, norm, 0.0f, 0.0f, 0, 0}, n_frames, offsets, total, nullptr);
}

int fvad_clips_split_fbank_check(const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b, size_t b_lanes,
                                 size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips, int out_format,
                                 const void* out, size_t out_capacity, int device_out, uint32_t step, const uint32_t* skips,
                                 uint32_t win_length, uint32_t n_fft, uint32_t hop, const float* window, uint32_t n_mels, const float* matrix,
                                 float scale, float preemph, int remove_dc, float floor, int cmn, uint64_t* n_frames, uint64_t* offsets,
                                 uint64_t* total)
{
    return feat_split_check(d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips, out_format, out, out_capacity,
                            device_out, Feat{step, skips, win_length, n_fft, hop, n_mels, true}, window, matrix, FeatCond{floor, nullptr, scale, preemph, remove_dc, cmn}, n_frames, offsets, total, nullptr);
}

} // extern "C"
