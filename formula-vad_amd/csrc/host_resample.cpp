// host_resample.cpp -- the host-only half of the resampling ingest (fvad_ingest_resample*, engine_ingest.cpp): the ratio, the
// output count, the window, the polyphase prototype's design and fvad_ingest_resample_check, every argument rule of the device
// calls.  Plain C++ without HIP headers (tests/sanitize/resample_san.cpp builds this file alone).
#include <algorithm>

#include "ingest_rules.h"
#include "resample.h"

using namespace fvad;

namespace {

// the modified Bessel function of the first kind, order 0, by its power series (fvad_clips_fir_design's)
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

int fvad_resample_ratio(uint32_t rate_in, uint32_t rate_out, uint32_t* up, uint32_t* down)
{
    if (!up || !down || rate_in == 0 || rate_out == 0) return FVAD_ERR_INVALID_ARGUMENT;
    uint32_t a = rate_in, b = rate_out;
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    if (rate_out / a > FVAD_RESAMPLE_UP_MAX) return FVAD_ERR_INVALID_ARGUMENT;
    *up = rate_out / a;
    *down = rate_in / a;
    return FVAD_OK;
}

uint64_t fvad_resample_out_frames(uint64_t file_frames, uint32_t up, uint32_t down)
{
    if (!ratio_ok(Ratio{up, down})) return 0;
    return resample_out_frames(file_frames, Ratio{up, down});
}

int fvad_resample_design(uint32_t up, uint32_t down, uint32_t half, double cutoff, double beta, float* taps, uint32_t* n_taps)
{
    if (!ratio_ok(Ratio{up, down}) || !taps || !n_taps) return FVAD_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(beta) || beta < 0 || !(cutoff >= 0 && cutoff <= 0.5)) return FVAD_ERR_INVALID_ARGUMENT;
    const uint32_t m = std::max(up, down);
    if (half == 0) half = 16;
    if ((uint64_t)half * m > (FVAD_RESAMPLE_TAPS_MAX - 1) / 2) return FVAD_ERR_INVALID_ARGUMENT;
    if (cutoff == 0) cutoff = 0.45 / m;
    if (beta == 0) beta = 6.0;
    const uint32_t K = half * m, n = 2 * K + 1;
    std::vector<double> h(n);
    const double i0b = bessel_i0(beta);
    double sum = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const double d = (double)k - (double)K, r = d / (double)K, a = kPi * 2 * cutoff * d;
        const double sinc = d == 0 ? 1.0 : std::sin(a) / a;
        const double w = bessel_i0(beta * std::sqrt(std::fmax(0.0, 1 - r * r))) / i0b;
        h[k] = 2 * cutoff * sinc * w;
        sum += h[k];
    }
    // a beta whose I0 overflows or a design whose taps sum to (nearly) nothing has no normalised form in f32: refused
    for (uint32_t k = 0; k < n; ++k) {
        h[k] = h[k] * (double)up / sum;
        if (!std::isfinite(h[k]) || std::fabs(h[k]) > 3.0e38) return FVAD_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t k = 0; k < n; ++k) taps[k] = (float)h[k];
    *n_taps = n;
    return FVAD_OK;
}

int fvad_resample_window(uint32_t up, uint32_t down, uint32_t n_taps, uint64_t file_frames, uint64_t out_from, uint64_t n_out,
                         uint64_t* frame_lo, uint64_t* frame_hi)
{
    if (!ratio_ok(Ratio{up, down}) || !frame_lo || !frame_hi || n_taps == 0 || n_taps % 2 == 0 || n_taps > FVAD_RESAMPLE_TAPS_MAX)
        return FVAD_ERR_INVALID_ARGUMENT;
    if (n_out > UINT64_MAX - out_from) return FVAD_ERR_INVALID_ARGUMENT;
    resample_window(Ratio{up, down}, n_taps, file_frames, out_from, n_out, frame_lo, frame_hi);
    return FVAD_OK;
}

uint64_t fvad_ingest_resample_tile(uint32_t up, uint32_t down, uint32_t n_taps, uint32_t n_channels, uint32_t format)
{
    if (!ratio_ok(Ratio{up, down}) || n_taps == 0 || n_taps % 2 == 0 || n_taps > FVAD_RESAMPLE_TAPS_MAX) return 0;
    if (n_channels < 1 || n_channels > 64 || format > FVAD_INGEST_PCM24) return 0;
    return resample_tile(Ratio{up, down}, n_taps, n_channels, format);
}

// The order: arguments (lane format, ratio, taps, sources, lane_stride); then every source's own rules (format, channels, the
// file's length, the outputs against the file, fill_to, the given frames against the file and against the window, the tile);
// then every source's ranges (lanes, fill_to against n_samples, bytes against raw_bytes); then the overlap of two sources'
// destinations (both ingest_rules.h's, shared with fvad_ingest_check).
int fvad_ingest_resample_check(const uint64_t* sources, size_t n_sources, uint64_t raw_bytes, uint32_t up, uint32_t down,
                               const float* taps, uint32_t n_taps, int out_format, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    if (out_format != FVAD_INGEST_F32) return FVAD_ERR_INVALID_ARGUMENT; // PCM16 lanes would be a conversion; anything else is no format
    const Ratio q{up, down};
    if (!ratio_ok(q)) return FVAD_ERR_INVALID_ARGUMENT;
    const char* why;
    if (!resample_taps_ok(Taps{taps, n_taps}, &why)) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sources == 0) return FVAD_OK;
    if (!sources) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_lanes > 1 && lane_stride < n_samples) return FVAD_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n_sources; ++i) {
        const uint64_t* r = sources + i * FVAD_RESAMPLE_FIELDS;
        const uint64_t n_frames = r[1], n_channels = r[2], format = r[3], dst_offset = r[5], fill_to = r[6];
        const uint64_t frame_base = r[7], file_frames = r[8], out_from = r[9], n_out = r[10];
        if (format != FVAD_INGEST_F32 && format != FVAD_INGEST_PCM16 && format != FVAD_INGEST_PCM24) return FVAD_ERR_INVALID_ARGUMENT;
        if (n_channels < 1 || n_channels > 64) return FVAD_ERR_INVALID_ARGUMENT;
        if ((u128)file_frames * up >= (u128)kResampleFramesUp) return FVAD_ERR_INVALID_ARGUMENT;
        if (n_out > UINT64_MAX - out_from || out_from + n_out > resample_out_frames(file_frames, q)) return FVAD_ERR_INVALID_ARGUMENT;
        if (n_out > UINT64_MAX - dst_offset || fill_to < dst_offset + n_out) return FVAD_ERR_INVALID_ARGUMENT;
        if (n_frames > UINT64_MAX - frame_base || frame_base + n_frames > file_frames) return FVAD_ERR_INVALID_ARGUMENT;
        uint64_t lo, hi;
        resample_window(q, n_taps, file_frames, out_from, n_out, &lo, &hi);
        if (hi > lo && (frame_base > lo || frame_base + n_frames < hi)) return FVAD_ERR_INVALID_ARGUMENT; // the slice would not be the file
        if (resample_tile(q, n_taps, n_channels, format) == 0) return FVAD_ERR_INVALID_ARGUMENT;         // taps too long for frames this wide
    }
    const int rc = ingest_ranges_check(sources, n_sources, FVAD_RESAMPLE_FIELDS, raw_bytes, n_lanes, n_samples);
    if (rc != FVAD_OK) return rc;
    if (!ingest_rows_disjoint(sources, n_sources, FVAD_RESAMPLE_FIELDS)) return FVAD_ERR_INVALID_ARGUMENT;
    return FVAD_OK;
}

} // extern "C"
