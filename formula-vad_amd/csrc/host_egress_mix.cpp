// host_egress_mix.cpp -- the host-only half of the two-source egress (fvad_egress_mix*, engine_egress_mix.cpp):
// fvad_nsnet2_delay, the lag of the denoised lanes behind the original ones, and fvad_egress_mix_check, every argument rule of
// the device calls.  Plain C++ without HIP headers, like host_egress.cpp, so that it can be tested (and run under sanitizers)
// on a machine without a device.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/fvad.h"

namespace {
uint64_t sample_bytes(uint64_t format) { return format == FVAD_INGEST_PCM16 ? 2 : format == FVAD_INGEST_PCM24 ? 3 : 4; }
struct Range { uint64_t from, to; };
} // namespace

extern "C" {

// One hop of the network's rate in front of the input (160 samples of 16 kHz, r each) and the up-sampler's r - 1 interpolated
// samples in front of every network sample: 160 r + (r - 1).
int fvad_nsnet2_delay(size_t in_sample_rate, uint64_t* delay)
{
    if (delay) *delay = 0;
    if (!delay) return FVAD_ERR_INVALID_ARGUMENT;
    if (in_sample_rate == 0 || in_sample_rate % 16000 != 0) return FVAD_ERR_INVALID_SAMPLE_RATE; // fvad_nsnet2_create's refusal
    *delay = 161 * (uint64_t)(in_sample_rate / 16000) - 1;
    return FVAD_OK;
}

// The order: the weights and the lanes' format; then NULL sinks and the strides; then every sink's own rules (format,
// channels); then every sink's ranges (lanes, the samples of each source whose weight is not zero, bytes against out_bytes);
// then the overlap of two sinks' bytes.
int fvad_egress_mix_check(const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, int src_format, float w_orig, float w_den, size_t n_lanes,
                          size_t orig_stride, size_t orig_samples, size_t den_stride, size_t den_samples)
{
    if (!std::isfinite(w_orig) || !std::isfinite(w_den) || (w_orig == 0.0f && w_den == 0.0f)) return FVAD_ERR_INVALID_ARGUMENT;
    if (src_format != FVAD_INGEST_F32) return FVAD_ERR_INVALID_ARGUMENT; // PCM16 lanes would be a conversion
    if (n_sinks == 0) return FVAD_OK;
    if (!sinks) return FVAD_ERR_INVALID_ARGUMENT;
    const bool use_orig = w_orig != 0.0f, use_den = w_den != 0.0f;
    if (n_lanes > 1 && ((use_orig && orig_stride < orig_samples) || (use_den && den_stride < den_samples))) return FVAD_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n_sinks; ++i) {
        const uint64_t* r = sinks + i * FVAD_EGRESS_MIX_FIELDS;
        const uint64_t n_channels = r[2], format = r[3];
        if (format != FVAD_INGEST_F32 && format != FVAD_INGEST_PCM16 && format != FVAD_INGEST_PCM24) return FVAD_ERR_INVALID_ARGUMENT;
        if (n_channels < 1 || n_channels > 64) return FVAD_ERR_INVALID_ARGUMENT;
    }
    size_t n_ranges = 0;
    for (size_t i = 0; i < n_sinks; ++i) {
        const uint64_t* r = sinks + i * FVAD_EGRESS_MIX_FIELDS;
        const uint64_t byte_offset = r[0], n_frames = r[1], n_channels = r[2], format = r[3], first_lane = r[4], src_offset = r[5];
        const uint64_t orig_offset = r[6], orig_zeros = r[7];
        if (first_lane >= n_lanes || n_channels > n_lanes - first_lane) return FVAD_ERR_OUT_OF_RANGE;
        if (use_den && (src_offset > den_samples || n_frames > den_samples - src_offset)) return FVAD_ERR_OUT_OF_RANGE;
        const uint64_t n_read = n_frames - std::min(orig_zeros, n_frames); // the frames that have an original sample
        if (use_orig && (orig_offset > orig_samples || n_read > orig_samples - orig_offset)) return FVAD_ERR_OUT_OF_RANGE;
        const uint64_t frame_bytes = n_channels * sample_bytes(format);
        if (n_frames > UINT64_MAX / frame_bytes) return FVAD_ERR_OUT_OF_RANGE;
        if (byte_offset > out_bytes || n_frames * frame_bytes > out_bytes - byte_offset) return FVAD_ERR_OUT_OF_RANGE;
        if (n_frames) ++n_ranges;
    }
    // two sinks may not write one byte (fvad_egress_check's rule: ranges that touch are fine)
    std::vector<Range> ranges;
    ranges.reserve(n_ranges);
    for (size_t i = 0; i < n_sinks; ++i) {
        const uint64_t* r = sinks + i * FVAD_EGRESS_MIX_FIELDS;
        if (r[1] == 0) continue; // writes nothing
        ranges.push_back({r[0], r[0] + r[1] * r[2] * sample_bytes(r[3])});
    }
    std::sort(ranges.begin(), ranges.end(), [](const Range& x, const Range& y) { return x.from < y.from; });
    for (size_t k = 1; k < ranges.size(); ++k)
        if (ranges[k].from < ranges[k - 1].to) return FVAD_ERR_INVALID_ARGUMENT;
    return FVAD_OK;
}

} // extern "C"
