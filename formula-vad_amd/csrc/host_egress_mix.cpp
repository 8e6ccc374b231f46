// host_egress_mix.cpp -- the host-only half of the two-source egress (fvad_egress_mix*, engine_egress.cpp):
// fvad_nsnet2_delay, the lag of the denoised lanes behind the original ones, and fvad_egress_mix_check, every argument rule of
// the device calls.  Plain C++ without HIP headers, like host_egress.cpp, so that it can be tested (and run under sanitizers)
// on a machine without a device.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "egress_rules.h"

using namespace fvad;

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
// then the overlap of two sinks' bytes (both of egress_rules.h).
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
    for (size_t i = 0; i < n_sinks; ++i) {
        const uint64_t* r = sinks + i * FVAD_EGRESS_MIX_FIELDS;
        const uint64_t n_frames = r[1], n_channels = r[2], first_lane = r[4], src_offset = r[5], orig_offset = r[6], orig_zeros = r[7];
        if (first_lane >= n_lanes || n_channels > n_lanes - first_lane) return FVAD_ERR_OUT_OF_RANGE;
        if (use_den && (src_offset > den_samples || n_frames > den_samples - src_offset)) return FVAD_ERR_OUT_OF_RANGE;
        const uint64_t n_read = n_frames - std::min(orig_zeros, n_frames); // the frames that have an original sample
        if (use_orig && (orig_offset > orig_samples || n_read > orig_samples - orig_offset)) return FVAD_ERR_OUT_OF_RANGE;
        if (!egress_bytes_ok(r, out_bytes)) return FVAD_ERR_OUT_OF_RANGE;
    }
    if (!egress_rows_disjoint(sinks, n_sinks, FVAD_EGRESS_MIX_FIELDS)) return FVAD_ERR_INVALID_ARGUMENT;
    return FVAD_OK;
}

} // extern "C"
