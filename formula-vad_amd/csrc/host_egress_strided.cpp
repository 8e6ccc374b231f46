// host_egress_strided.cpp -- the host-only half of the strided resampling egress (fvad_egress_resample_strided*, the strided
// entries of engine_egress_resample.cpp): fvad_egress_resample_strided_check, every argument rule of the device calls.  The tile
// and the ready count are fvad_egress_resample_tile's and fvad_egress_resample_ready's as they are.  Plain C++ without HIP
// headers, like host_egress_resample.cpp (tests/sanitize/egress_strided_san.cpp builds this file, host_egress_resample.cpp and
// host_resample.cpp alone).
#include <algorithm>

#include "egress_strided.h"

using namespace fvad;

static_assert(kEgressStepMax == FVAD_EGRESS_STEP_MAX, "egress_strided.h restates fvad.h's step");

namespace {
struct Range { uint64_t from, to; };
} // namespace

extern "C" {

// fvad_egress_resample_check's rules in its order, with two changes: the step's rule directly behind the ratio's, and the
// given frames' lane range counted `src_step` apart.  Every count of a row is in STRIDED samples.
int fvad_egress_resample_strided_check(const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, uint32_t up, uint32_t down, const float* taps,
                                       uint32_t n_taps, uint32_t src_step, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    if (src_format != FVAD_INGEST_F32) return FVAD_ERR_INVALID_ARGUMENT; // PCM16 lanes would be a conversion; anything else is no format
    const Ratio q{up, down};
    if (!ratio_ok(q)) return FVAD_ERR_INVALID_ARGUMENT;
    if (!egress_step_ok(src_step)) return FVAD_ERR_INVALID_ARGUMENT;
    const char* why;
    if (!resample_taps_ok(Taps{taps, n_taps}, &why)) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks == 0) return FVAD_OK;
    if (!sinks) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_lanes > 1 && lane_stride < n_samples) return FVAD_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n_sinks; ++i) {
        const uint64_t* r = sinks + i * FVAD_EGRESS_RESAMPLE_FIELDS;
        const uint64_t n_out = r[1], n_channels = r[2], format = r[3], frame_base = r[6], n_frames = r[7], stream_frames = r[8], out_from = r[9];
        if (format != FVAD_INGEST_F32 && format != FVAD_INGEST_PCM16 && format != FVAD_INGEST_PCM24) return FVAD_ERR_INVALID_ARGUMENT;
        if (n_channels < 1 || n_channels > 64) return FVAD_ERR_INVALID_ARGUMENT;
        if ((u128)stream_frames * up >= (u128)kResampleFramesUp) return FVAD_ERR_INVALID_ARGUMENT;
        if (n_out > UINT64_MAX - out_from || out_from + n_out > resample_out_frames(stream_frames, q)) return FVAD_ERR_INVALID_ARGUMENT;
        if (n_frames > UINT64_MAX - frame_base || frame_base + n_frames > stream_frames) return FVAD_ERR_INVALID_ARGUMENT;
        uint64_t lo, hi;
        resample_window(q, n_taps, stream_frames, out_from, n_out, &lo, &hi);
        if (hi > lo && (frame_base > lo || frame_base + n_frames < hi)) return FVAD_ERR_INVALID_ARGUMENT; // the slice would not be the stream
        if (egress_resample_tile(q, n_taps, n_channels, format) == 0) return FVAD_ERR_INVALID_ARGUMENT; // taps too long for a tile
    }
    size_t n_ranges = 0;
    for (size_t i = 0; i < n_sinks; ++i) {
        const uint64_t* r = sinks + i * FVAD_EGRESS_RESAMPLE_FIELDS;
        const uint64_t byte_offset = r[0], n_out = r[1], n_channels = r[2], format = r[3], first_lane = r[4], src_offset = r[5], n_frames = r[7];
        if (first_lane >= n_lanes || n_channels > n_lanes - first_lane) return FVAD_ERR_OUT_OF_RANGE;
        if (!egress_strided_span_ok(src_offset, n_frames, src_step, n_samples)) return FVAD_ERR_OUT_OF_RANGE;
        const uint64_t frame_bytes = n_channels * sample_bytes_of(format);
        if (n_out > UINT64_MAX / frame_bytes) return FVAD_ERR_OUT_OF_RANGE;
        if (byte_offset > out_bytes || n_out * frame_bytes > out_bytes - byte_offset) return FVAD_ERR_OUT_OF_RANGE;
        if (n_out) ++n_ranges;
    }
    // two rows may not write one byte (fvad_egress_check's rule; ranges that touch are fine)
    std::vector<Range> ranges;
    ranges.reserve(n_ranges);
    for (size_t i = 0; i < n_sinks; ++i) {
        const uint64_t* r = sinks + i * FVAD_EGRESS_RESAMPLE_FIELDS;
        if (r[1] == 0) continue; // writes nothing
        ranges.push_back({r[0], r[0] + r[1] * r[2] * sample_bytes_of(r[3])});
    }
    std::sort(ranges.begin(), ranges.end(), [](const Range& x, const Range& y) { return x.from < y.from; });
    for (size_t k = 1; k < ranges.size(); ++k)
        if (ranges[k].from < ranges[k - 1].to) return FVAD_ERR_INVALID_ARGUMENT;
    return FVAD_OK;
}

} // extern "C"
