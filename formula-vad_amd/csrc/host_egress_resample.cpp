// host_egress_resample.cpp -- the host-only half of the resampling egress (fvad_egress_resample*, engine_egress.cpp): the
// kernel's tile, the outputs a stream's leading frames can finish, and fvad_egress_resample_check, every argument rule of the
// device calls -- written once for it and for the strided form (host_egress_strided.cpp's entry calls it with its step).  Plain
// C++ without HIP headers, like host_egress.cpp (tests/sanitize/egress_resample_san.cpp builds this file and host_resample.cpp
// alone).
#include "egress_rules.h"
#include "egress_strided.h"

using namespace fvad;

namespace {
bool taps_count_ok(uint32_t n_taps) { return n_taps != 0 && n_taps % 2 == 1 && n_taps <= FVAD_RESAMPLE_TAPS_MAX; }
} // namespace

extern "C" {

uint64_t fvad_egress_resample_tile(uint32_t up, uint32_t down, uint32_t n_taps, uint32_t n_channels, uint32_t format)
{
    if (!ratio_ok(Ratio{up, down}) || !taps_count_ok(n_taps)) return 0;
    if (n_channels < 1 || n_channels > 64 || format > FVAD_INGEST_PCM24) return 0;
    return egress_resample_tile(Ratio{up, down}, n_taps, n_channels, format);
}

uint64_t fvad_egress_resample_ready(uint32_t up, uint32_t down, uint32_t n_taps, uint64_t stream_frames, uint64_t frames_have)
{
    if (!ratio_ok(Ratio{up, down}) || !taps_count_ok(n_taps)) return 0;
    return egress_resample_ready(Ratio{up, down}, n_taps, stream_frames, frames_have);
}

} // extern "C"

// Both checks.  The order: arguments (lane format, ratio, the step of the strided check, taps; then sinks, lane_stride); then every
// row's own rules (format, channels, the stream's length, the outputs against the stream, the given frames against the stream
// and against the window, the tile); then every row's ranges (lanes, given frames against n_samples -- `step` apart in the
// strided check, where a row without frames touches no sample whatever its src_offset --, bytes against out_bytes); then the
// overlap of two rows' bytes (both of egress_rules.h).  Every count of a strided row is in STRIDED samples.
int fvad::egress_resample_check(const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, uint32_t up, uint32_t down, const float* taps,
                                uint32_t n_taps, bool strided, uint32_t step, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    if (src_format != FVAD_INGEST_F32) return FVAD_ERR_INVALID_ARGUMENT; // PCM16 lanes would be a conversion; anything else is no format
    const Ratio q{up, down};
    if (!ratio_ok(q)) return FVAD_ERR_INVALID_ARGUMENT;
    if (strided && !egress_step_ok(step)) return FVAD_ERR_INVALID_ARGUMENT;
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
    for (size_t i = 0; i < n_sinks; ++i) {
        const uint64_t* r = sinks + i * FVAD_EGRESS_RESAMPLE_FIELDS;
        const uint64_t n_channels = r[2], first_lane = r[4], src_offset = r[5], n_frames = r[7];
        if (first_lane >= n_lanes || n_channels > n_lanes - first_lane) return FVAD_ERR_OUT_OF_RANGE;
        if (strided ? !egress_strided_span_ok(src_offset, n_frames, step, n_samples) : (src_offset > n_samples || n_frames > n_samples - src_offset))
            return FVAD_ERR_OUT_OF_RANGE;
        if (!egress_bytes_ok(r, out_bytes)) return FVAD_ERR_OUT_OF_RANGE;
    }
    if (!egress_rows_disjoint(sinks, n_sinks, FVAD_EGRESS_RESAMPLE_FIELDS)) return FVAD_ERR_INVALID_ARGUMENT;
    return FVAD_OK;
}

extern "C" {

int fvad_egress_resample_check(const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, uint32_t up, uint32_t down, const float* taps,
                               uint32_t n_taps, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    return egress_resample_check(sinks, n_sinks, out_bytes, up, down, taps, n_taps, false, 0, src_format, n_lanes, lane_stride, n_samples);
}

} // extern "C"
