// host_egress.cpp -- the host-only half of the device-side egress (fvad_egress*, engine_egress.cpp): fvad_wav_header, the
// 44-byte canonical header host_io.cpp's wav_put writes (and its 24-bit PCM form, which wav_put has not), and fvad_egress_check,
// every argument rule of the device calls.  Plain C++ without HIP headers, like host_ingest.cpp, so that it can be tested (and
// run under sanitizers) on a machine without a device.
#include <cstdint>
#include <cstring>

#include "egress_rules.h"

using namespace fvad;

namespace {
void wr16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
void wr32(uint8_t* p, uint32_t v) { wr16(p, v & 0xffff); wr16(p + 2, v >> 16); }
} // namespace

extern "C" {

int fvad_wav_header(int format, uint32_t n_channels, uint32_t sample_rate, uint64_t n_frames, uint8_t* out, size_t cap, size_t* n_bytes)
{
    if (n_bytes) *n_bytes = 0;
    if (!out || !n_bytes) return FVAD_ERR_INVALID_ARGUMENT;
    if (format != FVAD_INGEST_F32 && format != FVAD_INGEST_PCM16 && format != FVAD_INGEST_PCM24) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_channels == 0 || n_channels > 65535 || sample_rate == 0) return FVAD_ERR_INVALID_ARGUMENT; // wav_put's refusals
    const uint64_t bytes_per = sample_bytes_of((uint64_t)format), frame_bytes = n_channels * bytes_per;
    if (n_frames > 0xFFFFFF00ull / frame_bytes) return FVAD_ERR_INVALID_ARGUMENT; // RIFF sizes are 32-bit
    const uint64_t data_bytes = n_frames * frame_bytes;
    *n_bytes = FVAD_WAV_HEADER_BYTES;
    if (cap < FVAD_WAV_HEADER_BYTES) return FVAD_ERR_BUFFER_TOO_SMALL;
    memcpy(out, "RIFF", 4); wr32(out + 4, (uint32_t)(36 + data_bytes)); memcpy(out + 8, "WAVEfmt ", 8);
    wr32(out + 16, 16); wr16(out + 20, format == FVAD_INGEST_F32 ? 3 : 1); wr16(out + 22, n_channels); wr32(out + 24, sample_rate);
    wr32(out + 28, (uint32_t)(sample_rate * frame_bytes)); wr16(out + 32, (uint32_t)frame_bytes); wr16(out + 34, (uint32_t)(bytes_per * 8));
    memcpy(out + 36, "data", 4); wr32(out + 40, (uint32_t)data_bytes);
    return FVAD_OK;
}

// The order: arguments; then every sink's own rules (format and pair, channels); then every sink's ranges (lanes, samples
// against n_samples, bytes against out_bytes); then the overlap of two sinks' bytes (both of egress_rules.h).
int fvad_egress_check(const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, int src_format, size_t n_lanes, size_t lane_stride,
                      size_t n_samples)
{
    if (src_format != FVAD_INGEST_F32 && src_format != FVAD_INGEST_PCM16) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks == 0) return FVAD_OK;
    if (!sinks) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_lanes > 1 && lane_stride < n_samples) return FVAD_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n_sinks; ++i) {
        const uint64_t* r = sinks + i * FVAD_EGRESS_FIELDS;
        const uint64_t n_channels = r[2], format = r[3];
        if (format != FVAD_INGEST_F32 && format != FVAD_INGEST_PCM16 && format != FVAD_INGEST_PCM24) return FVAD_ERR_INVALID_ARGUMENT;
        // PCM16 lanes go to PCM16 files only: PCM16 -> f32 and PCM16 -> PCM24 are conversions, not egress
        if (src_format == FVAD_INGEST_PCM16 && format != FVAD_INGEST_PCM16) return FVAD_ERR_INVALID_ARGUMENT;
        if (n_channels < 1 || n_channels > 64) return FVAD_ERR_INVALID_ARGUMENT;
    }
    for (size_t i = 0; i < n_sinks; ++i) {
        const uint64_t* r = sinks + i * FVAD_EGRESS_FIELDS;
        const uint64_t n_frames = r[1], n_channels = r[2], first_lane = r[4], src_offset = r[5];
        if (first_lane >= n_lanes || n_channels > n_lanes - first_lane) return FVAD_ERR_OUT_OF_RANGE;
        if (src_offset > n_samples || n_frames > n_samples - src_offset) return FVAD_ERR_OUT_OF_RANGE;
        if (!egress_bytes_ok(r, out_bytes)) return FVAD_ERR_OUT_OF_RANGE;
    }
    if (!egress_rows_disjoint(sinks, n_sinks, FVAD_EGRESS_FIELDS)) return FVAD_ERR_INVALID_ARGUMENT;
    return FVAD_OK;
}

} // extern "C"
