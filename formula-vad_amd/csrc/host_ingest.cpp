// host_ingest.cpp -- the host-only half of the device-side ingest (fvad_ingest*, engine_ingest.cpp): fvad_wav_probe, which walks
// a WAV file's RIFF chunks as host_io.cpp's reader does but reads no sample, and fvad_ingest_check, every argument rule of the
// device calls.  Plain C++ without HIP headers, like host_io.cpp, so that both can be tested (and run under sanitizers) on a
// machine without a device.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/fvad.h"
#include "ingest_rules.h"

using namespace fvad;

namespace {
uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint16_t rd16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }

// n bytes at offset `at` of fp; false when the file ends before them
bool read_at(FILE* fp, uint64_t at, void* out, size_t n) { return fseeko(fp, (off_t)at, SEEK_SET) == 0 && fread(out, 1, n, fp) == n; }
} // namespace

extern "C" {

int fvad_wav_probe(const char* path, uint64_t* info)
{
    if (!path || !info) return FVAD_ERR_INVALID_ARGUMENT;
    FILE* fp = fopen(path, "rb");
    if (!fp) return FVAD_ERR_IO;
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{fp};
    if (fseeko(fp, 0, SEEK_END) != 0) return FVAD_ERR_IO;
    const off_t end = ftello(fp);
    if (end < 0) return FVAD_ERR_IO;
    const uint64_t size = (uint64_t)end;
    uint8_t head[12];
    if (size < 12) return FVAD_ERR_MODEL_FORMAT;
    if (!read_at(fp, 0, head, 12)) return FVAD_ERR_IO;
    if (memcmp(head, "RIFF", 4) != 0 || memcmp(head + 8, "WAVE", 4) != 0) return FVAD_ERR_MODEL_FORMAT;
    // fvad_wav_read's walk (host_io.cpp wav_parse): the first "fmt " chunk in front of the first "data" chunk
    int fmt_tag = 0, channels = 0, bits = 0;
    uint32_t rate = 0;
    bool have_data = false;
    uint64_t data_off = 0, data_bytes = 0;
    uint64_t pos = 12;
    while (pos + 8 <= size) {
        uint8_t ck[8];
        if (!read_at(fp, pos, ck, 8)) return FVAD_ERR_IO;
        const uint64_t len = rd32(ck + 4);
        const uint64_t body = pos + 8;
        if (memcmp(ck, "fmt ", 4) == 0 && len >= 16 && body + 16 <= size) {
            uint8_t f[26];
            const bool ext = len >= 26 && body + 26 <= size;
            if (!read_at(fp, body, f, ext ? 26 : 16)) return FVAD_ERR_IO;
            fmt_tag = rd16(f);
            channels = rd16(f + 2);
            rate = rd32(f + 4);
            bits = rd16(f + 14);
            if (fmt_tag == 0xFFFE && ext) fmt_tag = rd16(f + 24); // WAVE_FORMAT_EXTENSIBLE: sub-format GUID's first word
        } else if (memcmp(ck, "data", 4) == 0) {
            have_data = true;
            data_off = body;
            data_bytes = body + len <= size ? len : size - body; // tolerate a truncated / streaming length
            break;
        }
        pos = body + len + (len & 1);
    }
    if (!have_data || channels <= 0 || rate == 0) return FVAD_ERR_MODEL_FORMAT;
    uint64_t format;
    if (fmt_tag == 1 && bits == 16) format = FVAD_INGEST_PCM16;
    else if (fmt_tag == 1 && bits == 24) format = FVAD_INGEST_PCM24;
    else if (fmt_tag == 3 && bits == 32) format = FVAD_INGEST_F32;
    else return FVAD_ERR_MODEL_FORMAT;
    const uint64_t frame_bytes = (uint64_t)channels * (uint64_t)(bits / 8);
    info[0] = format;
    info[1] = (uint64_t)channels;
    info[2] = rate;
    info[3] = data_off;
    info[4] = data_bytes / frame_bytes; // a partial last frame is dropped
    info[5] = (uint64_t)bits;
    return FVAD_OK;
}

// The order: arguments; then every source's own rules (format and pair, channels, fill_to); then every source's ranges (lanes,
// fill_to against n_samples, bytes against raw_bytes); then the overlap of two sources' destinations -- the last two are
// ingest_rules.h's, shared with fvad_ingest_resample_check.
int fvad_ingest_check(const uint64_t* sources, size_t n_sources, uint64_t raw_bytes, int out_format, size_t n_lanes,
                      size_t lane_stride, size_t n_samples)
{
    if (out_format != FVAD_INGEST_F32 && out_format != FVAD_INGEST_PCM16) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sources == 0) return FVAD_OK;
    if (!sources) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_lanes > 1 && lane_stride < n_samples) return FVAD_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n_sources; ++i) {
        const uint64_t* r = sources + i * FVAD_INGEST_FIELDS;
        const uint64_t n_frames = r[1], n_channels = r[2], format = r[3], dst_offset = r[5], fill_to = r[6];
        if (format != FVAD_INGEST_F32 && format != FVAD_INGEST_PCM16 && format != FVAD_INGEST_PCM24) return FVAD_ERR_INVALID_ARGUMENT;
        // exact pairs only: PCM16 lanes take PCM16 sources; PCM24 -> PCM16 and f32 -> PCM16 are conversions, not ingest
        if (out_format == FVAD_INGEST_PCM16 && format != FVAD_INGEST_PCM16) return FVAD_ERR_INVALID_ARGUMENT;
        if (n_channels < 1 || n_channels > 64) return FVAD_ERR_INVALID_ARGUMENT;
        if (n_frames > UINT64_MAX - dst_offset || fill_to < dst_offset + n_frames) return FVAD_ERR_INVALID_ARGUMENT;
    }
    const int rc = ingest_ranges_check(sources, n_sources, FVAD_INGEST_FIELDS, raw_bytes, n_lanes, n_samples);
    if (rc != FVAD_OK) return rc;
    if (!ingest_rows_disjoint(sources, n_sources, FVAD_INGEST_FIELDS)) return FVAD_ERR_INVALID_ARGUMENT;
    return FVAD_OK;
}

} // extern "C"
