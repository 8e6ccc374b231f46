// egress_san.cpp -- the host-only half of the device-side egress (csrc/host_egress.cpp) under AddressSanitizer + UBSan:
// fvad_wav_header over seeded random arguments and capacities (the buffer is exactly `cap` bytes of the heap, so a byte past it
// is caught) and fvad_egress_check over seeded random sink tables with values near UINT64_MAX for the overflow paths.  Built by
// tests/test_sanitizers_egress.py; never loaded into Python.
//   usage: egress_san <seed>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "fvad.h"

namespace {
uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
} // namespace

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: egress_san <seed>\n"); return 2; }
    std::mt19937_64 rng((uint64_t)atoll(argv[1]));
    auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    auto near_max = [&]() -> uint64_t {
        switch (pick(6)) {
        case 0: return UINT64_MAX - pick(4);
        case 1: return (UINT64_MAX >> pick(4)) + pick(3);
        case 2: return (1ull << 63) + pick(5) - 2;
        default: return pick(200);
        }
    };
    long headers = 0, ok_headers = 0, tables = 0, ok_tables = 0;

    // ---- fvad_wav_header
    for (int round = 0; round < 3000; ++round) {
        const int format = pick(10) == 0 ? (int)pick(7) - 2 : (int)pick(3);
        const uint32_t channels = pick(4) == 0 ? (uint32_t)(pick(3) == 0 ? near_max() : 65530 + pick(12)) : (uint32_t)pick(70);
        const uint32_t rate = pick(8) == 0 ? (uint32_t)near_max() : (uint32_t)pick(200000);
        const uint64_t frames = pick(3) == 0 ? near_max() : pick(2) ? pick(1ull << 33) : pick(5000);
        const size_t cap = pick(3) == 0 ? (size_t)pick(44) : 44 + (size_t)pick(20);
        std::vector<uint8_t> out(cap, 0xEE);
        size_t n = 12345;
        const bool null_out = pick(40) == 0, null_n = pick(40) == 0;
        const int rc = fvad_wav_header(format, channels, rate, frames, null_out ? nullptr : out.data(), cap, null_n ? nullptr : &n);
        ++headers;
        if (rc == FVAD_OK) {
            ++ok_headers;
            // what is accepted is a whole header inside its buffer that says what was asked for, in 32 bits
            const uint64_t B = format == FVAD_INGEST_PCM16 ? 2 : format == FVAD_INGEST_PCM24 ? 3 : 4;
            if (null_out || null_n || n != FVAD_WAV_HEADER_BYTES || cap < n || format < 0 || format > 2 || channels < 1 || channels > 65535 || rate == 0 ||
                frames > 0xFFFFFF00ull / (channels * B) || rd32(&out[40]) != frames * channels * B || rd32(&out[4]) != 36 + frames * channels * B ||
                rd16(&out[22]) != channels || rd32(&out[24]) != rate || rd16(&out[34]) != 8 * B || rd16(&out[32]) != ((channels * B) & 0xFFFF) /* (16 bits, as fvad_wav_write leaves it) */ ||
                rd16(&out[20]) != (format == FVAD_INGEST_F32 ? 3u : 1u)) { fprintf(stderr, "an accepted header is wrong (round %d)\n", round); return 4; }
            for (size_t i = n; i < cap; ++i) if (out[i] != 0xEE) { fprintf(stderr, "a byte behind the header was written (round %d)\n", round); return 4; }
        } else if (rc == FVAD_ERR_BUFFER_TOO_SMALL) {
            if (cap >= FVAD_WAV_HEADER_BYTES || n != FVAD_WAV_HEADER_BYTES) { fprintf(stderr, "a wrong BUFFER_TOO_SMALL (round %d)\n", round); return 5; }
            for (size_t i = 0; i < cap; ++i) if (out[i] != 0xEE) { fprintf(stderr, "a refused call wrote (round %d)\n", round); return 5; }
        } else if (rc != FVAD_ERR_INVALID_ARGUMENT) { fprintf(stderr, "an unexpected status %d\n", rc); return 6; }
    }

    // ---- fvad_egress_check
    for (int round = 0; round < 4000; ++round) {
        const size_t n = (size_t)pick(7);
        const bool wild = pick(3) == 0;
        const size_t n_lanes = wild && pick(4) == 0 ? (size_t)near_max() : 1 + (size_t)pick(12);
        const size_t n_samples = wild && pick(4) == 0 ? (size_t)near_max() : (size_t)pick(300);
        const size_t lane_stride = wild && pick(4) == 0 ? (size_t)near_max() : n_samples + (size_t)pick(3);
        const uint64_t out_bytes = pick(3) == 0 ? UINT64_MAX : wild ? near_max() : pick(20000);
        std::vector<uint64_t> rows(n * FVAD_EGRESS_FIELDS + 1);
        uint64_t at = pick(50);
        for (size_t i = 0; i < n; ++i) {
            uint64_t* r = &rows[i * FVAD_EGRESS_FIELDS];
            r[1] = wild && pick(3) == 0 ? near_max() : pick(40);
            r[2] = wild && pick(5) == 0 ? near_max() : 1 + pick(pick(8) ? 4 : 70);
            r[3] = pick(12) == 0 ? near_max() : pick(3);
            r[4] = wild && pick(4) == 0 ? near_max() : pick(12);
            r[5] = wild && pick(3) == 0 ? near_max() : pick(250);
            // mostly one behind the other (so that tables are accepted), sometimes anywhere
            r[0] = wild && pick(3) == 0 ? near_max() : pick(4) == 0 ? pick(4000) : at;
            at = r[0] + r[1] * r[2] * 4 + pick(3); // (wraps with wild values: unsigned, and then just another offset)
        }
        const int src_format = pick(20) == 0 ? (int)pick(5) - 1 : (int)pick(2);
        const int rc = fvad_egress_check(n ? rows.data() : (pick(2) ? rows.data() : nullptr), n, out_bytes, src_format, n_lanes, lane_stride, n_samples);
        ++tables;
        if (rc == FVAD_OK) ++ok_tables;
        else if (rc != FVAD_ERR_INVALID_ARGUMENT && rc != FVAD_ERR_OUT_OF_RANGE) { fprintf(stderr, "an unexpected status %d\n", rc); return 6; }
        if (rc == FVAD_OK && n) { // what is accepted stays inside the lanes and the output bytes, without wrapping, and no two sinks share a byte
            for (size_t i = 0; i < n; ++i) {
                const uint64_t* r = &rows[i * FVAD_EGRESS_FIELDS];
                const uint64_t fb = r[2] * (r[3] == FVAD_INGEST_PCM16 ? 2 : r[3] == FVAD_INGEST_PCM24 ? 3 : 4);
                if (r[2] < 1 || r[2] > 64 || r[3] > 2 || (src_format == FVAD_INGEST_PCM16 && r[3] != FVAD_INGEST_PCM16) || r[4] >= n_lanes ||
                    r[2] > n_lanes - r[4] || r[5] > n_samples || r[1] > n_samples - r[5] || r[0] > out_bytes || r[1] > (out_bytes - r[0]) / fb ||
                    (n_lanes > 1 && lane_stride < n_samples)) { fprintf(stderr, "an accepted table is out of range (round %d)\n", round); return 7; }
                for (size_t k = 0; k < i; ++k) {
                    const uint64_t* q = &rows[k * FVAD_EGRESS_FIELDS];
                    const uint64_t qb = q[1] * q[2] * (q[3] == FVAD_INGEST_PCM16 ? 2 : q[3] == FVAD_INGEST_PCM24 ? 3 : 4);
                    if (r[1] && q[1] && r[0] < q[0] + qb && q[0] < r[0] + r[1] * fb) { fprintf(stderr, "two accepted sinks overlap (round %d)\n", round); return 7; }
                }
            }
        }
    }
    if (ok_tables == 0 || ok_tables == tables || ok_headers == 0 || ok_headers == headers) { fprintf(stderr, "the driver is one-sided: %ld of %ld tables, %ld of %ld headers\n", ok_tables, tables, ok_headers, headers); return 8; }
    printf("headers=%ld accepted=%ld tables=%ld ok=%ld\n", headers, ok_headers, tables, ok_tables);
    return 0;
}
