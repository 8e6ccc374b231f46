// ingest_san.cpp -- the host-only half of the device-side ingest (csrc/host_ingest.cpp) under AddressSanitizer + UBSan:
// fvad_wav_probe over seeded mutations of valid WAV headers (truncations, huge lengths, zero channels, block_align / bits that
// disagree, random byte flips) and fvad_ingest_check over seeded random source tables with values near UINT64_MAX for the
// overflow paths.  Built by tests/test_sanitizers_ingest.py; never loaded into Python.
//   usage: ingest_san <seed> <scratch file>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "fvad.h"

namespace {
using Bytes = std::vector<uint8_t>;
void put16(Bytes& b, uint32_t v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }
void put32(Bytes& b, uint32_t v) { put16(b, v & 0xffff); put16(b, v >> 16); }
void put_tag(Bytes& b, const char* t) { b.insert(b.end(), t, t + 4); }

// a valid file: [junk chunk] fmt (plain or extensible) data
Bytes valid_wav(std::mt19937_64& rng, int tag, int channels, int bits, bool extensible, bool junk, size_t frames)
{
    Bytes b;
    put_tag(b, "RIFF"); put32(b, 0); put_tag(b, "WAVE");
    if (junk) { put_tag(b, "junk"); put32(b, 3); b.insert(b.end(), {1, 2, 3, 0}); }
    const uint32_t block = (uint32_t)(channels * bits / 8);
    put_tag(b, "fmt "); put32(b, extensible ? 40 : 16);
    put16(b, extensible ? 0xFFFE : (uint32_t)tag); put16(b, (uint32_t)channels); put32(b, 48000); put32(b, 48000 * block); put16(b, block); put16(b, (uint32_t)bits);
    if (extensible) { put16(b, 22); put16(b, (uint32_t)bits); put32(b, 0); put16(b, (uint32_t)tag); for (int i = 0; i < 14; ++i) b.push_back((uint8_t)i); }
    put_tag(b, "data"); put32(b, (uint32_t)(frames * block));
    for (size_t i = 0; i < frames * block; ++i) b.push_back((uint8_t)rng());
    const uint32_t riff = (uint32_t)b.size() - 8;
    memcpy(&b[4], &riff, 4);
    return b;
}

bool write_file(const char* path, const Bytes& b)
{
    FILE* fp = fopen(path, "wb");
    if (!fp) return false;
    const size_t put = b.empty() ? 0 : fwrite(b.data(), 1, b.size(), fp);
    return fclose(fp) == 0 && put == b.size();
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: ingest_san <seed> <scratch file>\n"); return 2; }
    std::mt19937_64 rng((uint64_t)atoll(argv[1]));
    const char* path = argv[2];
    auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    long probes = 0, accepted = 0, tables = 0, ok_tables = 0;

    // ---- fvad_wav_probe
    const int kinds[3][2] = {{1, 16}, {1, 24}, {3, 32}};
    for (int round = 0; round < 120; ++round) {
        const int* k = kinds[pick(3)];
        const int channels = 1 + (int)pick(3);
        const size_t frames = (size_t)pick(9);
        Bytes b = valid_wav(rng, k[0], channels, k[1], pick(2) != 0, pick(2) != 0, frames);
        uint64_t info[FVAD_WAV_INFO_FIELDS];
        if (!write_file(path, b)) return 3;
        if (fvad_wav_probe(path, info) != FVAD_OK || info[1] != (uint64_t)channels || info[4] != frames || info[5] != (uint64_t)k[1] ||
            info[3] + frames * channels * (k[1] / 8) != b.size()) { fprintf(stderr, "a valid file was misread (round %d)\n", round); return 4; }
        for (int m = 0; m < 12; ++m) {
            Bytes x = b;
            switch (m) {
            case 0: x.resize(pick(x.size() + 1)); break;                                             // truncated anywhere
            case 1: { const uint32_t v = 0xFFFFFFF0u + (uint32_t)pick(16); memcpy(&x[x.size() - frames * channels * (k[1] / 8) - 4], &v, 4); } break; // a huge data length
            case 2: { const uint32_t v = 0xFFFFFFFFu - (uint32_t)pick(64); const size_t at = 16 + pick(x.size() > 24 ? x.size() - 24 : 1); if (at + 4 <= x.size()) memcpy(&x[at], &v, 4); } break;
            case 3: for (size_t i = 12; i + 24 < x.size(); ++i) if (!memcmp(&x[i], "fmt ", 4)) { x[i + 10] = x[i + 11] = 0; } break;   // zero channels
            case 4: for (size_t i = 12; i + 24 < x.size(); ++i) if (!memcmp(&x[i], "fmt ", 4)) { x[i + 20] = (uint8_t)pick(256); x[i + 22] = (uint8_t)pick(64); } break; // block_align / bits disagree
            case 5: for (size_t i = 12; i + 24 < x.size(); ++i) if (!memcmp(&x[i], "fmt ", 4)) { const uint32_t v = (uint32_t)pick(60); memcpy(&x[i + 4], &v, 4); } break; // the fmt chunk's own length
            case 6: x.resize(12 + pick(30)); break;
            default: for (int f = 0; f < 1 + (int)pick(6); ++f) if (!x.empty()) x[pick(x.size())] = (uint8_t)rng(); break; // random flips
            }
            if (!write_file(path, x)) return 3;
            uint64_t got[FVAD_WAV_INFO_FIELDS] = {0, 0, 0, 0, 0, 0};
            const int rc = fvad_wav_probe(path, got);
            ++probes;
            if (rc == FVAD_OK) {
                ++accepted;
                // what is accepted describes bytes that are in the file
                const uint64_t fb = got[1] * (got[5] / 8);
                if (got[0] > FVAD_INGEST_PCM24 || got[1] == 0 || got[2] == 0 || fb == 0 || got[3] > x.size() || got[4] > (x.size() - got[3]) / fb) {
                    fprintf(stderr, "an accepted header points outside its file (round %d, mutation %d)\n", round, m);
                    return 5;
                }
            }
        }
    }
    remove(path);

    // ---- fvad_ingest_check
    auto near_max = [&]() -> uint64_t {
        switch (pick(6)) {
        case 0: return UINT64_MAX - pick(4);
        case 1: return (UINT64_MAX >> pick(4)) + pick(3);
        case 2: return (1ull << 63) + pick(5) - 2;
        default: return pick(200);
        }
    };
    for (int round = 0; round < 4000; ++round) {
        const size_t n = (size_t)pick(7);
        const bool wild = pick(3) == 0;
        const size_t n_lanes = wild && pick(4) == 0 ? (size_t)near_max() : 1 + (size_t)pick(12);
        const size_t n_samples = wild && pick(4) == 0 ? (size_t)near_max() : (size_t)pick(300);
        const size_t lane_stride = wild && pick(4) == 0 ? (size_t)near_max() : n_samples + (size_t)pick(3);
        const uint64_t raw_bytes = pick(3) == 0 ? UINT64_MAX : wild ? near_max() : pick(5000);
        std::vector<uint64_t> rows(n * FVAD_INGEST_FIELDS + 1);
        for (size_t i = 0; i < n; ++i) {
            uint64_t* r = &rows[i * FVAD_INGEST_FIELDS];
            r[0] = wild && pick(3) == 0 ? near_max() : pick(4000);
            r[1] = wild && pick(3) == 0 ? near_max() : pick(40);
            r[2] = wild && pick(5) == 0 ? near_max() : 1 + pick(pick(8) ? 4 : 70);
            r[3] = pick(12) == 0 ? near_max() : pick(3);
            r[4] = wild && pick(4) == 0 ? near_max() : pick(12);
            r[5] = wild && pick(3) == 0 ? near_max() : pick(250);
            r[6] = wild && pick(3) == 0 ? near_max() : r[5] + r[1] + pick(30) - (pick(10) == 0);
        }
        const int out_format = pick(20) == 0 ? (int)pick(5) - 1 : (int)pick(2);
        const int rc = fvad_ingest_check(n ? rows.data() : (pick(2) ? rows.data() : nullptr), n, raw_bytes, out_format, n_lanes, lane_stride, n_samples);
        ++tables;
        if (rc == FVAD_OK) ++ok_tables;
        else if (rc != FVAD_ERR_INVALID_ARGUMENT && rc != FVAD_ERR_OUT_OF_RANGE) { fprintf(stderr, "an unexpected status %d\n", rc); return 6; }
        if (rc == FVAD_OK && n) { // what is accepted stays inside the lanes and the raw bytes, without wrapping
            for (size_t i = 0; i < n; ++i) {
                const uint64_t* r = &rows[i * FVAD_INGEST_FIELDS];
                const uint64_t fb = r[2] * (r[3] == FVAD_INGEST_PCM16 ? 2 : r[3] == FVAD_INGEST_PCM24 ? 3 : 4);
                if (r[2] < 1 || r[2] > 64 || r[3] > 2 || r[4] + r[2] > n_lanes || r[6] > n_samples || r[5] + r[1] > r[6] ||
                    r[1] > (raw_bytes - r[0]) / fb || r[0] > raw_bytes) { fprintf(stderr, "an accepted table is out of range (round %d)\n", round); return 7; }
            }
        }
    }
    if (ok_tables == 0 || ok_tables == tables || accepted == probes) { fprintf(stderr, "the driver is one-sided: %ld of %ld tables, %ld of %ld headers\n", ok_tables, tables, accepted, probes); return 8; }
    printf("probes=%ld accepted=%ld tables=%ld ok=%ld\n", probes, accepted, tables, ok_tables);
    return 0;
}
