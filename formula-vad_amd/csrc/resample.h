// resample.h -- the rules of the resampling ingest (fvad_resample_*, fvad_ingest_resample*), host only: the ratio, the output
// count, the input window of a range of outputs, the tap rules and the kernel's tile.  Inline, so that host_resample.cpp and
// engine_ingest.cpp state them once and host_resample.cpp still builds alone (tests/sanitize/resample_san.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/fvad.h"

namespace fvad {

typedef unsigned __int128 u128;

constexpr uint64_t kResampleTileBytes = 16384; // the window a tile stages when the filter's reach leaves room for 64 outputs
constexpr uint64_t kResampleLdsMax = 65520;    // ... and the most a tile may stage (+ 16 bytes of alignment slack = 64 KB of LDS)
constexpr uint64_t kResampleTileMax = 4096;    // outputs of one channel per tile at most
constexpr uint64_t kResampleFramesUp = 1ull << 62; // file_frames * up stays below this: o * down + K fits 64 bits with room

struct Ratio { uint32_t up, down; };
inline bool ratio_ok(const Ratio& r) { return r.up >= 1 && r.up <= FVAD_RESAMPLE_UP_MAX && r.down >= 1; }

inline uint64_t sample_bytes_of(uint64_t format) { return format == FVAD_INGEST_PCM16 ? 2 : format == FVAD_INGEST_PCM24 ? 3 : 4; }

// ceil(file_frames * up / down), saturated at UINT64_MAX
inline uint64_t resample_out_frames(uint64_t file_frames, const Ratio& r)
{
    const u128 n = ((u128)file_frames * r.up + r.down - 1) / r.down;
    return n > (u128)UINT64_MAX ? UINT64_MAX : (uint64_t)n;
}

// The input frames outputs [out_from, out_from + n_out) read, clipped to the file: output o reads the n with
// 0 <= K + o down - n up <= 2 K.  An empty window (n_out == 0, outputs behind the file's reach, a phase without taps) is
// lo == hi.
inline void resample_window(const Ratio& r, uint32_t n_taps, uint64_t file_frames, uint64_t out_from, uint64_t n_out, uint64_t* lo, uint64_t* hi)
{
    *lo = *hi = 0;
    if (n_out == 0) return;
    const u128 K = (n_taps - 1) / 2;
    const u128 p0 = (u128)out_from * r.down, p1 = ((u128)out_from + (n_out - 1)) * r.down;
    const u128 a = p0 > K ? (p0 - K + r.up - 1) / r.up : 0; // ceil((p0 - K) / up), at least 0
    const u128 b = (p1 + K) / r.up + 1;                       // floor((p1 + K) / up) + 1
    const u128 lo128 = a < (u128)file_frames ? a : (u128)file_frames;
    const u128 hi128 = b < (u128)file_frames ? b : (u128)file_frames;
    *lo = (uint64_t)lo128;
    *hi = hi128 > lo128 ? (uint64_t)hi128 : *lo;
}

// the most frames n consecutive outputs read: floor(((n - 1) down + 2 K) / up) + 1
inline u128 resample_reach(const Ratio& r, uint32_t n_taps, uint64_t n) { return ((u128)(n - 1) * r.down + (n_taps - 1)) / r.up + 1; }

// the most consecutive outputs (a multiple of 4, at most `most`) whose window fits `bytes`; 0 when not even 4 do
inline uint64_t resample_fit(const Ratio& r, uint32_t n_taps, uint64_t frame_bytes, uint64_t bytes, uint64_t most)
{
    const u128 frames = bytes / frame_bytes; // reach(n) <= frames  <=>  (n - 1) down + 2 K < frames up
    if (frames == 0 || frames * r.up <= (u128)(n_taps - 1)) return 0;
    u128 n = (frames * r.up - (n_taps - 1) - 1) / r.down + 1;
    if (n > most) n = most;
    return (uint64_t)n / 4 * 4;
}

// The kernel's tile in outputs of one channel: what fits kResampleTileBytes of staged source bytes; when the filter's reach
// leaves room for fewer than 64 outputs there, what fits kResampleLdsMax.  0: not even 4 outputs' window fits (refused).
inline uint64_t resample_tile(const Ratio& r, uint32_t n_taps, uint64_t n_channels, uint64_t format)
{
    const uint64_t fb = n_channels * sample_bytes_of(format);
    const uint64_t t = resample_fit(r, n_taps, fb, kResampleTileBytes, kResampleTileMax);
    return t >= 64 ? t : resample_fit(r, n_taps, fb, kResampleLdsMax, kResampleTileMax);
}

struct Taps { const float* taps; uint32_t n_taps; }; // host memory

// false: *why says which rule
inline bool resample_taps_ok(const Taps& f, const char** why)
{
    if (!f.taps) { *why = "NULL taps"; return false; }
    if (f.n_taps == 0 || f.n_taps % 2 == 0) { *why = "n_taps is 0 or even"; return false; }
    if (f.n_taps > FVAD_RESAMPLE_TAPS_MAX) { *why = "n_taps above FVAD_RESAMPLE_TAPS_MAX"; return false; }
    for (uint32_t k = 0; k < f.n_taps; ++k)
        if (!std::isfinite(f.taps[k])) { *why = "a tap that is not finite"; return false; }
    return true;
}

// taps per phase at most: ceil(n_taps / up)
inline uint32_t resample_phase_taps(uint32_t up, uint32_t n_taps) { return (n_taps + up - 1) / up; }

// The taps as the kernel walks them: table[j * up + (o mod up)] = taps[r + j * up], r = (K + o down) mod up, the phase of every
// output with that o mod up; 0 where r + j * up is past the taps (the kernel does not read those).  So the lanes of a
// wavefront, which take neighbouring outputs, read neighbouring words.
inline std::vector<float> resample_table(const Taps& f, const Ratio& q)
{
    const uint32_t J = resample_phase_taps(q.up, f.n_taps), K = (f.n_taps - 1) / 2;
    std::vector<float> t((size_t)J * q.up, 0.0f);
    for (uint32_t om = 0; om < q.up; ++om) {
        const uint32_t r = (uint32_t)(((uint64_t)K + (uint64_t)om * q.down) % q.up);
        for (uint32_t j = 0; (uint64_t)r + (uint64_t)j * q.up < f.n_taps; ++j) t[(size_t)j * q.up + om] = f.taps[r + j * q.up];
    }
    return t;
}

} // namespace fvad
