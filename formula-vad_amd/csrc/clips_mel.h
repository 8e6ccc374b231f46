// clips_mel.h -- the rules of a log-mel clip export (fvad_clips_plan_mel, fvad_clips_mel_check, fvad_clips_export_mel*), host
// only: the frame parameters, a clip's feature stream, its frame count and slot, and every argument rule of the two exports in
// the one order both report them in.  Inline, so that host_clips_mel.cpp and engine_clips.cpp state them once and the host
// file still builds alone (tests/sanitize/clips_mel_san.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/fvad.h"
#include "clips_strided.h"

namespace fvad {

constexpr uint64_t kMelSrcTile = 8192;  // kClipTile of kernels.h (engine_clips.cpp asserts it)
constexpr uint64_t kMelTileFrames = 32; // kClipMelTileFrames of kernels.h

struct Mel {
    uint32_t step;
    const uint32_t* skips; // NULL: all zero
    uint32_t n_fft, hop, n_mels;
};

inline bool mel_frames_ok(const Mel& m, const char** why)
{
    if (!strided_step_ok(m.step)) { *why = "a step of 0 or above FVAD_CLIP_STEP_MAX"; return false; }
    if (m.n_fft < 4 || m.n_fft > FVAD_CLIP_MEL_NFFT_MAX || m.n_fft % 2 != 0) { *why = "n_fft is odd or outside 4..FVAD_CLIP_MEL_NFFT_MAX"; return false; }
    if (m.hop < 1 || m.hop > m.n_fft) { *why = "hop is outside 1..n_fft"; return false; }
    if (m.n_mels < 1 || m.n_mels > FVAD_CLIP_MEL_BANDS_MAX) { *why = "n_mels is outside 1..FVAD_CLIP_MEL_BANDS_MAX"; return false; }
    return true;
}

// frames of one tile: as many as the staged window (F - 1) hop + n_fft <= kMelSrcTile allows, at most kMelTileFrames
inline uint64_t mel_tile_frames(uint32_t n_fft, uint32_t hop)
{
    const uint64_t fit = (kMelSrcTile - n_fft) / hop + 1;
    return fit < kMelTileFrames ? fit : kMelTileFrames;
}

// clip i of `len` samples: its skip's rules and the stream's length *L = ceil((len - skip) / step).  false: *why says which rule
inline bool mel_stream(uint32_t step, const uint32_t* skips, size_t i, uint64_t len, uint64_t* L, const char** why)
{
    const uint64_t skip = skips ? skips[i] : 0;
    if (skip >= step) { *why = "a skip that is not below the step"; return false; }
    if (len <= skip) { *why = "a clip that keeps no sample (len <= skip)"; return false; }
    const uint64_t rest = len - skip;
    *L = rest / step + (rest % step != 0);
    return true;
}

// a slot of t * n_mels floats at *at, which moves on to the next 16-byte boundary behind the slot
inline bool mel_advance(uint64_t t, uint32_t n_mels, uint64_t* at, const char** why)
{
    uint64_t cells, end;
    if (__builtin_mul_overflow(t, (uint64_t)n_mels, &cells) || __builtin_add_overflow(cells, (uint64_t)3, &cells) ||
        __builtin_add_overflow(*at, cells / 4 * 4, &end)) { *why = "the clips' total does not fit 64 bits"; return false; }
    *at = end;
    return true;
}

// clip i of `len` samples: its stream (mel_stream), *T = floor(L / hop) frames and its slot (mel_advance)
inline bool mel_slot(const Mel& m, size_t i, uint64_t len, uint64_t* at, uint64_t* L, uint64_t* T, const char** why)
{
    uint64_t n;
    if (!mel_stream(m.step, m.skips, i, len, &n, why)) return false;
    if (n < (uint64_t)m.n_fft / 2 + 1) { *why = "a clip too short to reflect (L < n_fft / 2 + 1)"; return false; }
    const uint64_t t = n / m.hop;
    if (t == 0) { *why = "a clip of no frame (L < hop)"; return false; }
    if (!mel_advance(t, m.n_mels, at, why)) return false;
    *L = n;
    *T = t;
    return true;
}

// the rules that a feature export's arguments share with fvad_clips_export's, in its order: NULLs, formats, alignment, lane_stride
// and the rows' own rules.  false: *why says which
inline bool feat_args_ok(const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples, const uint64_t* clips,
                         size_t n_clips, int out_format, const void* out, int device_out, const float* window, const float* matrix,
                         const char** why)
{
    if (!d_src || !clips || !out || !window || !matrix) { *why = "NULL argument"; return false; }
    if (src_format != FVAD_CLIP_F32 && src_format != FVAD_CLIP_PCM16) { *why = "unknown sample format"; return false; }
    if (out_format != FVAD_CLIP_F32) { *why = "features are f32: out_format must be FVAD_CLIP_F32"; return false; }
    if (device_out && (uintptr_t)out % 16 != 0) { *why = "the output must be 16-byte aligned"; return false; }
    if ((uintptr_t)d_src % (src_format == FVAD_CLIP_PCM16 ? 2 : 4) != 0) { *why = "the source is not aligned to its samples"; return false; }
    if (n_lanes > 1 && lane_stride < n_samples) { *why = "lane_stride < n_samples"; return false; }
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t* r = clips + i * FVAD_CLIP_FIELDS;
        if (r[3] <= r[2] || r[1] == 0) { *why = "a clip with sample_to <= sample_from or no channels"; return false; }
    }
    return true;
}

// FVAD_ERR_OUT_OF_RANGE for a clip past n_samples or n_lanes
inline int feat_range_ok(size_t n_lanes, size_t n_samples, const uint64_t* clips, size_t n_clips, const char** why)
{
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t* r = clips + i * FVAD_CLIP_FIELDS;
        if (r[3] > n_samples) { *why = "a clip ends past n_samples"; return FVAD_ERR_OUT_OF_RANGE; }
        if (r[0] >= n_lanes || r[1] > n_lanes - r[0]) { *why = "a clip's lanes end past n_lanes"; return FVAD_ERR_OUT_OF_RANGE; }
    }
    return FVAD_OK;
}

// the grids of a feature export: one workgroup per (clip, channel, tile) of the RMS and one per tile of frames, frames(i) a clip's
// frame count and tf the frames of a tile
template <typename Frames>
inline bool feat_grids_ok(const uint64_t* clips, size_t n_clips, Frames frames, uint64_t tf, const char** why)
{
    uint64_t tiles = 0, units = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t* r = clips + i * FVAD_CLIP_FIELDS;
        const uint64_t len = r[3] - r[2], nt = len / kMelSrcTile + (len % kMelSrcTile != 0), T = frames(i);
        uint64_t u;
        if (__builtin_mul_overflow(nt, r[1], &u) || __builtin_add_overflow(units, u, &units) || units > 0x7fffffffull ||
            __builtin_add_overflow(tiles, T / tf + (T % tf != 0), &tiles) || tiles > 0x7fffffffull) {
            *why = "more than 2^31 tiles in one call: export in batches";
            return false;
        }
    }
    return true;
}

inline bool mel_finite(float x) { return std::isfinite(x); }

// every rule of fvad_clips_export_mel(_device).  Pointers are addresses: nothing is read through d_src or out; window, matrix,
// norm, clips and skips are host memory and are read.  n_frames, offsets (may be NULL) and *total (may be NULL) are filled as far
// as the rules held.
inline int mel_check(const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples, const uint64_t* clips,
                     size_t n_clips, int out_format, const void* out, size_t out_capacity, int device_out, const Mel& m, const float* window,
                     const float* matrix, float floor, const float* norm, uint64_t* n_frames, uint64_t* offsets, uint64_t* total,
                     const char** why)
{
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (total) *total = 0;
    if (n_clips == 0) return FVAD_OK;
    if (!feat_args_ok(d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, out, device_out, window, matrix, why)) return FVAD_ERR_INVALID_ARGUMENT;
    if (!mel_frames_ok(m, why)) return FVAD_ERR_INVALID_ARGUMENT;
    uint64_t at = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t* r = clips + i * FVAD_CLIP_FIELDS;
        const uint64_t slot = at;
        uint64_t L, T;
        if (!mel_slot(m, i, r[3] - r[2], &at, &L, &T, why)) return FVAD_ERR_INVALID_ARGUMENT;
        if (offsets) offsets[i] = slot;
        if (n_frames) n_frames[i] = T;
    }
    if (total) *total = at;
    for (uint32_t i = 0; i < m.n_fft; ++i)
        if (!mel_finite(window[i])) { *why = "a window value that is not finite"; return FVAD_ERR_INVALID_ARGUMENT; }
    for (size_t i = 0; i < (size_t)m.n_mels * (m.n_fft / 2 + 1); ++i)
        if (!mel_finite(matrix[i])) { *why = "a matrix value that is not finite"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (!mel_finite(floor) || !(floor > 0.0f)) { *why = "a floor that is not finite and positive"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (norm && (!mel_finite(norm[0]) || !mel_finite(norm[1]) || !mel_finite(norm[2]))) { *why = "a norm value that is not finite"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (const int rc = feat_range_ok(n_lanes, n_samples, clips, n_clips, why)) return rc;
    if (at > out_capacity) { *why = "out_capacity is below fvad_clips_plan_mel's total"; return FVAD_ERR_BUFFER_TOO_SMALL; }
    const uint64_t tf = mel_tile_frames(m.n_fft, m.hop);
    const auto frames = [&](size_t i) {
        const uint64_t* r = clips + i * FVAD_CLIP_FIELDS;
        const uint64_t rest = r[3] - r[2] - (m.skips ? m.skips[i] : 0);
        return (rest / m.step + (rest % m.step != 0)) / m.hop;
    };
    if (!feat_grids_ok(clips, n_clips, frames, tf, why)) return FVAD_ERR_INVALID_ARGUMENT;
    return FVAD_OK;
}

} // namespace fvad
