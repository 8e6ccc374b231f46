// clips_features.h -- the rules of the feature clip exports, host only: the log-mel family (fvad_clips_plan_mel,
// fvad_clips_mel_check, fvad_clips_export_mel*) and the Kaldi-style filter-bank family (fvad_clips_plan_fbank,
// fvad_clips_fbank_check, fvad_clips_export_fbank*).  One set of frame parameters, a clip's feature stream, its frame count
// (feature_frames.h) and slot, and every argument rule in the one order all of a family's entry points report them in; what
// differs between the families hangs on Feat::snip.  Inline, so that host_clips_features.cpp and engine_clips.cpp state them
// once and the host file still builds alone (tests/sanitize/clips_mel_san.cpp, clips_fbank_san.cpp, clips_feat_split_san.cpp).
// The split-source calls (fvad_clips_split_mel_check, fvad_clips_split_fbank_check, fvad_clips_export_split_mel*, _split_fbank*)
// take clips_split.h's rows and its piece and overlap rules around the same family rules (feat_split_check).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/fvad.h"
#include "clips_split.h"
#include "clips_strided.h"
#include "feature_frames.h"

namespace fvad {

// the frame parameters of a family: frames of `taps` samples every `hop`, transformed at n_fft.
//   log-mel:     taps == n_fft, centred with reflection (snip off)
//   filter-bank: taps == win_length <= n_fft, Kaldi's snip_edges (snip on); a plan, which does not know n_fft, holds
//                win_length to the largest one by stating n_fft = FVAD_CLIP_MEL_NFFT_MAX
struct Feat {
    uint32_t step;
    const uint32_t* skips; // NULL: all zero
    uint32_t taps, n_fft, hop, n_mels;
    bool snip;
};

// what a family's own rules look at: floor and norm (log-mel; norm may be NULL), or scale, preemph, remove_dc, floor and cmn
struct FeatCond {
    float floor;
    const float* norm;
    float scale, preemph;
    int remove_dc, cmn;
};

inline bool feat_frames_ok(const Feat& f, const char** why)
{
    if (!strided_step_ok(f.step)) { *why = "a step of 0 or above FVAD_CLIP_STEP_MAX"; return false; }
    if (f.n_fft < 4 || f.n_fft > FVAD_CLIP_MEL_NFFT_MAX || f.n_fft % 2 != 0) { *why = "n_fft is odd or outside 4..FVAD_CLIP_MEL_NFFT_MAX"; return false; }
    if (f.snip && (f.taps < 2 || f.taps > f.n_fft)) { *why = "win_length is outside 2..n_fft"; return false; }
    if (f.hop < 1 || f.hop > f.taps) { *why = f.snip ? "hop is outside 1..win_length" : "hop is outside 1..n_fft"; return false; }
    if (f.n_mels < 1 || f.n_mels > FVAD_CLIP_MEL_BANDS_MAX) { *why = "n_mels is outside 1..FVAD_CLIP_MEL_BANDS_MAX"; return false; }
    return true;
}

// a slot of t * n_mels floats at *at, which moves on to the next 16-byte boundary behind the slot
inline bool feat_advance(uint64_t t, uint32_t n_mels, uint64_t* at, const char** why)
{
    uint64_t cells, end;
    if (__builtin_mul_overflow(t, (uint64_t)n_mels, &cells) || __builtin_add_overflow(cells, (uint64_t)3, &cells) ||
        __builtin_add_overflow(*at, cells / 4 * 4, &end)) { *why = "the clips' total does not fit 64 bits"; return false; }
    *at = end;
    return true;
}

// clip i of `len` samples: its skip's rules, its stream of L = ceil((len - skip) / step) samples, *T frames of it and its slot
// (feat_advance).  false: *why says which rule
inline bool feat_slot(const Feat& f, size_t i, uint64_t len, uint64_t* at, uint64_t* T, const char** why)
{
    const uint64_t skip = f.skips ? f.skips[i] : 0;
    if (skip >= f.step) { *why = "a skip that is not below the step"; return false; }
    if (len <= skip) { *why = "a clip that keeps no sample (len <= skip)"; return false; }
    const uint64_t L = feat_stream_len<uint64_t>(len, skip, f.step);
    if (!f.snip && L < (uint64_t)f.n_fft / 2 + 1) { *why = "a clip too short to reflect (L < n_fft / 2 + 1)"; return false; }
    if (f.snip && L < f.taps) { *why = "a clip shorter than one frame (L < win_length)"; return false; }
    const uint64_t t = feat_frames<uint64_t>(f.snip, L, f.taps, f.hop);
    if (t == 0) { *why = "a clip of no frame (L < hop)"; return false; }
    if (!feat_advance(t, f.n_mels, at, why)) return false;
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

// the grids of a feature export: one workgroup per (clip, channel, tile) of the RMS and one per tile of frames.  len(i) and
// chans(i) are clip i's samples and channels; n_frames is what the slot walk wrote; NULL: the clips' frame counts are computed
// again (every clip has passed feat_slot)
template <typename Len, typename Chans>
inline bool feat_grids_ok(const Feat& f, size_t n_clips, Len len_of, Chans chans, const uint64_t* n_frames, const char** why)
{
    const uint64_t tf = feat_tile_frames(f.taps, f.hop);
    uint64_t tiles = 0, units = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t len = len_of(i), nt = len / kFeatSrcTile + (len % kFeatSrcTile != 0);
        const uint64_t T = n_frames ? n_frames[i] : feat_frames<uint64_t>(f.snip, feat_stream_len<uint64_t>(len, f.skips ? f.skips[i] : 0, f.step), f.taps, f.hop);
        uint64_t u;
        if (__builtin_mul_overflow(nt, chans(i), &u) || __builtin_add_overflow(units, u, &units) || units > 0x7fffffffull ||
            __builtin_add_overflow(tiles, T / tf + (T % tf != 0), &tiles) || tiles > 0x7fffffffull) {
            *why = "more than 2^31 tiles in one call: export in batches";
            return false;
        }
    }
    return true;
}

inline const char* feat_capacity_why(const Feat& f) { return f.snip ? "out_capacity is below fvad_clips_plan_fbank's total" : "out_capacity is below fvad_clips_plan_mel's total"; }

inline bool feat_finite(float x) { return std::isfinite(x); }

// A family's own rules, in feat_check's order from the frame parameters on: every clip's skip, length (len(i) samples) and slot,
// window and matrix finite, the family's conditions.  n_frames, offsets (may be NULL) and *total (may be NULL) are filled as far
// as the rules held; *end is the total
template <typename Len>
inline bool feat_family_ok(const Feat& f, size_t n_clips, Len len, const float* window, const float* matrix, const FeatCond& c, uint64_t* n_frames,
                           uint64_t* offsets, uint64_t* total, uint64_t* end, const char** why)
{
    if (!feat_frames_ok(f, why)) return false;
    uint64_t at = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t slot = at;
        uint64_t T;
        if (!feat_slot(f, i, len(i), &at, &T, why)) return false;
        if (offsets) offsets[i] = slot;
        if (n_frames) n_frames[i] = T;
    }
    if (total) *total = at;
    for (uint32_t i = 0; i < f.taps; ++i)
        if (!feat_finite(window[i])) { *why = "a window value that is not finite"; return false; }
    for (size_t i = 0; i < (size_t)f.n_mels * (f.n_fft / 2 + 1); ++i)
        if (!feat_finite(matrix[i])) { *why = "a matrix value that is not finite"; return false; }
    if (f.snip) {
        if (!feat_finite(c.scale) || c.scale == 0.0f) { *why = "a scale that is not finite and non-zero"; return false; }
        if (!feat_finite(c.preemph) || !(c.preemph >= 0.0f) || !(c.preemph <= 1.0f)) { *why = "a preemph that is not in 0..1"; return false; }
        if (c.remove_dc != 0 && c.remove_dc != 1) { *why = "remove_dc is not 0 or 1"; return false; }
    }
    if (!feat_finite(c.floor) || !(c.floor > 0.0f)) { *why = "a floor that is not finite and positive"; return false; }
    if (f.snip && c.cmn != 0 && c.cmn != 1) { *why = "cmn is not 0 or 1"; return false; }
    if (!f.snip && c.norm && (!feat_finite(c.norm[0]) || !feat_finite(c.norm[1]) || !feat_finite(c.norm[2]))) { *why = "a norm value that is not finite"; return false; }
    *end = at;
    return true;
}

// every rule of a family's export.  Pointers are addresses: nothing is read through d_src or out; window, matrix, c.norm, clips
// and skips are host memory and are read.  n_frames, offsets (may be NULL) and *total (may be NULL) are filled as far as the
// rules held.
inline int feat_check(const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples, const uint64_t* clips,
                      size_t n_clips, int out_format, const void* out, size_t out_capacity, int device_out, const Feat& f, const float* window,
                      const float* matrix, const FeatCond& c, uint64_t* n_frames, uint64_t* offsets, uint64_t* total, const char** why)
{
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (total) *total = 0;
    if (n_clips == 0) return FVAD_OK;
    if (!feat_args_ok(d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, out, device_out, window, matrix, why)) return FVAD_ERR_INVALID_ARGUMENT;
    uint64_t at = 0;
    const auto len = [&](size_t i) { return clips[i * FVAD_CLIP_FIELDS + 3] - clips[i * FVAD_CLIP_FIELDS + 2]; };
    if (!feat_family_ok(f, n_clips, len, window, matrix, c, n_frames, offsets, total, &at, why)) return FVAD_ERR_INVALID_ARGUMENT;
    if (const int rc = feat_range_ok(n_lanes, n_samples, clips, n_clips, why)) return rc;
    if (at > out_capacity) { *why = feat_capacity_why(f); return FVAD_ERR_BUFFER_TOO_SMALL; }
    if (!feat_grids_ok(f, n_clips, len, [&](size_t i) { return clips[i * FVAD_CLIP_FIELDS + 1]; }, n_frames, why)) return FVAD_ERR_INVALID_ARGUMENT;
    return FVAD_OK;
}

// Every rule of a family's split-source export, in the one order its six entry points report them in (fvad.h): the split
// export's rules (host_clips_split.cpp) down to the rows' own, with the feature calls' NULLs and output format directly behind
// the format rule; the family's rules over len = a_len + b_len; the pieces' ranges; the capacity; the output beside the sources;
// the two grids.  Pointers are addresses, as in feat_check.
inline int feat_split_check(const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b, size_t b_lanes, size_t b_stride,
                            size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips, int out_format, const void* out,
                            size_t out_capacity, int device_out, const Feat& f, const float* window, const float* matrix, const FeatCond& c,
                            uint64_t* n_frames, uint64_t* offsets, uint64_t* total, const char** why)
{
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (total) *total = 0;
    if (n_clips == 0) return FVAD_OK;
    if (!clips || !out) { *why = "NULL argument"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (!format_ok(src_format) || !format_ok(out_format)) { *why = "unknown sample format"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (!window || !matrix) { *why = "NULL argument"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (out_format != FVAD_CLIP_F32) { *why = "features are f32: out_format must be FVAD_CLIP_F32"; return FVAD_ERR_INVALID_ARGUMENT; }
    for (size_t i = 0; i < n_clips; ++i) {
        const SplitRow r = split_row(clips, i);
        if ((r.a_len && !d_a) || (r.b_len && !d_b)) { *why = "a NULL source that a clip takes samples from"; return FVAD_ERR_INVALID_ARGUMENT; }
    }
    const uint64_t sb = format_bytes(src_format);
    if ((uintptr_t)d_a % sb != 0 || (uintptr_t)d_b % sb != 0) { *why = "a source is not aligned to its samples"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (device_out && (uintptr_t)out % 16 != 0) { *why = "the output must be 16-byte aligned"; return FVAD_ERR_INVALID_ARGUMENT; }
    if ((a_lanes > 1 && a_stride < a_samples) || (b_lanes > 1 && b_stride < b_samples)) { *why = "a stride below its sample count"; return FVAD_ERR_INVALID_ARGUMENT; }
    const auto len = [&](size_t i) {
        const SplitRow r = split_row(clips, i);
        uint64_t n;
        return r.n_channels == 0 || __builtin_add_overflow(r.a_len, r.b_len, &n) ? 0 : n;
    };
    for (size_t i = 0; i < n_clips; ++i)
        if (len(i) == 0) { *why = "a clip with both lengths 0 or no channels"; return FVAD_ERR_INVALID_ARGUMENT; }
    uint64_t at = 0;
    if (!feat_family_ok(f, n_clips, len, window, matrix, c, n_frames, offsets, total, &at, why)) return FVAD_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n_clips; ++i) {
        const SplitRow r = split_row(clips, i);
        if (!piece_ok(r.a_lane, r.n_channels, r.a_from, r.a_len, a_lanes, a_samples) ||
            !piece_ok(r.b_lane, r.n_channels, r.b_from, r.b_len, b_lanes, b_samples)) {
            *why = "a piece ends past its buffer's samples or lanes";
            return FVAD_ERR_OUT_OF_RANGE;
        }
    }
    if (at > out_capacity) { *why = feat_capacity_why(f); return FVAD_ERR_BUFFER_TOO_SMALL; }
    const Range o = buffer_range(out, 1, 0, at, sizeof(float));
    if (overlap(o, buffer_range(d_a, a_lanes, a_stride, a_samples, sb)) || overlap(o, buffer_range(d_b, b_lanes, b_stride, b_samples, sb))) {
        *why = "the output overlaps a source";
        return FVAD_ERR_INVALID_ARGUMENT;
    }
    if (!feat_grids_ok(f, n_clips, len, [&](size_t i) { return split_row(clips, i).n_channels; }, n_frames, why)) return FVAD_ERR_INVALID_ARGUMENT;
    return FVAD_OK;
}

} // namespace fvad
