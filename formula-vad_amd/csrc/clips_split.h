// clips_split.h -- the argument rules of fvad_clips_export_split(_device), host only (host_clips_split.cpp), shared with the
// export itself (engine_clips.cpp); the rows, the piece and overlap rules are inline, so that the split feature calls' rules
// (clips_features.h) state them too and host_clips_features.cpp still builds alone
#pragma once
#include "clips_rules.h"

namespace fvad {

struct SplitRow { uint64_t n_channels, a_lane, a_from, a_len, b_lane, b_from, b_len; };
inline SplitRow split_row(const uint64_t* clips, size_t i)
{
    const uint64_t* r = clips + i * FVAD_CLIP_SPLIT_FIELDS;
    return {r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
}

// the bytes [lo, hi) a buffer of n_lanes lanes covers, saturating at the top of the address space
struct Range { uint64_t lo, hi; };
inline Range buffer_range(const void* p, uint64_t n_lanes, uint64_t stride, uint64_t n_samples, uint64_t bytes)
{
    const uint64_t lo = (uint64_t)(uintptr_t)p;
    if (!p || n_lanes == 0) return {lo, lo};
    uint64_t n, b, hi;
    if (__builtin_mul_overflow(n_lanes - 1, n_lanes > 1 ? stride : 0, &n) || __builtin_add_overflow(n, n_samples, &n) ||
        __builtin_mul_overflow(n, bytes, &b) || __builtin_add_overflow(lo, b, &hi))
        return {lo, UINT64_MAX};
    return {lo, hi};
}
inline bool overlap(Range x, Range y) { return x.lo < x.hi && y.lo < y.hi && x.lo < y.hi && y.lo < x.hi; }

// one piece of a row inside its buffer (a piece of no samples takes nothing and has no rule)
inline bool piece_ok(uint64_t lane, uint64_t n_channels, uint64_t from, uint64_t len, uint64_t n_lanes, uint64_t n_samples)
{
    if (len == 0) return true;
    return from <= n_samples && len <= n_samples - from && lane < n_lanes && n_channels <= n_lanes - lane;
}

// fvad_clips_split_check with the reason of a refusal in *why (a literal).  form (clips_rules.h): the rules of the strided,
// filtered or resampled split export as well, directly after the rows' own; offsets, total and the capacity rule are then that
// form's slots', and its gather's tiles are in the count of the grid
int clips_split_check(const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b, size_t b_lanes,
                      size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips, int out_format,
                      const void* out, size_t out_capacity, int device_out, uint64_t* offsets, uint64_t* total, const char** why,
                      const ClipForm& form);

} // namespace fvad
