// clips_split.h -- the argument rules of fvad_clips_export_split(_device), host only (host_clips_split.cpp), shared with the
// export itself (engine_clips.cpp)
#pragma once
#include "clips_rules.h"

namespace fvad {

struct SplitRow { uint64_t n_channels, a_lane, a_from, a_len, b_lane, b_from, b_len; };
inline SplitRow split_row(const uint64_t* clips, size_t i)
{
    const uint64_t* r = clips + i * FVAD_CLIP_SPLIT_FIELDS;
    return {r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
}

// fvad_clips_split_check with the reason of a refusal in *why (a literal).  form (clips_rules.h): the rules of the strided,
// filtered or resampled split export as well, directly after the rows' own; offsets, total and the capacity rule are then that
// form's slots', and its gather's tiles are in the count of the grid
int clips_split_check(const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b, size_t b_lanes,
                      size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips, int out_format,
                      const void* out, size_t out_capacity, int device_out, uint64_t* offsets, uint64_t* total, const char** why,
                      const ClipForm& form);

} // namespace fvad
