// ingest_rules.h -- the two rules both ingest checks share (fvad_ingest_check, fvad_ingest_resample_check), host only: every
// source's ranges, and no sample written by two sources.  Every ingest row begins {byte_offset, n_frames, n_channels, format,
// first_lane, dst_offset, fill_to}.  Both come after a check's own rules (format, 1 .. 64 channels, fill_to not below what the
// source writes), so which refusal wins stays each check's.  Inline and free of HIP headers, so that host_ingest.cpp and
// host_resample.cpp still build alone (tests/sanitize/ingest_san.cpp, resample_san.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "resample.h" // sample_bytes_of

namespace fvad {

// every source's lanes against n_lanes, fill_to against n_samples, bytes against raw_bytes: FVAD_OK or FVAD_ERR_OUT_OF_RANGE
inline int ingest_ranges_check(const uint64_t* rows, size_t n_rows, size_t n_fields, uint64_t raw_bytes, size_t n_lanes, size_t n_samples)
{
    for (size_t i = 0; i < n_rows; ++i) {
        const uint64_t* r = rows + i * n_fields;
        const uint64_t byte_offset = r[0], n_frames = r[1], n_channels = r[2], format = r[3], first_lane = r[4], fill_to = r[6];
        if (first_lane >= n_lanes || n_channels > n_lanes - first_lane) return FVAD_ERR_OUT_OF_RANGE;
        if (fill_to > n_samples) return FVAD_ERR_OUT_OF_RANGE;
        const uint64_t frame_bytes = n_channels * sample_bytes_of(format);
        if (n_frames > UINT64_MAX / frame_bytes) return FVAD_ERR_OUT_OF_RANGE;
        if (byte_offset > raw_bytes || n_frames * frame_bytes > raw_bytes - byte_offset) return FVAD_ERR_OUT_OF_RANGE;
    }
    return FVAD_OK;
}

// Two sources may not write one sample: the order of the writes would decide the result.  Per lane, the ranges [dst_offset,
// fill_to) sorted by their start must not reach into their successors (a source with fill_to == dst_offset writes nothing).
inline bool ingest_rows_disjoint(const uint64_t* rows, size_t n_rows, size_t n_fields)
{
    struct Rect { uint64_t lane, from, to; };
    size_t n_rects = 0;
    for (size_t i = 0; i < n_rows; ++i)
        if (rows[i * n_fields + 6] > rows[i * n_fields + 5]) n_rects += (size_t)rows[i * n_fields + 2];
    std::vector<Rect> rects;
    rects.reserve(n_rects);
    for (size_t i = 0; i < n_rows; ++i) {
        const uint64_t* r = rows + i * n_fields;
        if (r[6] <= r[5]) continue; // writes nothing
        for (uint64_t c = 0; c < r[2]; ++c) rects.push_back({r[4] + c, r[5], r[6]});
    }
    std::sort(rects.begin(), rects.end(), [](const Rect& x, const Rect& y) { return x.lane != y.lane ? x.lane < y.lane : x.from < y.from; });
    for (size_t k = 1; k < rects.size(); ++k)
        if (rects[k].lane == rects[k - 1].lane && rects[k].from < rects[k - 1].to) return false;
    return true;
}

} // namespace fvad
