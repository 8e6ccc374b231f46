// egress_rules.h -- the two rules every egress check shares (fvad_egress_check, fvad_egress_mix_check, fvad_egress_resample_check
// and its strided form), host only: a row's bytes against the output, and no byte written by two rows.  Every egress row begins
// {byte_offset, count (frames or outputs), n_channels, format}.  Inline and free of HIP headers, so that each host_egress*.cpp
// still builds alone (tests/sanitize/*_san.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "resample.h" // sample_bytes_of

namespace fvad {

// the row's count * frame bytes neither wraps nor leaves [byte_offset, out_bytes)
inline bool egress_bytes_ok(const uint64_t* r, uint64_t out_bytes)
{
    const uint64_t byte_offset = r[0], count = r[1], frame_bytes = r[2] * sample_bytes_of(r[3]);
    return count <= UINT64_MAX / frame_bytes && byte_offset <= out_bytes && count * frame_bytes <= out_bytes - byte_offset;
}

// Two rows may not write one byte: the order of the writes would decide the result.  The ranges sorted by their start must
// not reach into their successors (a range that ends where the next one starts is fine; a row without frames writes nothing).
// After egress_bytes_ok of every row: no range wraps.
inline bool egress_rows_disjoint(const uint64_t* rows, size_t n_rows, size_t n_fields)
{
    struct Range { uint64_t from, to; };
    std::vector<Range> ranges;
    ranges.reserve(n_rows);
    for (size_t i = 0; i < n_rows; ++i) {
        const uint64_t* r = rows + i * n_fields;
        if (r[1]) ranges.push_back({r[0], r[0] + r[1] * r[2] * sample_bytes_of(r[3])});
    }
    std::sort(ranges.begin(), ranges.end(), [](const Range& x, const Range& y) { return x.from < y.from; });
    for (size_t k = 1; k < ranges.size(); ++k)
        if (ranges[k].from < ranges[k - 1].to) return false;
    return true;
}

} // namespace fvad
