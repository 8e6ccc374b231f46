// host_clips_split.cpp -- fvad_clips_split_check: every argument rule of fvad_clips_export_split(_device), in the one order both
// forms report them in, without a device (plain C++: tests/sanitize/clips_split_san.cpp builds this file alone).  Pointers are
// addresses here; nothing is read through d_a, d_b or out.
#include "clips_split.h"

namespace fvad {

int clips_split_check(const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b, size_t b_lanes,
                      size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips, int out_format,
                      const void* out, size_t out_capacity, int device_out, uint64_t* offsets, uint64_t* total, const char** why,
                      const ClipForm& form)
{
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (total) *total = 0;
    if (n_clips == 0) return FVAD_OK;
    // NULLs and formats
    if (!clips || !out) { *why = "NULL argument"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (!format_ok(src_format) || !format_ok(out_format)) { *why = "unknown sample format"; return FVAD_ERR_INVALID_ARGUMENT; }
    for (size_t i = 0; i < n_clips; ++i) {
        const SplitRow r = split_row(clips, i);
        if ((r.a_len && !d_a) || (r.b_len && !d_b)) { *why = "a NULL source that a clip takes samples from"; return FVAD_ERR_INVALID_ARGUMENT; }
    }
    // alignment
    const uint64_t sb = format_bytes(src_format), ob = format_bytes(out_format);
    if ((uintptr_t)d_a % sb != 0 || (uintptr_t)d_b % sb != 0) { *why = "a source is not aligned to its samples"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (device_out && (uintptr_t)out % 16 != 0) { *why = "the output must be 16-byte aligned"; return FVAD_ERR_INVALID_ARGUMENT; }
    // strides
    if ((a_lanes > 1 && a_stride < a_samples) || (b_lanes > 1 && b_stride < b_samples)) { *why = "a stride below its sample count"; return FVAD_ERR_INVALID_ARGUMENT; }
    // every row's own rules and the slots fvad_clips_plan gives clips of these lengths, then the form's rules and slots
    const auto len = [&](size_t i) {
        const SplitRow r = split_row(clips, i);
        uint64_t n;
        return r.n_channels == 0 || __builtin_add_overflow(r.a_len, r.b_len, &n) ? 0 : n;
    };
    const char* family;
    uint64_t at = 0;
    if (!clip_slots(form, n_clips, len, "a clip with both lengths 0 or no channels", 16 / ob, offsets, &at, &family, why)) return FVAD_ERR_INVALID_ARGUMENT;
    if (total) *total = at;
    // ranges and lanes
    for (size_t i = 0; i < n_clips; ++i) {
        const SplitRow r = split_row(clips, i);
        if (!piece_ok(r.a_lane, r.n_channels, r.a_from, r.a_len, a_lanes, a_samples) ||
            !piece_ok(r.b_lane, r.n_channels, r.b_from, r.b_len, b_lanes, b_samples)) {
            *why = "a piece ends past its buffer's samples or lanes";
            return FVAD_ERR_OUT_OF_RANGE;
        }
    }
    if (at > out_capacity) { *why = "out_capacity is below the plan's total"; return FVAD_ERR_BUFFER_TOO_SMALL; }
    // the output beside the sources: what the call may write against what it may read, by address
    const Range o = buffer_range(out, 1, 0, at, ob);
    if (overlap(o, buffer_range(d_a, a_lanes, a_stride, a_samples, sb)) || overlap(o, buffer_range(d_b, b_lanes, b_stride, b_samples, sb))) {
        *why = "the output overlaps a source";
        return FVAD_ERR_INVALID_ARGUMENT;
    }
    // the grid: one workgroup per (clip, channel, tile); a strided gather has tiles of its own, of at most as many samples
    uint64_t units = 0, gather = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const SplitRow r = split_row(clips, i);
        const uint64_t len = r.a_len + r.b_len, nt = len / kClipSrcTile + (len % kClipSrcTile != 0);
        uint64_t u;
        if (__builtin_mul_overflow(nt, r.n_channels, &u) || __builtin_add_overflow(units, u, &units) || units > 0x7fffffffull) {
            *why = "more than 2^31 tiles in one call: export in batches";
            return FVAD_ERR_INVALID_ARGUMENT;
        }
        if (__builtin_add_overflow(gather, form_gather_tiles(form, i, len), &gather) || gather > 0x7fffffffull) {
            *why = "more than 2^31 tiles in one call: export in batches";
            return FVAD_ERR_INVALID_ARGUMENT;
        }
    }
    return FVAD_OK;
}

} // namespace fvad

extern "C" int fvad_clips_split_check(const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                      size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips,
                                      size_t n_clips, int out_format, const void* out, size_t out_capacity, int device_out,
                                      uint64_t* offsets, uint64_t* total)
{
    return fvad::clips_split_check(d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips,
                                   out_format, out, out_capacity, device_out, offsets, total, nullptr, fvad::ClipForm{});
}
