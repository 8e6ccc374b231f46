// clips_rules.h -- the rules every clip export shares (fvad_clips_plan, fvad_clips_export*, fvad_clips_export_split*,
// fvad_clips_split_check), host only: the sample formats, the walk that gives every clip its slot in the full-rate, strided /
// filtered and resampled forms, and the gather's tiles per clip.  The forms' own rules are clips_strided.h's, clips_fir.h's and
// clips_resample.h's.  Inline and free of HIP headers, so that engine_clips.cpp and host_clips_split.cpp state them once and the
// host file still builds alone (tests/sanitize/clips_split_san.cpp).
#pragma once
#include "clips_fir.h"
#include "clips_resample.h"
#include "clips_strided.h"

namespace fvad {

constexpr uint64_t kClipSrcTile = 8192; // kClipTile of kernels.h (engine_clips.cpp asserts it)

inline bool format_ok(int f) { return f == FVAD_CLIP_F32 || f == FVAD_CLIP_PCM16; }
inline uint64_t format_bytes(int f) { return f == FVAD_CLIP_PCM16 ? 2 : 4; }

// which export: all NULL the full-rate one; strided, with fir or without; or rs (never beside strided)
struct ClipForm {
    const Strided* strided;
    const Fir* fir;
    const Resampled* rs;
};

// Every clip's slot: offsets[i] (offsets may be NULL) and *total, in samples of the output format (per16 of them in 16 bytes;
// every slot starts on a 16-byte boundary).  len(i) is clip i's length, 0 for a row that breaks its own rules (*why = bad_row).
// First the full-rate slots of all clips, then the form's own rules and its slots in place of them: the step, each clip's skip
// and slot, the taps (strided / fir); or the ratio and the taps, each clip's 2^62 / up rule and slot (rs).  false: *why says
// which rule and *family whose it is ("" the shared ones, "strided", "fir", "resampled").
template <typename Len>
inline bool clip_slots(const ClipForm& f, size_t n_clips, Len len, const char* bad_row, uint64_t per16, uint64_t* offsets, uint64_t* total,
                       const char** family, const char** why)
{
    *family = "";
    uint64_t at = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t n = len(i);
        if (n == 0) { *why = bad_row; return false; }
        if (offsets) offsets[i] = at;
        if (at > UINT64_MAX - per16 || n > UINT64_MAX - per16 - at) { *why = "the clips' total does not fit 64 bits"; return false; }
        at += (n + per16 - 1) / per16 * per16;
    }
    if (f.strided) {
        *family = "strided";
        if (!strided_step_ok(f.strided->step)) { *why = "a step of 0 or above FVAD_CLIP_STEP_MAX"; return false; }
    }
    if (f.rs) {
        *family = "resampled";
        if (!resampled_ok(*f.rs, why)) return false;
    }
    if (f.strided || f.rs) {
        at = 0;
        for (size_t i = 0; i < n_clips; ++i) {
            const uint64_t slot = at;
            uint64_t out_len;
            if (f.rs) {
                if ((u128)len(i) * f.rs->up >= (u128)kResampleFramesUp) { *why = "a clip of 2^62 / up samples or more"; return false; }
                if (!resampled_slot(Ratio{f.rs->up, f.rs->down}, len(i), per16, &at, &out_len, why)) return false;
            } else if (!strided_slot(*f.strided, i, len(i), per16, &at, &out_len, why)) return false;
            if (offsets) offsets[i] = slot;
        }
    }
    if (f.fir) {
        *family = "fir";
        if (!fir_taps_ok(*f.fir, why)) return false;
    }
    *total = at;
    return true;
}

// the gather's tile in output samples (clip_tile_out, clip_fir_tile_out of kernels.h; a step of 1 keeps every sample: the
// full-rate gather, whose tiles are the strided gather's)
inline uint64_t form_tile_out(const ClipForm& f)
{
    if (f.rs) return resampled_tile_out(Ratio{f.rs->up, f.rs->down}, f.rs->n_taps);
    const uint32_t step = f.strided ? f.strided->step : 1;
    return f.fir ? fir_tile_out(step, f.fir->n_taps) : strided_tile_out(step);
}

inline uint32_t form_skip(const ClipForm& f, size_t i) { return f.strided && f.strided->skips ? f.strided->skips[i] : 0; }

// the gather's tiles of clip i of `len` samples (after clip_slots): its outputs in tiles of form_tile_out
inline uint64_t form_gather_tiles(const ClipForm& f, size_t i, uint64_t len)
{
    const uint64_t step = f.strided ? f.strided->step : 1, to = form_tile_out(f);
    const uint64_t n = f.rs ? resample_out_frames(len, Ratio{f.rs->up, f.rs->down}) : (len - form_skip(f, i) + step - 1) / step;
    return n / to + (n % to != 0);
}

} // namespace fvad
