// clips_fbank.h -- the rules of a Kaldi-style filter-bank clip export (fvad_clips_plan_fbank, fvad_clips_fbank_check,
// fvad_clips_export_fbank*), host only: the frame parameters, a clip's frame count (snip_edges) and slot, and every argument rule
// of the two exports in the one order both report them in.  The feature stream, the slots and the rules shared with every clip
// export are clips_mel.h's.  Inline, so that host_clips_fbank.cpp and engine_clips.cpp state them once and the host file still
// builds alone (tests/sanitize/clips_fbank_san.cpp).
#pragma once
#include "clips_mel.h"

namespace fvad {

struct Fbank {
    uint32_t step;
    const uint32_t* skips; // NULL: all zero
    uint32_t win_length, n_fft, hop, n_mels;
};

// the plan's rules: it does not know n_fft, so win_length is held to the largest one
inline bool fbank_plan_ok(uint32_t step, uint32_t win_length, uint32_t hop, uint32_t n_mels, const char** why)
{
    if (!strided_step_ok(step)) { *why = "a step of 0 or above FVAD_CLIP_STEP_MAX"; return false; }
    if (win_length < 2 || win_length > FVAD_CLIP_MEL_NFFT_MAX) { *why = "win_length is outside 2..n_fft"; return false; }
    if (hop < 1 || hop > win_length) { *why = "hop is outside 1..win_length"; return false; }
    if (n_mels < 1 || n_mels > FVAD_CLIP_MEL_BANDS_MAX) { *why = "n_mels is outside 1..FVAD_CLIP_MEL_BANDS_MAX"; return false; }
    return true;
}

inline bool fbank_frames_ok(const Fbank& f, const char** why)
{
    if (!strided_step_ok(f.step)) { *why = "a step of 0 or above FVAD_CLIP_STEP_MAX"; return false; }
    if (f.n_fft < 4 || f.n_fft > FVAD_CLIP_MEL_NFFT_MAX || f.n_fft % 2 != 0) { *why = "n_fft is odd or outside 4..FVAD_CLIP_MEL_NFFT_MAX"; return false; }
    if (f.win_length > f.n_fft) { *why = "win_length is outside 2..n_fft"; return false; }
    return fbank_plan_ok(f.step, f.win_length, f.hop, f.n_mels, why);
}

// frames of one tile: as many as the staged window (F - 1) hop + win_length <= kMelSrcTile allows, at most kMelTileFrames
inline uint64_t fbank_tile_frames(uint32_t win_length, uint32_t hop) { return mel_tile_frames(win_length, hop); }

// a stream of L samples: T = 1 + (L - win_length) / hop frames (Kaldi's snip_edges = true); 0 for L < win_length
inline uint64_t fbank_frames(uint64_t L, uint32_t win_length, uint32_t hop) { return L < win_length ? 0 : 1 + (L - win_length) / hop; }

// clip i of `len` samples: its stream (mel_stream), *T frames and its slot (mel_advance).  false: *why says which rule
inline bool fbank_slot(uint32_t step, const uint32_t* skips, uint32_t win_length, uint32_t hop, uint32_t n_mels, size_t i, uint64_t len,
                       uint64_t* at, uint64_t* T, const char** why)
{
    uint64_t n;
    if (!mel_stream(step, skips, i, len, &n, why)) return false;
    const uint64_t t = fbank_frames(n, win_length, hop);
    if (t == 0) { *why = "a clip shorter than one frame (L < win_length)"; return false; }
    if (!mel_advance(t, n_mels, at, why)) return false;
    *T = t;
    return true;
}

// what the conditioning and the end of a call take beside the frames
struct FbankCond {
    float scale, preemph;
    int remove_dc;
    float floor;
    int cmn;
};

// every rule of fvad_clips_export_fbank(_device).  Pointers are addresses: nothing is read through d_src or out; window, matrix,
// clips and skips are host memory and are read.  n_frames, offsets (may be NULL) and *total (may be NULL) are filled as far as
// the rules held.
inline int fbank_check(const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples, const uint64_t* clips,
                       size_t n_clips, int out_format, const void* out, size_t out_capacity, int device_out, const Fbank& f,
                       const float* window, const float* matrix, const FbankCond& c, uint64_t* n_frames, uint64_t* offsets,
                       uint64_t* total, const char** why)
{
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (total) *total = 0;
    if (n_clips == 0) return FVAD_OK;
    if (!feat_args_ok(d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, out, device_out, window, matrix, why)) return FVAD_ERR_INVALID_ARGUMENT;
    if (!fbank_frames_ok(f, why)) return FVAD_ERR_INVALID_ARGUMENT;
    uint64_t at = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t* r = clips + i * FVAD_CLIP_FIELDS;
        const uint64_t slot = at;
        uint64_t T;
        if (!fbank_slot(f.step, f.skips, f.win_length, f.hop, f.n_mels, i, r[3] - r[2], &at, &T, why)) return FVAD_ERR_INVALID_ARGUMENT;
        if (offsets) offsets[i] = slot;
        if (n_frames) n_frames[i] = T;
    }
    if (total) *total = at;
    for (uint32_t i = 0; i < f.win_length; ++i)
        if (!mel_finite(window[i])) { *why = "a window value that is not finite"; return FVAD_ERR_INVALID_ARGUMENT; }
    for (size_t i = 0; i < (size_t)f.n_mels * (f.n_fft / 2 + 1); ++i)
        if (!mel_finite(matrix[i])) { *why = "a matrix value that is not finite"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (!mel_finite(c.scale) || c.scale == 0.0f) { *why = "a scale that is not finite and non-zero"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (!mel_finite(c.preemph) || !(c.preemph >= 0.0f) || !(c.preemph <= 1.0f)) { *why = "a preemph that is not in 0..1"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (c.remove_dc != 0 && c.remove_dc != 1) { *why = "remove_dc is not 0 or 1"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (!mel_finite(c.floor) || !(c.floor > 0.0f)) { *why = "a floor that is not finite and positive"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (c.cmn != 0 && c.cmn != 1) { *why = "cmn is not 0 or 1"; return FVAD_ERR_INVALID_ARGUMENT; }
    if (const int rc = feat_range_ok(n_lanes, n_samples, clips, n_clips, why)) return rc;
    if (at > out_capacity) { *why = "out_capacity is below fvad_clips_plan_fbank's total"; return FVAD_ERR_BUFFER_TOO_SMALL; }
    const auto frames = [&](size_t i) {
        const uint64_t* r = clips + i * FVAD_CLIP_FIELDS;
        const uint64_t rest = r[3] - r[2] - (f.skips ? f.skips[i] : 0);
        return fbank_frames(rest / f.step + (rest % f.step != 0), f.win_length, f.hop);
    };
    if (!feat_grids_ok(clips, n_clips, frames, fbank_tile_frames(f.win_length, f.hop), why)) return FVAD_ERR_INVALID_ARGUMENT;
    return FVAD_OK;
}

} // namespace fvad
