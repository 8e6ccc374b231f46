// clips_resample.h -- the rules of a resampled clip export (fvad_clips_resample_check, fvad_clips_resample_tile,
// fvad_clips_plan_resampled, fvad_clips_export*_resampled), host only: the ratio, the taps, a clip's slot and the gather's tile.
// The ratio, the output count, the tap rules and the [j][o mod up] table are resample.h's.  Inline, so that
// host_clips_resample.cpp, host_clips_split.cpp and engine_clips.cpp state them once and each of the host files still builds alone.
#pragma once
#include "resample.h"

namespace fvad {

constexpr uint64_t kResampledWindow = 8192;  // the clip samples a tile stages at most: kClipTile of kernels.h (engine_clips.cpp asserts it)
constexpr uint64_t kResampledTileMax = 8192; // outputs per tile at most

struct Resampled { uint32_t up, down; const float* taps; uint32_t n_taps; }; // taps in host memory

// The gather's tile in output samples (clip_resampled_tile_out of kernels.h): the most outputs, a multiple of 8 so that a tile's
// first output is on a 16-byte boundary of its slot, whose window floor(((n - 1) down + 2 K) / up) + 1 fits kResampledWindow;
// 0 when not even 8 do.  (n - 1) down + 2 K < kResampledWindow * FVAD_RESAMPLE_UP_MAX < 2^23: the kernel's tile-relative
// induction is 32-bit.
inline uint64_t resampled_tile_out(const Ratio& r, uint32_t n_taps)
{
    return resample_fit(r, n_taps, 1, kResampledWindow, kResampledTileMax) / 8 * 8;
}

// false: *why says which rule (the ratio's, then the taps', then the tile's)
inline bool resampled_ok(const Resampled& f, const char** why)
{
    if (!ratio_ok(Ratio{f.up, f.down})) { *why = "a ratio with up == 0, up above FVAD_RESAMPLE_UP_MAX or down == 0"; return false; }
    if (!resample_taps_ok(Taps{f.taps, f.n_taps}, why)) return false;
    if (resampled_tile_out(Ratio{f.up, f.down}, f.n_taps) == 0) { *why = "the window of 8 outputs does not fit a tile"; return false; }
    return true;
}

// clip of `len` samples: *out_len = ceil(len up / down) and its slot at *at, which moves on to the next 16-byte boundary behind
// the slot (per16 = samples of the output format in 16 bytes).  false: *why says which rule
inline bool resampled_slot(const Ratio& r, uint64_t len, uint64_t per16, uint64_t* at, uint64_t* out_len, const char** why)
{
    if (len == 0) { *why = "a clip of no samples"; return false; }
    const uint64_t n = resample_out_frames(len, r); // (saturated at UINT64_MAX: refused below)
    if (*at > UINT64_MAX - per16 || n > UINT64_MAX - per16 - *at) { *why = "the clips' total does not fit 64 bits"; return false; }
    *out_len = n;
    *at += (n + per16 - 1) / per16 * per16;
    return true;
}

} // namespace fvad
