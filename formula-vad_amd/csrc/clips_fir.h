// clips_fir.h -- the rules of a filtered clip export (fvad_clips_fir_check, fvad_clips_export*_fir), host only: the taps and the
// gather's tile.  Inline, so that host_clips_fir.cpp, host_clips_split.cpp and engine_clips.cpp state them once and each of the
// host files still builds alone.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/fvad.h"

namespace fvad {

constexpr uint64_t kFirSrcTile = 8192; // kClipTile of kernels.h (engine_clips.cpp asserts it)

struct Fir { const float* taps; uint32_t n_taps; }; // host memory

// the filtered gathers' tile in output samples (clip_fir_tile_out of kernels.h): its (tile - 1) * step + 1 + 2 H source samples,
// the zero extension included, fit kFirSrcTile, and a tile's first output is on a 16-byte boundary of its slot
inline uint64_t fir_tile_out(uint32_t step, uint32_t n_taps) { return ((kFirSrcTile - n_taps) / step + 1) / 8 * 8; }

// false: *why says which rule
inline bool fir_taps_ok(const Fir& f, const char** why)
{
    if (!f.taps) { *why = "NULL taps"; return false; }
    if (f.n_taps == 0 || f.n_taps % 2 == 0) { *why = "n_taps is 0 or even"; return false; }
    if (f.n_taps > FVAD_CLIP_FIR_TAPS_MAX) { *why = "n_taps above FVAD_CLIP_FIR_TAPS_MAX"; return false; }
    for (uint32_t k = 0; k < f.n_taps; ++k)
        if (!std::isfinite(f.taps[k])) { *why = "a tap that is not finite"; return false; }
    return true;
}

// the taps as the kernels walk them, branch by branch: taps[j], taps[j + step], ... for j = 0 .. step - 1
inline std::vector<float> fir_branches(const Fir& f, uint32_t step)
{
    std::vector<float> t;
    t.reserve(f.n_taps);
    for (uint32_t j = 0; j < step; ++j)
        for (uint32_t k = j; k < f.n_taps; k += step) t.push_back(f.taps[k]);
    return t;
}

} // namespace fvad
