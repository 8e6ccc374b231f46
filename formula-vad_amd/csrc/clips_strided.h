// clips_strided.h -- the rules of a strided clip export (fvad_clips_plan_strided, fvad_clips_export*_strided), host only: the step,
// a clip's skip and its slot.  Inline, so that host_clips_strided.cpp, host_clips_split.cpp and engine_clips.cpp state them once
// and each of the two host files still builds alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fvad.h"

namespace fvad {

constexpr uint64_t kStridedSrcTile = 8192; // kClipTile of kernels.h (engine_clips.cpp asserts it)
// the strided gathers' tile in output samples: clip_tile_out of kernels.h
inline uint64_t strided_tile_out(uint32_t step) { return kStridedSrcTile / step / 8 * 8; }

struct Strided { uint32_t step; const uint32_t* skips; }; // skips NULL: all zero

inline bool strided_step_ok(uint32_t step) { return step >= 1 && step <= FVAD_CLIP_STEP_MAX; }

// clip i of `len` samples: its skip's rules, *out_len = ceil((len - skip) / step) and its slot at *at, which moves on to the next
// 16-byte boundary behind the slot (per16 = samples of the output format in 16 bytes).  false: *why says which rule
inline bool strided_slot(const Strided& s, size_t i, uint64_t len, uint64_t per16, uint64_t* at, uint64_t* out_len, const char** why)
{
    const uint64_t skip = s.skips ? s.skips[i] : 0;
    if (skip >= s.step) { *why = "a skip that is not below the step"; return false; }
    if (len <= skip) { *why = "a clip that keeps no sample (len <= skip)"; return false; }
    const uint64_t rest = len - skip, n = rest / s.step + (rest % s.step != 0);
    if (*at > UINT64_MAX - per16 || n > UINT64_MAX - per16 - *at) { *why = "the clips' total does not fit 64 bits"; return false; }
    *out_len = n;
    *at += (n + per16 - 1) / per16 * per16;
    return true;
}

} // namespace fvad
