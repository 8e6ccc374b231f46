// feature_frames.h -- how a feature clip export (fvad_clips_export_mel*, fvad_clips_export_fbank*) cuts a clip into frames, once
// for the host rules (clips_features.h), the engine (engine_clips.cpp) and the kernels (kernels_clips_mel.hip): the stream's
// length, the frame count of a stream under either framing, and the frames of a tile.  No HIP includes: constexpr functions are
// callable on both sides.  The integer type is the caller's (uint64_t on the host, the kernels' long long).
//   centred (the log-mel export):      T = L / hop,                         frames of n_fft taps, n_fft / 2 of padding in front
//   snip-edges (the filter-bank one):  T = 1 + (L - win) / hop for L >= win, frames of win taps, no padding (no frame below win)
#pragma once
#include <cstdint>

namespace fvad {

constexpr uint32_t kFeatSrcTile = 8192;  // the samples a tile stages: kClipTile of kernels.h, which asserts it
constexpr uint32_t kFeatTileFrames = 32; // four wavefronts of eight frames in the 400-point form

// the stream s[i] = sample skip + i * step of a clip of `len` > skip samples: L = ceil((len - skip) / step)
template <typename I> constexpr I feat_stream_len(I len, I skip, I step) { return (len - skip - 1) / step + 1; }

// the frames of a stream of L samples; snip: of L >= taps samples (a shorter stream has none: the rules refuse it)
template <typename I> constexpr I feat_frames(bool snip, I L, I taps, I hop) { return snip ? 1 + (L - taps) / hop : L / hop; }

// the samples in front of stream sample t * hop that frame t starts at
template <typename I> constexpr I feat_pad(bool snip, I taps) { return snip ? 0 : taps / 2; }

// frames of one tile: as many as the staged window (F - 1) hop + taps <= kFeatSrcTile allows, at most kFeatTileFrames
constexpr uint32_t feat_tile_frames(uint32_t taps, uint32_t hop)
{
    return (kFeatSrcTile - taps) / hop + 1 < kFeatTileFrames ? (kFeatSrcTile - taps) / hop + 1 : kFeatTileFrames;
}

} // namespace fvad
