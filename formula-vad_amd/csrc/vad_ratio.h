// vad_ratio.h -- the volume ratio an FFT frame carries into its VAD machine, from the channels' chunk RMS: the per-chunk ratio
// (BufferedVolumeAnalyzer.zig:48-69) through the two metadata hand-overs that leave a chunk's ratio alone in its result
// (BufferedVolumeAnalyzer.zig:33-45, BufferedDenoiser.zig:83-86,115; VADMetadata.zig:16-60), then the sample-weighted mean over
// the chunks a frame overlaps (BufferedFFT.zig:137-140,153), all in f32 and in chunk order.  Shared by the host
// (sweep_frame_ratios, host_vad.cpp) and the device (kernels_vadratio.hip): the same operations in the same order on both
// sides, so both give the same bits (the library is built with -ffp-contract=off; f32 division and u64 -> f32 conversion are
// correctly rounded on both sides).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vad_machine.h" // FVAD_HD

namespace fvad {

// VADMetadata's ratio of one push (v, weight) into an empty Metadata, as toResult gives it (VADMetadata.zig:16-27,29-43)
FVAD_HD inline float meta_hand_over(float v, float weight)
{
    float ratio_sum = 0.0f, ratio_weight = 0.0f;
    ratio_sum += v * weight;
    ratio_weight += weight;
    return ratio_sum / ratio_weight;
}

// The ratio of one chunk as the buffered FFT stage receives it.  rms(c): channel c's RMS of the chunk.
template <class Rms> FVAD_HD inline float chunk_volume_ratio(Rms rms, size_t n_channels, float chunk_size_f)
{
    float vol_min = 1, vol_max = 0; // BufferedVolumeAnalyzer.zig:52-53
    for (size_t c = 0; c < n_channels; ++c) {
        const float vol = rms(c);
        if (vol < vol_min) vol_min = vol;
        if (vol > vol_max) vol_max = vol;
    }
    const float r = (vol_max == 0) ? 0.0f : vol_min / vol_max;
    return meta_hand_over(meta_hand_over(r, chunk_size_f), chunk_size_f);
}

// The ratio of the frame of fft_size samples that starts at sample `from`: chunk_ratio(k) is chunk k's ratio (k absolute:
// chunk k covers samples [k * chunk_size, (k + 1) * chunk_size)), weighted by the samples of the chunk inside the frame.
template <class ChunkRatio> FVAD_HD inline float frame_volume_ratio(ChunkRatio chunk_ratio, uint64_t from, uint64_t fft_size, uint64_t chunk_size)
{
    const uint64_t to = from + fft_size;
    float ratio_sum = 0.0f, ratio_weight = 0.0f; // VADMetadata.zig:29-43 (every chunk has a ratio)
    for (uint64_t k = from / chunk_size; k * chunk_size < to; ++k) {
        const uint64_t lo = from > k * chunk_size ? from : k * chunk_size;
        const uint64_t hi = to < (k + 1) * chunk_size ? to : (k + 1) * chunk_size;
        const float weight = (float)(hi - lo);
        ratio_sum += chunk_ratio(k) * weight;
        ratio_weight += weight;
    }
    return ratio_sum / ratio_weight;
}

} // namespace fvad
