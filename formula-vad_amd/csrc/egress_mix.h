// egress_mix.h -- the two-source egress (fvad_egress_mix*): what engine_egress.cpp builds and kernels_egress_mix.hip reads.
// A header of its own, not a part of kernels.h: the translation units of the other egress kernels do not see it.
// A work unit is kernels_egress.hip's: a tile of one sink -- kIngestTileBytes of its DESTINATION bytes rounded down to whole
// frames in multiples of 4 (tile_frames), every channel of them.  Frame f of the sink pairs denoised sample den_off + f with
// original sample orig_off + (f - orig_zeros), +0.0f for f < orig_zeros.  A launch serves the jobs of ONE file format;
// unit_prefix[j] counts the units in front of job j (a job has at least one unit).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct EgressMixJob {
    uint64_t dst_off;    // bytes from `out` to the sink's frame 0
    uint64_t n_frames;
    uint64_t den_off;    // elements from `den` to the denoised sample of frame 0, channel 0
    uint64_t orig_off;   // elements from `orig` to the original sample of frame orig_zeros, channel 0
    uint64_t orig_zeros; // the leading frames whose original sample is +0.0f (may pass n_frames)
    uint32_t tile_frames, n_channels;
};
struct EgressMixArgs {
    const float* orig;   // f32 lanes, orig_stride apart; never dereferenced when w_orig == 0 (may be NULL then)
    const float* den;    // f32 lanes, den_stride apart; never dereferenced when w_den == 0 (may be NULL then)
    uint64_t orig_stride, den_stride;
    uint8_t* out;
    const EgressMixJob* jobs;     // [n_jobs] (device)
    const uint32_t* unit_prefix;  // [n_jobs + 1]
    uint32_t n_jobs, n_units;
    float w_orig, w_den;          // finite, not both zero
    int file_format;              // FVAD_INGEST_*
};
int fvad_launch_egress_mix(const EgressMixArgs& a, hipStream_t stream); // hipError_t as int
