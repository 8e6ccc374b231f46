// egress_resample.h -- the rules of the resampling egress (fvad_egress_resample*), host only: the kernel's tile and the outputs
// a stream's leading frames can finish.  The ratio, the output count, the window and the tap rules are resample.h's.  Inline, so
// that host_egress_resample.cpp (the check), engine_egress.cpp (the tables) and, through the job the engine builds,
// kernels_egress_resample.hip state the tile once, and host_egress_resample.cpp still builds alone
// (tests/sanitize/egress_resample_san.cpp).
#pragma once
#include "resample.h"

namespace fvad {

constexpr uint64_t kEgressResampleTileBytes = 16384; // a tile's DESTINATION bytes at most: kIngestTileBytes (drain_tile and the LDS image are the egress's)
constexpr uint64_t kEgressResampleWindow = 8192;     // the lane samples of one channel a tile stages at most: kClipTile (engine_egress.cpp asserts both)

// The kernel's tile in OUTPUT frames: the most frames, a multiple of 4, whose bytes fit kEgressResampleTileBytes and whose
// window of one channel, floor(((n - 1) down + 2 K) / up) + 1 lane samples, fits kEgressResampleWindow; 0 when not even 4 do.
// (n - 1) down + 2 K < kEgressResampleWindow * FVAD_RESAMPLE_UP_MAX < 2^23: the kernel's tile-relative induction is 32-bit.
inline uint64_t egress_resample_tile(const Ratio& r, uint32_t n_taps, uint64_t n_channels, uint64_t format)
{
    const uint64_t most = kEgressResampleTileBytes / (n_channels * sample_bytes_of(format)) / 4 * 4; // >= 64: a frame is at most 256 bytes
    return resample_fit(r, n_taps, 1, kEgressResampleWindow, most);
}

// The leading outputs of a stream of stream_frames lane samples whose whole window lies below frames_have: all of them
// (out_frames) once frames_have >= stream_frames -- the zero extension behind the stream needs no frame --, otherwise the o with
// floor((o down + K) / up) < frames_have, that is o down + K < frames_have up: ceil((frames_have up - K) / down) of them.
inline uint64_t egress_resample_ready(const Ratio& r, uint32_t n_taps, uint64_t stream_frames, uint64_t frames_have)
{
    const uint64_t out_frames = resample_out_frames(stream_frames, r);
    if (frames_have >= stream_frames) return out_frames;
    const u128 K = (n_taps - 1) / 2, have = (u128)frames_have * r.up;
    if (have <= K) return 0;
    const u128 n = (have - K + r.down - 1) / r.down;
    return n < (u128)out_frames ? (uint64_t)n : out_frames;
}

// fvad_egress_resample_check (strided false, step unused) and fvad_egress_resample_strided_check (true, its src_step) in one:
// host_egress_resample.cpp
int egress_resample_check(const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps,
                          bool strided, uint32_t step, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples);

} // namespace fvad
