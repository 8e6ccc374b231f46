// egress_strided.h -- the rules of the strided resampling egress (fvad_egress_resample_strided*), host only: the step and the
// lane span of a row's given frames.  The tile, the ready count, the ratio, the window and the tap rules are egress_resample.h's
// and resample.h's, counted in strided samples.  Inline, so that host_egress_strided.cpp (the check) still builds alone
// (tests/sanitize/egress_strided_san.cpp).
#pragma once
#include "egress_resample.h"

namespace fvad {

constexpr uint32_t kEgressStepMax = 16; // FVAD_EGRESS_STEP_MAX (host_egress_strided.cpp asserts it)

inline bool egress_step_ok(uint32_t step) { return step >= 1 && step <= kEgressStepMax; }

// The n_frames strided samples from src_offset on lie inside a lane of n_samples: the last of them, src_offset +
// (n_frames - 1) step, is below n_samples.  Without wrapping (128-bit); no frames touch no sample.
inline bool egress_strided_span_ok(uint64_t src_offset, uint64_t n_frames, uint32_t step, uint64_t n_samples)
{
    return n_frames == 0 || (u128)src_offset + (u128)(n_frames - 1) * step + 1 <= (u128)n_samples;
}

} // namespace fvad
