// host_egress_strided.cpp -- the host-only half of the strided resampling egress (fvad_egress_resample_strided*, the strided
// entries of engine_egress.cpp): fvad_egress_resample_strided_check, every argument rule of the device calls.  The tile and the
// ready count are fvad_egress_resample_tile's and fvad_egress_resample_ready's as they are.  Plain C++ without HIP headers, like
// host_egress_resample.cpp (tests/sanitize/egress_strided_san.cpp builds this file, host_egress_resample.cpp and
// host_resample.cpp alone).
#include "egress_strided.h"

using namespace fvad;

static_assert(kEgressStepMax == FVAD_EGRESS_STEP_MAX, "egress_strided.h restates fvad.h's step");

extern "C" {

// fvad_egress_resample_check's rules in its order (egress_resample_check of host_egress_resample.cpp), with two changes: the
// step's rule directly behind the ratio's, and the given frames' lane range counted `src_step` apart.
int fvad_egress_resample_strided_check(const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, uint32_t up, uint32_t down, const float* taps,
                                       uint32_t n_taps, uint32_t src_step, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    return egress_resample_check(sinks, n_sinks, out_bytes, up, down, taps, n_taps, true, src_step, src_format, n_lanes, lane_stride, n_samples);
}

} // extern "C"
