// host_clips_resample.cpp -- fvad_clips_resample_check, fvad_clips_resample_tile and fvad_clips_plan_resampled: the rules, the
// gather's tile and the slots of a resampled clip export, without a device (plain C++: tests/sanitize/clips_resample_san.cpp
// builds this file and host_resample.cpp alone).
#include "clips_resample.h"

using namespace fvad;

extern "C" {

int fvad_clips_resample_check(uint32_t up, uint32_t down, const float* taps, uint32_t n_taps)
{
    const char* why;
    return resampled_ok(Resampled{up, down, taps, n_taps}, &why) ? FVAD_OK : FVAD_ERR_INVALID_ARGUMENT;
}

uint64_t fvad_clips_resample_tile(uint32_t up, uint32_t down, uint32_t n_taps)
{
    if (!ratio_ok(Ratio{up, down}) || n_taps == 0 || n_taps % 2 == 0 || n_taps > FVAD_RESAMPLE_TAPS_MAX) return 0;
    return resampled_tile_out(Ratio{up, down}, n_taps);
}

int fvad_clips_plan_resampled(const uint64_t* lens, size_t n_clips, uint32_t up, uint32_t down, int out_format, uint64_t* out_lens,
                              uint64_t* offsets, uint64_t* total)
{
    if ((out_format != FVAD_CLIP_F32 && out_format != FVAD_CLIP_PCM16) || !total || (n_clips && (!lens || !out_lens || !offsets)))
        return FVAD_ERR_INVALID_ARGUMENT;
    const Ratio q{up, down};
    if (!ratio_ok(q)) return FVAD_ERR_INVALID_ARGUMENT;
    const uint64_t per16 = out_format == FVAD_CLIP_PCM16 ? 8 : 4;
    const char* why;
    uint64_t at = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t slot = at;
        if (!resampled_slot(q, lens[i], per16, &at, &out_lens[i], &why)) return FVAD_ERR_INVALID_ARGUMENT;
        offsets[i] = slot;
    }
    *total = at;
    return FVAD_OK;
}

} // extern "C"
