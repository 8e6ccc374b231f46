// host_clips_strided.cpp -- fvad_clips_phase_skips and fvad_clips_plan_strided: which samples a strided clip export keeps and where
// they go, without a device (plain C++: tests/sanitize/clips_stride_san.cpp builds this file alone).
#include "clips_strided.h"

using namespace fvad;

extern "C" {

int fvad_clips_phase_skips(const uint64_t* sample_from, size_t n_clips, uint32_t step, uint32_t phase, uint32_t* skips)
{
    if (!strided_step_ok(step) || phase >= step || (n_clips && (!sample_from || !skips))) return FVAD_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n_clips; ++i) skips[i] = (uint32_t)((phase + step - sample_from[i] % step) % step);
    return FVAD_OK;
}

int fvad_clips_plan_strided(const uint64_t* lens, const uint32_t* skips, size_t n_clips, uint32_t step, int out_format,
                            uint64_t* out_lens, uint64_t* offsets, uint64_t* total)
{
    if ((out_format != FVAD_CLIP_F32 && out_format != FVAD_CLIP_PCM16) || !total || (n_clips && (!lens || !out_lens || !offsets)))
        return FVAD_ERR_INVALID_ARGUMENT;
    if (!strided_step_ok(step)) return FVAD_ERR_INVALID_ARGUMENT;
    const uint64_t per16 = out_format == FVAD_CLIP_PCM16 ? 8 : 4;
    const Strided s{step, skips};
    const char* why;
    uint64_t at = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t slot = at;
        if (!strided_slot(s, i, lens[i], per16, &at, &out_lens[i], &why)) return FVAD_ERR_INVALID_ARGUMENT;
        offsets[i] = slot;
    }
    *total = at;
    return FVAD_OK;
}

} // extern "C"
