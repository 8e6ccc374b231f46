// engine_clips_split.cpp -- fvad_clips_export_split(_device): the batch Recorder over a split source (kernels_clips_split.hip).
// The argument rules are fvad_clips_split_check's (host_clips_split.cpp); here are the tables a launch searches -- engine_clips.cpp's,
// plus one ClipSplit per clip -- and the three launches.  The strided forms (fvad_clips_export_split*_strided) are the same calls
// with the strided rules and slots (clips_strided.h) and kernels_clips_strided.hip's gather over tiles of its own; the filtered
// forms (fvad_clips_export_split_fir*) are the strided calls with the tap rules (clips_fir.h) and kernels_clips_fir.hip's gather;
// the resampled forms (fvad_clips_export_split_resampled*) are the full-rate calls with the rules and slots of clips_resample.h
// and kernels_clips_resample.hip's gather.
#include <vector>

#include "clips_fir.h"
#include "clips_resample.h"
#include "clips_split.h"
#include "clips_strided.h"
#include "internal.h"

using namespace fvad;

static_assert(kSplitTile == (uint64_t)kClipTile, "host_clips_split.cpp counts the kernels' tiles");

namespace {

int check_call(const fvad_ctx* ctx, const char* who, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
               size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips, int out_format,
               const void* out, size_t out_capacity, bool device_out, std::vector<uint64_t>& offsets, uint64_t& total,
               const Strided* strided, const Fir* fir, const Resampled* rs)
{
    offsets.resize(n_clips);
    const char* why = "";
    const int rc = clips_split_check(d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips,
                                     out_format, out, out_capacity, device_out, offsets.data(), &total, &why, strided, fir, rs);
    return rc == FVAD_OK ? rc : set_err(ctx, rc, std::string(who) + ": " + why);
}

// fvad_clips_export_split_device (strided NULL), fvad_clips_export_split_strided_device and fvad_clips_export_split_fir_device
// (fir not NULL); fvad_clips_export_split_resampled_device (rs not NULL, strided NULL)
int export_split_device(fvad_ctx* ctx, const char* who, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                        size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips,
                        int out_format, void* d_out, size_t out_capacity, int32_t* best_channel, float* best_rms, float* runner_up_rms,
                        uint64_t* out_offsets, const Strided* strided, const Fir* fir, const Resampled* rs = nullptr)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_clips == 0) return FVAD_OK;
    std::vector<uint64_t> offsets;
    uint64_t total = 0;
    const int bad = check_call(ctx, who, d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips,
                               out_format, d_out, out_capacity, true, offsets, total, strided, fir, rs);
    if (bad != FVAD_OK) return bad;
    // a step of 1 keeps every sample: the full-rate gather, whose tiles are the strided gather's
    const uint32_t step = strided ? strided->step : 1;
    const uint64_t tile_out = rs ? resampled_tile_out(Ratio{rs->up, rs->down}, rs->n_taps) : fir ? clip_fir_tile_out(step, fir->n_taps) : clip_tile_out(step);
    // the tables: engine_clips.cpp's job per clip and prefix tables (the check has bounded the units), and the clips' pieces
    std::vector<ClipJob> jobs(n_clips);
    std::vector<ClipSplit> splits(n_clips);
    std::vector<uint32_t> unit_prefix(n_clips + 1), tile_prefix(n_clips + 1);
    uint64_t units = 0, tiles = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const SplitRow c = split_row(clips, i);
        const uint64_t len = c.a_len + c.b_len;
        const uint64_t nt = (len + kClipTile - 1) / kClipTile;
        const uint32_t skip = strided && strided->skips ? strided->skips[i] : 0;
        const uint64_t out_len = rs ? resample_out_frames(len, Ratio{rs->up, rs->down}) : (len - skip + step - 1) / step;
        unit_prefix[i] = (uint32_t)units;
        tile_prefix[i] = (uint32_t)tiles;
        ClipJob& j = jobs[i];
        j.src_off = 0;
        j.len = len;
        j.out_off = offsets[i];
        j.first_unit = (uint32_t)units;
        j.n_tiles = (uint32_t)nt;
        j.n_channels = (uint32_t)c.n_channels;
        j.skip = skip;
        ClipSplit& s = splits[i];
        s.a_off = c.a_len ? c.a_lane * (uint64_t)a_stride + c.a_from : 0; // (a piece of no samples is never addressed)
        s.a_len = c.a_len;
        s.b_off = c.b_len ? c.b_lane * (uint64_t)b_stride + c.b_from : 0;
        s.pad = 0;
        units += nt * c.n_channels;
        tiles += (out_len + tile_out - 1) / tile_out; // (step 1: nt)
    }
    unit_prefix[n_clips] = (uint32_t)units;
    tile_prefix[n_clips] = (uint32_t)tiles;

    hipSetDevice(ctx->device);
    // one allocation for the call's tables, every part 16-byte aligned
    auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t o_jobs = 0, o_split = o_jobs + up16(n_clips * sizeof(ClipJob)), o_up = o_split + up16(n_clips * sizeof(ClipSplit)),
                 o_tp = o_up + up16((n_clips + 1) * 4), o_part = o_tp + up16((n_clips + 1) * 4),
                 o_info = o_part + up16(units * sizeof(double)), o_taps = o_info + up16(n_clips * sizeof(ClipInfo)),
                 bytes = o_taps + up16(rs ? (size_t)resample_phase_taps(rs->up, rs->n_taps) * rs->up * sizeof(float) : fir ? fir->n_taps * sizeof(float) : 0);
    // the taps as the gather walks them: branch by branch (fir) or [j][o mod up] (resampled)
    const std::vector<float> taps = rs ? resample_table(Taps{rs->taps, rs->n_taps}, Ratio{rs->up, rs->down}) : fir ? fir_branches(*fir, step) : std::vector<float>();
    char* d = nullptr;
    if (hipMalloc((void**)&d, bytes) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, std::string(who) + ": hipMalloc of the clip tables failed"); }
    std::vector<ClipInfo> infos(n_clips);
    auto run = [&]() -> int {
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_jobs, jobs.data(), n_clips * sizeof(ClipJob), hipMemcpyHostToDevice, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_split, splits.data(), n_clips * sizeof(ClipSplit), hipMemcpyHostToDevice, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_up, unit_prefix.data(), (n_clips + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_tp, tile_prefix.data(), (n_clips + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        if (fir || rs) FVAD_HIP(ctx, hipMemcpyAsync(d + o_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        ClipSplitArgs a{};
        a.c.src = d_a;
        a.c.out = d_out;
        a.c.lane_stride = a_stride;
        a.c.jobs = reinterpret_cast<const ClipJob*>(d + o_jobs);
        a.c.unit_prefix = reinterpret_cast<const uint32_t*>(d + o_up);
        a.c.tile_prefix = reinterpret_cast<const uint32_t*>(d + o_tp);
        a.c.partials = reinterpret_cast<double*>(d + o_part);
        a.c.infos = reinterpret_cast<ClipInfo*>(d + o_info);
        a.c.n_clips = (uint32_t)n_clips;
        a.c.n_units = (uint32_t)units;
        a.c.n_tiles = (uint32_t)tiles;
        a.c.src_i16 = src_format == FVAD_CLIP_PCM16;
        a.c.out_i16 = out_format == FVAD_CLIP_PCM16;
        a.b = d_b;
        a.b_stride = b_stride;
        a.splits = reinterpret_cast<const ClipSplit*>(d + o_split);
        time_begin(ctx, "clip_rms_split");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_rms_split(a, ctx->stream));
        time_end(ctx);
        time_begin(ctx, "clip_pick");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_pick(a.c, ctx->stream));
        time_end(ctx);
        if (rs) {
            time_begin(ctx, "clip_gather_resampled_split");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_gather_resampled_split(ClipSplitResampleArgs{a, reinterpret_cast<const float*>(d + o_taps), rs->up, rs->down, (uint32_t)tile_out, rs->n_taps}, ctx->stream));
        } else if (fir) {
            time_begin(ctx, "clip_gather_fir_split");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_gather_fir_split(ClipSplitFirArgs{a, reinterpret_cast<const float*>(d + o_taps), step, (uint32_t)tile_out, fir->n_taps, 0}, ctx->stream));
        } else if (step == 1) {
            time_begin(ctx, "clip_gather_split");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_gather_split(a, ctx->stream));
        } else {
            time_begin(ctx, "clip_gather_strided_split");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_gather_strided_split(ClipSplitStridedArgs{a, step, (uint32_t)tile_out}, ctx->stream));
        }
        time_end(ctx);
        FVAD_HIP(ctx, hipMemcpyAsync(infos.data(), d + o_info, n_clips * sizeof(ClipInfo), hipMemcpyDeviceToHost, ctx->stream));
        FVAD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FVAD_OK;
    };
    const int rc = run();
    if (rc != FVAD_OK) (void)hipStreamSynchronize(ctx->stream);
    hipFree(d);
    if (rc != FVAD_OK) return rc;
    for (size_t i = 0; i < n_clips; ++i) {
        if (best_channel) best_channel[i] = infos[i].best_channel;
        if (best_rms) best_rms[i] = infos[i].best_rms;
        if (runner_up_rms) runner_up_rms[i] = infos[i].runner_up_rms;
        if (out_offsets) out_offsets[i] = infos[i].out_offset;
    }
    return FVAD_OK;
}

// fvad_clips_export_split (strided NULL), fvad_clips_export_split_strided, fvad_clips_export_split_fir (fir not NULL) and
// fvad_clips_export_split_resampled (rs not NULL, strided NULL)
int export_split_host(fvad_ctx* ctx, const char* who, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                      size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips,
                      int out_format, void* out, size_t out_capacity, int32_t* best_channel, float* best_rms, float* runner_up_rms,
                      uint64_t* out_offsets, const Strided* strided, const Fir* fir, const Resampled* rs = nullptr)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_clips == 0) return FVAD_OK;
    std::vector<uint64_t> offsets;
    uint64_t total = 0;
    const int bad = check_call(ctx, who, d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips,
                               out_format, out, out_capacity, false, offsets, total, strided, fir, rs);
    if (bad != FVAD_OK) return bad;
    // a device staging buffer of the plan's size, one copy back, then freed, as fvad_clips_export does
    hipSetDevice(ctx->device);
    const size_t bytes = (size_t)total * (out_format == FVAD_CLIP_PCM16 ? 2 : 4);
    void* d_out = nullptr;
    if (hipMalloc(&d_out, bytes) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, std::string(who) + ": hipMalloc of the staging buffer failed"); }
    // the padding between slots is never written by the kernels: zero it, so that the host gets no stale device memory
    hipError_t e = hipMemsetAsync(d_out, 0, bytes, ctx->stream);
    int rc = e == hipSuccess ? export_split_device(ctx, who, d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format,
                                                   clips, n_clips, out_format, d_out, (size_t)total, best_channel, best_rms, runner_up_rms,
                                                   out_offsets, strided, fir, rs)
                             : hip_fail(ctx, e, "fvad_clips_export_split: hipMemsetAsync");
    if (rc == FVAD_OK) {
        e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = hip_fail(ctx, e, "fvad_clips_export_split: copy back");
    }
    hipFree(d_out);
    return rc;
}

} // namespace

extern "C" {

int fvad_clips_export_split_device(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                   size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips,
                                   size_t n_clips, int out_format, void* d_out, size_t out_capacity, int32_t* best_channel,
                                   float* best_rms, float* runner_up_rms, uint64_t* out_offsets)
{
    return export_split_device(ctx, "fvad_clips_export_split", d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format,
                               clips, n_clips, out_format, d_out, out_capacity, best_channel, best_rms, runner_up_rms, out_offsets, nullptr, nullptr);
}

int fvad_clips_export_split(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                            size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips,
                            int out_format, void* out, size_t out_capacity, int32_t* best_channel, float* best_rms,
                            float* runner_up_rms, uint64_t* out_offsets)
{
    return export_split_host(ctx, "fvad_clips_export_split", d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format,
                             clips, n_clips, out_format, out, out_capacity, best_channel, best_rms, runner_up_rms, out_offsets, nullptr, nullptr);
}

int fvad_clips_export_split_strided_device(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                           const void* d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                           const uint64_t* clips, size_t n_clips, int out_format, void* d_out, size_t out_capacity,
                                           int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets,
                                           uint32_t step, const uint32_t* skips)
{
    const Strided s{step, skips};
    return export_split_device(ctx, "fvad_clips_export_split_strided", d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples,
                               src_format, clips, n_clips, out_format, d_out, out_capacity, best_channel, best_rms, runner_up_rms, out_offsets, &s, nullptr);
}

int fvad_clips_export_split_strided(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                    size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips,
                                    size_t n_clips, int out_format, void* out, size_t out_capacity, int32_t* best_channel,
                                    float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step, const uint32_t* skips)
{
    const Strided s{step, skips};
    return export_split_host(ctx, "fvad_clips_export_split_strided", d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples,
                             src_format, clips, n_clips, out_format, out, out_capacity, best_channel, best_rms, runner_up_rms, out_offsets, &s, nullptr);
}

int fvad_clips_export_split_fir_device(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                       size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips,
                                       size_t n_clips, int out_format, void* d_out, size_t out_capacity, int32_t* best_channel,
                                       float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step, const uint32_t* skips,
                                       const float* taps, uint32_t n_taps)
{
    const Strided s{step, skips};
    const Fir f{taps, n_taps};
    return export_split_device(ctx, "fvad_clips_export_split_fir", d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples,
                               src_format, clips, n_clips, out_format, d_out, out_capacity, best_channel, best_rms, runner_up_rms, out_offsets, &s, &f);
}

int fvad_clips_export_split_fir(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips,
                                int out_format, void* out, size_t out_capacity, int32_t* best_channel, float* best_rms,
                                float* runner_up_rms, uint64_t* out_offsets, uint32_t step, const uint32_t* skips, const float* taps,
                                uint32_t n_taps)
{
    const Strided s{step, skips};
    const Fir f{taps, n_taps};
    return export_split_host(ctx, "fvad_clips_export_split_fir", d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples,
                             src_format, clips, n_clips, out_format, out, out_capacity, best_channel, best_rms, runner_up_rms, out_offsets, &s, &f);
}

int fvad_clips_export_split_resampled_device(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                             const void* d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                             const uint64_t* clips, size_t n_clips, int out_format, void* d_out, size_t out_capacity,
                                             int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets,
                                             uint32_t up, uint32_t down, const float* taps, uint32_t n_taps)
{
    const Resampled r{up, down, taps, n_taps};
    return export_split_device(ctx, "fvad_clips_export_split_resampled", d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples,
                               src_format, clips, n_clips, out_format, d_out, out_capacity, best_channel, best_rms, runner_up_rms, out_offsets,
                               nullptr, nullptr, &r);
}

int fvad_clips_export_split_resampled(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                      size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips,
                                      size_t n_clips, int out_format, void* out, size_t out_capacity, int32_t* best_channel,
                                      float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t up, uint32_t down,
                                      const float* taps, uint32_t n_taps)
{
    const Resampled r{up, down, taps, n_taps};
    return export_split_host(ctx, "fvad_clips_export_split_resampled", d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples,
                             src_format, clips, n_clips, out_format, out, out_capacity, best_channel, best_rms, runner_up_rms, out_offsets,
                             nullptr, nullptr, &r);
}

} // extern "C"
