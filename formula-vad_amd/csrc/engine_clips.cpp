// engine_clips.cpp -- the batch Recorder: fvad_clips_plan / _from_segments (host only) and fvad_clips_export(_device), which
// run kernels_clips.hip over device-resident lanes.  The reference finalises one AudioBuffer per completed segment, the quietest
// channel over [sample_from, sample_to) (Recorder.zig:74-164); here every clip of a call is picked and packed in three launches
// and only the packed clips leave the device.  The strided forms (fvad_clips_export_strided*) are the same calls with the strided
// rules and slots (clips_strided.h) and kernels_clips_strided.hip's gather over tiles of its own; the filtered forms
// (fvad_clips_export_fir*) are the strided calls with the tap rules (clips_fir.h) and kernels_clips_fir.hip's gather; the
// resampled forms (fvad_clips_export_resampled*) are the full-rate calls with the ratio and tap rules and the slots of
// clips_resample.h and kernels_clips_resample.hip's gather.
#include <vector>

#include "clips_fir.h"
#include "clips_resample.h"
#include "clips_strided.h"
#include "internal.h"

using namespace fvad;

static_assert(kStridedSrcTile == (uint64_t)kClipTile && FVAD_CLIP_STEP_MAX == kClipStepMax, "clips_strided.h counts the kernels' tiles");
static_assert(kFirSrcTile == (uint64_t)kClipTile && FVAD_CLIP_FIR_TAPS_MAX == kClipFirTapsMax, "clips_fir.h counts the kernels' tiles");
static_assert(kResampledWindow == (uint64_t)kClipTile, "clips_resample.h counts the kernels' window");

namespace {

bool format_ok(int f) { return f == FVAD_CLIP_F32 || f == FVAD_CLIP_PCM16; }
size_t format_bytes(int f) { return f == FVAD_CLIP_PCM16 ? 2 : 4; }

struct ClipRow { uint64_t first_lane, n_channels, sample_from, sample_to; };
ClipRow row(const uint64_t* clips, size_t i)
{
    const uint64_t* r = clips + i * FVAD_CLIP_FIELDS;
    return {r[0], r[1], r[2], r[3]};
}

// the argument rules of fvad_clips_plan, shared with the export: every slot starts on a 16-byte boundary
int plan_clips(const uint64_t* clips, size_t n, int out_format, uint64_t* offsets, uint64_t* total)
{
    const uint64_t per16 = 16 / format_bytes(out_format);
    uint64_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        const ClipRow c = row(clips, i);
        if (c.sample_to <= c.sample_from || c.n_channels == 0) return FVAD_ERR_INVALID_ARGUMENT;
        if (offsets) offsets[i] = at;
        const uint64_t len = c.sample_to - c.sample_from;
        if (len > UINT64_MAX - at - per16) return FVAD_ERR_INVALID_ARGUMENT; // (the total would not fit 64 bits)
        at += (len + per16 - 1) / per16 * per16;
    }
    if (total) *total = at;
    return FVAD_OK;
}

// Every rule of fvad_clips_export(_device), in one order for both forms: arguments, then every clip's own rules, then its range
// and lanes, then the capacity.  Fills offsets and total.  strided (may be NULL): the strided exports' rules directly after the
// clips' own, and their slots in place of the full-rate ones.  fir (may be NULL, with strided only): the tap rules after those.
// rs (may be NULL, without strided): the resampled exports' ratio and tap rules in the same place, and their slots.
int check_export(const fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                 const uint64_t* clips, size_t n_clips, int out_format, const void* out, size_t out_capacity, bool device_out,
                 std::vector<uint64_t>& offsets, uint64_t& total, const Strided* strided, const Fir* fir, const Resampled* rs)
{
    if (!d_src || !clips || !out) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: NULL argument");
    if (!format_ok(src_format) || !format_ok(out_format)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: unknown sample format");
    if (device_out && (uintptr_t)out % 16 != 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: the output must be 16-byte aligned");
    if ((uintptr_t)d_src % format_bytes(src_format) != 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: the source is not aligned to its samples");
    if (n_lanes > 1 && lane_stride < n_samples) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: lane_stride < n_samples");
    offsets.resize(n_clips);
    if (plan_clips(clips, n_clips, out_format, offsets.data(), &total) != FVAD_OK)
        return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: a clip with sample_to <= sample_from or no channels");
    if (strided) {
        if (!strided_step_ok(strided->step)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export_strided: a step of 0 or above FVAD_CLIP_STEP_MAX");
        const char* why = "";
        total = 0;
        for (size_t i = 0; i < n_clips; ++i) {
            const ClipRow c = row(clips, i);
            uint64_t out_len;
            offsets[i] = total;
            if (!strided_slot(*strided, i, c.sample_to - c.sample_from, 16 / format_bytes(out_format), &total, &out_len, &why))
                return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, std::string("fvad_clips_export_strided: ") + why);
        }
        if (fir && !fir_taps_ok(*fir, &why)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, std::string("fvad_clips_export_fir: ") + why);
    }
    if (rs) {
        const char* why = "";
        if (!resampled_ok(*rs, &why)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, std::string("fvad_clips_export_resampled: ") + why);
        total = 0;
        for (size_t i = 0; i < n_clips; ++i) {
            const ClipRow c = row(clips, i);
            uint64_t out_len;
            offsets[i] = total;
            if ((u128)(c.sample_to - c.sample_from) * rs->up >= (u128)kResampleFramesUp)
                return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export_resampled: a clip of 2^62 / up samples or more");
            if (!resampled_slot(Ratio{rs->up, rs->down}, c.sample_to - c.sample_from, 16 / format_bytes(out_format), &total, &out_len, &why))
                return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, std::string("fvad_clips_export_resampled: ") + why);
        }
    }
    for (size_t i = 0; i < n_clips; ++i) {
        const ClipRow c = row(clips, i);
        if (c.sample_to > n_samples) return set_err(ctx, FVAD_ERR_OUT_OF_RANGE, "fvad_clips_export: a clip ends past n_samples");
        if (c.first_lane >= n_lanes || c.n_channels > n_lanes - c.first_lane)
            return set_err(ctx, FVAD_ERR_OUT_OF_RANGE, "fvad_clips_export: a clip's lanes end past n_lanes");
    }
    if (total > out_capacity) return set_err(ctx, FVAD_ERR_BUFFER_TOO_SMALL, "fvad_clips_export: out_capacity is below fvad_clips_plan's total");
    return FVAD_OK;
}

int export_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                  const uint64_t* clips, size_t n_clips, int out_format, void* d_out, size_t out_capacity, int32_t* best_channel,
                  float* best_rms, float* runner_up_rms, uint64_t* out_offsets, const Strided* strided, const Fir* fir, const Resampled* rs = nullptr);
int export_host(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity, int32_t* best_channel,
                float* best_rms, float* runner_up_rms, uint64_t* out_offsets, const Strided* strided, const Fir* fir, const Resampled* rs = nullptr);

} // namespace

extern "C" {

int fvad_clips_plan(const uint64_t* clips, size_t n_clips, int out_format, uint64_t* offsets, uint64_t* total)
{
    if (!format_ok(out_format) || !total || (n_clips && (!clips || !offsets))) return FVAD_ERR_INVALID_ARGUMENT;
    return plan_clips(clips, n_clips, out_format, offsets, total);
}

int fvad_clips_from_segments(const fvad_speech_segment* segs, size_t n_segs, uint32_t first_lane, uint32_t n_channels,
                             uint64_t n_available, uint64_t* clips, size_t cap, size_t* n_out, size_t* n_skipped)
{
    if (!n_out || !n_skipped || (n_segs && !segs) || (cap && !clips) || n_channels == 0) return FVAD_ERR_INVALID_ARGUMENT;
    size_t n = 0, skipped = 0;
    for (size_t i = 0; i < n_segs; ++i) {
        if (segs[i].sample_to <= segs[i].sample_from) return FVAD_ERR_INVALID_ARGUMENT;
        // Recorder.finalize never runs for a recording whose end the stream does not reach (MRBRecorder.zig:160-192)
        if (segs[i].sample_to > n_available) { ++skipped; continue; }
        if (n < cap) {
            uint64_t* r = clips + n * FVAD_CLIP_FIELDS;
            r[0] = first_lane;
            r[1] = n_channels;
            r[2] = segs[i].sample_from;
            r[3] = segs[i].sample_to;
        }
        ++n;
    }
    *n_out = n;
    *n_skipped = skipped;
    return n > cap ? FVAD_ERR_BUFFER_TOO_SMALL : FVAD_OK;
}

int fvad_clips_export_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride,
                             size_t n_samples, const uint64_t* clips, size_t n_clips, int out_format, void* d_out,
                             size_t out_capacity, int32_t* best_channel, float* best_rms, float* runner_up_rms,
                             uint64_t* out_offsets)
{
    return export_device(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, d_out, out_capacity,
                         best_channel, best_rms, runner_up_rms, out_offsets, nullptr, nullptr);
}

int fvad_clips_export(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                      const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity,
                      int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets)
{
    return export_host(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, out, out_capacity, best_channel,
                       best_rms, runner_up_rms, out_offsets, nullptr, nullptr);
}

int fvad_clips_export_strided_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride,
                                     size_t n_samples, const uint64_t* clips, size_t n_clips, int out_format, void* d_out,
                                     size_t out_capacity, int32_t* best_channel, float* best_rms, float* runner_up_rms,
                                     uint64_t* out_offsets, uint32_t step, const uint32_t* skips)
{
    const Strided s{step, skips};
    return export_device(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, d_out, out_capacity,
                         best_channel, best_rms, runner_up_rms, out_offsets, &s, nullptr);
}

int fvad_clips_export_strided(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                              const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity,
                              int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step,
                              const uint32_t* skips)
{
    const Strided s{step, skips};
    return export_host(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, out, out_capacity, best_channel,
                       best_rms, runner_up_rms, out_offsets, &s, nullptr);
}

int fvad_clips_export_fir_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                 const uint64_t* clips, size_t n_clips, int out_format, void* d_out, size_t out_capacity,
                                 int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step,
                                 const uint32_t* skips, const float* taps, uint32_t n_taps)
{
    const Strided s{step, skips};
    const Fir f{taps, n_taps};
    return export_device(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, d_out, out_capacity,
                         best_channel, best_rms, runner_up_rms, out_offsets, &s, &f);
}

int fvad_clips_export_fir(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                          const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity, int32_t* best_channel,
                          float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step, const uint32_t* skips,
                          const float* taps, uint32_t n_taps)
{
    const Strided s{step, skips};
    const Fir f{taps, n_taps};
    return export_host(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, out, out_capacity, best_channel,
                       best_rms, runner_up_rms, out_offsets, &s, &f);
}

int fvad_clips_export_resampled_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride,
                                       size_t n_samples, const uint64_t* clips, size_t n_clips, int out_format, void* d_out,
                                       size_t out_capacity, int32_t* best_channel, float* best_rms, float* runner_up_rms,
                                       uint64_t* out_offsets, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps)
{
    const Resampled r{up, down, taps, n_taps};
    return export_device(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, d_out, out_capacity,
                         best_channel, best_rms, runner_up_rms, out_offsets, nullptr, nullptr, &r);
}

int fvad_clips_export_resampled(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity,
                                int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t up,
                                uint32_t down, const float* taps, uint32_t n_taps)
{
    const Resampled r{up, down, taps, n_taps};
    return export_host(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, out, out_capacity, best_channel,
                       best_rms, runner_up_rms, out_offsets, nullptr, nullptr, &r);
}

} // extern "C"

namespace {

// fvad_clips_export_device (strided NULL), fvad_clips_export_strided_device, fvad_clips_export_fir_device (fir not NULL) and
// fvad_clips_export_resampled_device (rs not NULL, strided NULL)
int export_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                  const uint64_t* clips, size_t n_clips, int out_format, void* d_out, size_t out_capacity, int32_t* best_channel,
                  float* best_rms, float* runner_up_rms, uint64_t* out_offsets, const Strided* strided, const Fir* fir, const Resampled* rs)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_clips == 0) return FVAD_OK;
    std::vector<uint64_t> offsets;
    uint64_t total = 0;
    const int bad = check_export(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, d_out, out_capacity,
                                 true, offsets, total, strided, fir, rs);
    if (bad != FVAD_OK) return bad;
    // a step of 1 keeps every sample: the full-rate gather, whose tiles are the strided gather's
    const uint32_t step = strided ? strided->step : 1;
    const uint64_t tile_out = rs ? resampled_tile_out(Ratio{rs->up, rs->down}, rs->n_taps) : fir ? clip_fir_tile_out(step, fir->n_taps) : clip_tile_out(step);
    // the tables: one job per clip and the two prefix tables the workgroups search
    std::vector<ClipJob> jobs(n_clips);
    std::vector<uint32_t> unit_prefix(n_clips + 1), tile_prefix(n_clips + 1);
    uint64_t units = 0, tiles = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const ClipRow c = row(clips, i);
        const uint64_t len = c.sample_to - c.sample_from;
        const uint64_t nt = (len + kClipTile - 1) / kClipTile;
        const uint32_t skip = strided && strided->skips ? strided->skips[i] : 0;
        const uint64_t out_len = rs ? resample_out_frames(len, Ratio{rs->up, rs->down}) : (len - skip + step - 1) / step;
        unit_prefix[i] = (uint32_t)units;
        tile_prefix[i] = (uint32_t)tiles;
        ClipJob& j = jobs[i];
        j.src_off = c.first_lane * (uint64_t)lane_stride + c.sample_from;
        j.len = len;
        j.out_off = offsets[i];
        j.first_unit = (uint32_t)units;
        j.n_tiles = (uint32_t)nt;
        j.n_channels = (uint32_t)c.n_channels;
        j.skip = skip;
        units += nt * c.n_channels;
        tiles += (out_len + tile_out - 1) / tile_out; // (step 1: nt)
        if (units > 0x7fffffffull || tiles > 0x7fffffffull) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: more than 2^31 tiles in one call: export in batches");
    }
    unit_prefix[n_clips] = (uint32_t)units;
    tile_prefix[n_clips] = (uint32_t)tiles;

    hipSetDevice(ctx->device);
    // one allocation for the call's tables, every part 16-byte aligned
    auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t o_jobs = 0, o_up = o_jobs + up16(n_clips * sizeof(ClipJob)), o_tp = o_up + up16((n_clips + 1) * 4),
                 o_part = o_tp + up16((n_clips + 1) * 4), o_info = o_part + up16(units * sizeof(double)),
                 o_taps = o_info + up16(n_clips * sizeof(ClipInfo)), bytes = o_taps + up16(rs ? (size_t)resample_phase_taps(rs->up, rs->n_taps) * rs->up * sizeof(float) : fir ? fir->n_taps * sizeof(float) : 0);
    // the taps as the gather walks them: branch by branch (fir) or [j][o mod up] (resampled)
    const std::vector<float> taps = rs ? resample_table(Taps{rs->taps, rs->n_taps}, Ratio{rs->up, rs->down}) : fir ? fir_branches(*fir, step) : std::vector<float>();
    char* d = nullptr;
    if (hipMalloc((void**)&d, bytes) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "fvad_clips_export: hipMalloc of the clip tables failed"); }
    std::vector<ClipInfo> infos(n_clips);
    auto run = [&]() -> int {
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_jobs, jobs.data(), n_clips * sizeof(ClipJob), hipMemcpyHostToDevice, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_up, unit_prefix.data(), (n_clips + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_tp, tile_prefix.data(), (n_clips + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        if (fir || rs) FVAD_HIP(ctx, hipMemcpyAsync(d + o_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        ClipArgs a{};
        a.src = d_src;
        a.out = d_out;
        a.lane_stride = lane_stride;
        a.jobs = reinterpret_cast<const ClipJob*>(d + o_jobs);
        a.unit_prefix = reinterpret_cast<const uint32_t*>(d + o_up);
        a.tile_prefix = reinterpret_cast<const uint32_t*>(d + o_tp);
        a.partials = reinterpret_cast<double*>(d + o_part);
        a.infos = reinterpret_cast<ClipInfo*>(d + o_info);
        a.n_clips = (uint32_t)n_clips;
        a.n_units = (uint32_t)units;
        a.n_tiles = (uint32_t)tiles;
        a.src_i16 = src_format == FVAD_CLIP_PCM16;
        a.out_i16 = out_format == FVAD_CLIP_PCM16;
        time_begin(ctx, "clip_rms");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_rms(a, ctx->stream));
        time_end(ctx);
        time_begin(ctx, "clip_pick");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_pick(a, ctx->stream));
        time_end(ctx);
        if (rs) {
            time_begin(ctx, "clip_gather_resampled");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_gather_resampled(ClipResampleArgs{a, reinterpret_cast<const float*>(d + o_taps), rs->up, rs->down, (uint32_t)tile_out, rs->n_taps}, ctx->stream));
        } else if (fir) {
            time_begin(ctx, "clip_gather_fir");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_gather_fir(ClipFirArgs{a, reinterpret_cast<const float*>(d + o_taps), step, (uint32_t)tile_out, fir->n_taps, 0}, ctx->stream));
        } else if (step == 1) {
            time_begin(ctx, "clip_gather");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_gather(a, ctx->stream));
        } else {
            time_begin(ctx, "clip_gather_strided");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_gather_strided(ClipStridedArgs{a, step, (uint32_t)tile_out}, ctx->stream));
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

// fvad_clips_export (strided NULL), fvad_clips_export_strided, fvad_clips_export_fir (fir not NULL) and
// fvad_clips_export_resampled (rs not NULL, strided NULL)
int export_host(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity, int32_t* best_channel,
                float* best_rms, float* runner_up_rms, uint64_t* out_offsets, const Strided* strided, const Fir* fir, const Resampled* rs)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_clips == 0) return FVAD_OK;
    std::vector<uint64_t> offsets;
    uint64_t total = 0;
    const int bad = check_export(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, out, out_capacity,
                                 false, offsets, total, strided, fir, rs);
    if (bad != FVAD_OK) return bad;
    // a device staging buffer of the plan's size, one copy back, then freed (hipMalloc returns 256-byte aligned memory)
    hipSetDevice(ctx->device);
    const size_t bytes = (size_t)total * format_bytes(out_format);
    void* d_out = nullptr;
    if (hipMalloc(&d_out, bytes) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "fvad_clips_export: hipMalloc of the staging buffer failed"); }
    // the padding between slots is never written by the kernels: zero it, so that the host gets no stale device memory
    hipError_t e = hipMemsetAsync(d_out, 0, bytes, ctx->stream);
    int rc = e == hipSuccess ? export_device(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, d_out,
                                             (size_t)total, best_channel, best_rms, runner_up_rms, out_offsets, strided, fir, rs)
                             : hip_fail(ctx, e, "fvad_clips_export: hipMemsetAsync");
    if (rc == FVAD_OK) {
        e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = hip_fail(ctx, e, "fvad_clips_export: copy back");
    }
    hipFree(d_out);
    return rc;
}

} // namespace
