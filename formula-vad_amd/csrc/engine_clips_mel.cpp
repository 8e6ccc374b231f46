// engine_clips_mel.cpp -- fvad_clips_export_mel(_device): log-mel features of the clips of device-resident lanes.  The full-rate
// Recorder's RMS and pick (kernels_clips.hip) over every sample, then kernels_clips_mel.hip's frames over the picked channel's
// strided stream; only [T][n_mels] floats per clip leave the device.  The rules are clips_mel.h's, shared with the host-only
// fvad_clips_mel_check.
#include <cmath>
#include <vector>

#include "clips_mel.h"
#include "internal.h"

using namespace fvad;

static_assert(kMelSrcTile == (uint64_t)kClipTile && kMelTileFrames == (uint64_t)kClipMelTileFrames, "clips_mel.h counts the kernels' tiles");
static_assert(FVAD_CLIP_MEL_NFFT_MAX == kClipMelNfftMax && FVAD_CLIP_MEL_BANDS_MAX == kClipMelBandsMax, "fvad.h states the kernels' limits");

namespace {

struct MelCall {
    Mel m;
    const float* window;
    const float* matrix;
    float floor;
    const float* norm;
};

int mel_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
               const uint64_t* clips, size_t n_clips, int out_format, void* d_out, size_t out_capacity, bool device_out, int32_t* best_channel,
               float* best_rms, float* runner_up_rms, uint64_t* out_offsets, const MelCall& mc, uint64_t* n_frames, float* feat_max)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_clips == 0) return FVAD_OK;
    std::vector<uint64_t> offsets(n_clips), frames(n_clips);
    uint64_t total = 0;
    const char* why = "";
    const int bad = mel_check(d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, d_out, out_capacity, device_out,
                              mc.m, mc.window, mc.matrix, mc.floor, mc.norm, frames.data(), offsets.data(), &total, &why);
    if (bad != FVAD_OK) return set_err(ctx, bad, std::string("fvad_clips_export_mel: ") + why);
    const Mel& m = mc.m;
    const uint32_t tf = clip_mel_tile_frames(m.n_fft, m.hop), n_bins = m.n_fft / 2 + 1;
    // the tables: one job per clip and the two prefix tables the workgroups search (the check counted both grids)
    std::vector<ClipJob> jobs(n_clips);
    std::vector<uint32_t> unit_prefix(n_clips + 1), tile_prefix(n_clips + 1);
    uint64_t units = 0, tiles = 0;
    for (size_t i = 0; i < n_clips; ++i) {
        const uint64_t* r = clips + i * FVAD_CLIP_FIELDS;
        const uint64_t len = r[3] - r[2], nt = (len + kClipTile - 1) / kClipTile;
        unit_prefix[i] = (uint32_t)units;
        tile_prefix[i] = (uint32_t)tiles;
        ClipJob& j = jobs[i];
        j.src_off = r[0] * (uint64_t)lane_stride + r[2];
        j.len = len;
        j.out_off = offsets[i];
        j.first_unit = (uint32_t)units;
        j.n_tiles = (uint32_t)nt;
        j.n_channels = (uint32_t)r[1];
        j.skip = m.skips ? m.skips[i] : 0;
        units += nt * r[1];
        tiles += (frames[i] + tf - 1) / tf;
    }
    unit_prefix[n_clips] = (uint32_t)units;
    tile_prefix[n_clips] = (uint32_t)tiles;
    // the matrix as the kernels read it: [bin][band]
    std::vector<float> matrix_t((size_t)n_bins * m.n_mels);
    for (uint32_t b = 0; b < m.n_mels; ++b)
        for (uint32_t k = 0; k < n_bins; ++k) matrix_t[(size_t)k * m.n_mels + b] = mc.matrix[(size_t)b * n_bins + k];

    hipSetDevice(ctx->device);
    ClipMelArgs a{};
    // the transform's tables (twiddles, un-mixing factors, radices), cached per context and size
    { const int rc = get_vad_plan(ctx, m.n_fft, &a.pl, true); if (rc != FVAD_OK) return rc; }
    auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t o_jobs = 0, o_up = o_jobs + up16(n_clips * sizeof(ClipJob)), o_tp = o_up + up16((n_clips + 1) * 4),
                 o_part = o_tp + up16((n_clips + 1) * 4), o_info = o_part + up16(units * sizeof(double)),
                 o_win = o_info + up16(n_clips * sizeof(ClipInfo)), o_mat = o_win + up16(m.n_fft * sizeof(float)),
                 o_tmax = o_mat + up16(matrix_t.size() * sizeof(float)), o_fmax = o_tmax + up16(tiles * sizeof(float)),
                 bytes = o_fmax + up16(n_clips * sizeof(float));
    char* d = nullptr;
    if (hipMalloc((void**)&d, bytes) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "fvad_clips_export_mel: hipMalloc of the clip tables failed"); }
    std::vector<ClipInfo> infos(n_clips);
    std::vector<float> fmax(n_clips);
    auto run = [&]() -> int {
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_jobs, jobs.data(), n_clips * sizeof(ClipJob), hipMemcpyHostToDevice, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_up, unit_prefix.data(), (n_clips + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_tp, tile_prefix.data(), (n_clips + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_win, mc.window, m.n_fft * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_mat, matrix_t.data(), matrix_t.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        ClipArgs& c = a.c;
        c.src = d_src;
        c.out = d_out;
        c.lane_stride = lane_stride;
        c.jobs = reinterpret_cast<const ClipJob*>(d + o_jobs);
        c.unit_prefix = reinterpret_cast<const uint32_t*>(d + o_up);
        c.tile_prefix = reinterpret_cast<const uint32_t*>(d + o_tp);
        c.partials = reinterpret_cast<double*>(d + o_part);
        c.infos = reinterpret_cast<ClipInfo*>(d + o_info);
        c.n_clips = (uint32_t)n_clips;
        c.n_units = (uint32_t)units;
        c.n_tiles = (uint32_t)tiles;
        c.src_i16 = src_format == FVAD_CLIP_PCM16;
        c.out_i16 = 0;
        a.window = reinterpret_cast<const float*>(d + o_win);
        a.matrix_t = reinterpret_cast<const float*>(d + o_mat);
        a.tile_max = reinterpret_cast<float*>(d + o_tmax);
        a.feat_max = reinterpret_cast<float*>(d + o_fmax);
        a.step = m.step;
        a.hop = m.hop;
        a.n_mels = m.n_mels;
        a.tile_frames = tf;
        a.floor = mc.floor;
        a.log_floor = (float)std::log10((double)mc.floor);
        if (mc.norm) { a.norm_range = mc.norm[0]; a.norm_offset = mc.norm[1]; a.norm_scale = mc.norm[2]; }
        a.fft400 = m.n_fft == 400 && !ctx->tune.clip_mel_generic;
        time_begin(ctx, "clip_rms");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_rms(c, ctx->stream));
        time_end(ctx);
        time_begin(ctx, "clip_pick");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_pick(c, ctx->stream));
        time_end(ctx);
        time_begin(ctx, a.fft400 ? "clip_mel400" : "clip_mel");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_mel(a, ctx->stream));
        time_end(ctx);
        time_begin(ctx, "clip_mel_max");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_mel_max(a, ctx->stream));
        time_end(ctx);
        if (mc.norm) {
            time_begin(ctx, "clip_mel_norm");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_mel_norm(a, ctx->stream));
            time_end(ctx);
        }
        FVAD_HIP(ctx, hipMemcpyAsync(infos.data(), d + o_info, n_clips * sizeof(ClipInfo), hipMemcpyDeviceToHost, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(fmax.data(), d + o_fmax, n_clips * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
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
        if (n_frames) n_frames[i] = frames[i];
        if (feat_max) feat_max[i] = fmax[i];
    }
    return FVAD_OK;
}

} // namespace

extern "C" {

int fvad_clips_export_mel_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                 const uint64_t* clips, size_t n_clips, int out_format, void* d_out, size_t out_capacity,
                                 int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step,
                                 const uint32_t* skips, uint32_t n_fft, uint32_t hop, const float* window, uint32_t n_mels,
                                 const float* matrix, float floor, const float* norm, uint64_t* n_frames, float* feat_max)
{
    const MelCall mc{Mel{step, skips, n_fft, hop, n_mels}, window, matrix, floor, norm};
    return mel_device(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, d_out, out_capacity, true,
                      best_channel, best_rms, runner_up_rms, out_offsets, mc, n_frames, feat_max);
}

int fvad_clips_export_mel(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                          const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity, int32_t* best_channel,
                          float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step, const uint32_t* skips,
                          uint32_t n_fft, uint32_t hop, const float* window, uint32_t n_mels, const float* matrix, float floor,
                          const float* norm, uint64_t* n_frames, float* feat_max)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_clips == 0) return FVAD_OK;
    const MelCall mc{Mel{step, skips, n_fft, hop, n_mels}, window, matrix, floor, norm};
    // every rule against the caller's own buffer first, then a device staging buffer of the plan's size, one copy back
    uint64_t total = 0;
    const char* why = "";
    const int bad = mel_check(d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, out, out_capacity, 0, mc.m,
                              window, matrix, floor, norm, nullptr, nullptr, &total, &why);
    if (bad != FVAD_OK) return set_err(ctx, bad, std::string("fvad_clips_export_mel: ") + why);
    hipSetDevice(ctx->device);
    const size_t bytes = (size_t)total * sizeof(float);
    void* d_out = nullptr;
    if (hipMalloc(&d_out, bytes) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "fvad_clips_export_mel: hipMalloc of the staging buffer failed"); }
    // the padding between slots is never written by the kernels: zero it, so that the host gets no stale device memory
    hipError_t e = hipMemsetAsync(d_out, 0, bytes, ctx->stream);
    int rc = e == hipSuccess ? mel_device(ctx, d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips, out_format, d_out, (size_t)total,
                                          true, best_channel, best_rms, runner_up_rms, out_offsets, mc, n_frames, feat_max)
                             : hip_fail(ctx, e, "fvad_clips_export_mel: hipMemsetAsync");
    if (rc == FVAD_OK) {
        e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = hip_fail(ctx, e, "fvad_clips_export_mel: copy back");
    }
    hipFree(d_out);
    return rc;
}

} // extern "C"
