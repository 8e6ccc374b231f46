// engine_sweep.cpp -- parameter sweeps on the GPU: several speech bands per K4 pass (fvad_engine_band_sums_device) and every
// (stream, config) VAD machine of a sweep batch at once (fvad_vad_batch_run_device, kernels_vad.hip), scored against the
// streams' labels on the device when the batch has them (kernels_eval.hip).
#include <algorithm>
#include <cmath>
#include <vector>

#include "host_vad.h"
#include "internal.h"

using namespace fvad;

static_assert(sizeof(fvad_single_stats) == 11 * sizeof(float), "fvad_single_stats is copied back as it is");

namespace {

// Without a context there is nothing to run on: FVAD_ERR_NO_DEVICE where no device exists (what fvad_ctx_create would
// have said), else a plain argument error
int no_ctx()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FVAD_ERR_NO_DEVICE;
    return FVAD_ERR_INVALID_ARGUMENT;
}

// device buffers of one call, freed on every way out
struct DevScratch {
    std::vector<void*> ptrs;
    ~DevScratch() { for (void* p : ptrs) hipFree(p); }
    template <class T> hipError_t alloc(T** p, size_t n)
    {
        *p = nullptr;
        const hipError_t e = hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(*p);
        return e;
    }
};

} // namespace

extern "C" {

int fvad_engine_band_sums_device(fvad_ctx* ctx, const float* d_denoised, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                 size_t fft_size, const int32_t* bins, size_t n_bands, float* d_band_sum, size_t band_stride)
{
    if (!ctx) return no_ctx();
    if (n_lanes == 0 || n_bands == 0) return FVAD_OK;
    if (!d_denoised || !bins || !d_band_sum) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null buffer");
    hipSetDevice(ctx->device);
    VadFftPlan plan;
    int rc = get_vad_plan(ctx, fft_size, &plan);
    if (rc) return rc;
    const int F = (int)fft_size;
    for (size_t j = 0; j < n_bands; ++j)
        if (bins[2 * j] < 0 || bins[2 * j + 1] > F / 2 || bins[2 * j + 1] < bins[2 * j]) return set_err(ctx, FVAD_ERR_OUT_OF_RANGE, "band bins out of range");
    const size_t n_frames = n_samples / fft_size;
    if (n_frames == 0) return FVAD_OK;
    if (band_stride < n_frames) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "band_stride < n_samples / fft_size");
    // the FFT kernels read a frame as float pairs
    if ((uintptr_t)d_denoised % 8 || lane_stride % 2) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "denoised frames must be 8-byte aligned");
    hipStream_t st = ctx->stream;
    std::vector<VadFftJob> jobs(n_lanes);
    for (size_t l = 0; l < n_lanes; ++l) jobs[l] = {d_denoised + l * lane_stride, d_band_sum + l * band_stride, nullptr, (long)n_frames};
    DevScratch scratch;
    VadFftJob* d_jobs = nullptr;
    FVAD_HIP(ctx, scratch.alloc(&d_jobs, n_lanes));
    FVAD_HIP(ctx, hipMemcpyAsync(d_jobs, jobs.data(), n_lanes * sizeof(VadFftJob), hipMemcpyHostToDevice, st));
    // the kernel each band's single-band engine call would take (fvad_launch_vadfft_jobs): at 1024 points a band inside 1..47 is the
    // pruned kernel's, every other band the full-spectrum (or generic) kernel's; up to kVadBandsPerLaunch bands share one FFT pass
    const long step = (long)(n_lanes * band_stride);
    std::vector<size_t> cls[2];
    for (size_t j = 0; j < n_bands; ++j) {
        const bool pruned = !plan.generic && F == 1024 && bins[2 * j] >= 1 && bins[2 * j + 1] <= 47;
        cls[pruned ? 1 : 0].push_back(j);
    }
    time_begin(ctx, "k4_bands");
    for (int pruned = 0; pruned < 2; ++pruned) {
        for (size_t b0 = 0; b0 < cls[pruned].size(); b0 += kVadBandsPerLaunch) {
            VadBandSet bs{};
            bs.step = step;
            bs.n = (int)std::min<size_t>(kVadBandsPerLaunch, cls[pruned].size() - b0);
            for (int b = 0; b < bs.n; ++b) {
                const size_t j = cls[pruned][b0 + (size_t)b];
                bs.lo[b] = (int16_t)bins[2 * j];
                bs.hi[b] = (int16_t)bins[2 * j + 1];
                bs.idx[b] = (int32_t)j;
            }
            const int e = fvad_launch_vadfft_bands(d_jobs, (int)n_lanes, (long)n_frames, plan, bs, pruned, st, ctx->n_cu,
                                                   ctx->tune.k4_plain_loads ? 1 : 0);
            if (e != (int)hipSuccess) { time_end(ctx); return hip_fail(ctx, (hipError_t)e, "fvad_launch_vadfft_bands"); }
        }
    }
    time_end(ctx);
    FVAD_HIP(ctx, hipStreamSynchronize(st));
    FVAD_HIP(ctx, hipGetLastError());
    return FVAD_OK;
}

int fvad_vad_batch_run_device(fvad_ctx* ctx, fvad_vad_batch* b, const float* d_band, size_t band_stride, const size_t* n_frames,
                              const float* chunk_rms, size_t rms_stride, const size_t* n_chunks, size_t chunk_size)
{
    if (!ctx) return no_ctx();
    if (!b || !d_band || !n_frames || !n_chunks || !chunk_rms || chunk_size == 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null argument");
    const size_t S = b->n_streams, NC = b->cfgs.size(), C = b->n_channels, F = b->fft_size;
    size_t max_nf = 0;
    for (size_t s = 0; s < S; ++s) {
        if (n_frames[s] * F > n_chunks[s] * chunk_size) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a frame without its chunk's ratio");
        max_nf = std::max(max_nf, n_frames[s]);
    }
    if (band_stride < max_nf) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "band_stride < frames of a stream");
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;

    // ---- host: the frame ratios (one per stream: they do not depend on the config) and the configs' derived constants
    const size_t ratio_stride = std::max<size_t>(max_nf, 1);
    std::vector<float> ratio(S * ratio_stride, 0.0f);
    deal(S, 16, [&](size_t s) {
        sweep_frame_ratios(chunk_rms + s * C * rms_stride, rms_stride, C, n_chunks[s], n_frames[s], F, chunk_size, ratio.data() + s * ratio_stride);
    });
    std::vector<VadMachineCfg> hc(NC);
    uint32_t lt_max = 1, st_max = 1, cr_max = 1;
    for (size_t c = 0; c < NC; ++c) {
        if (vad_machine_cfg(b->cfgs[c], b->sample_rate, F, &hc[c])) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "ring length out of range");
        hc[c].band = b->band_of[c];
        lt_max = std::max(lt_max, hc[c].long_len);
        st_max = std::max(st_max, hc[c].short_len);
        cr_max = std::max(cr_max, hc[c].ratio_len);
    }

    // ---- device
    const long M = (long)(S * NC);
    DevScratch scratch;
    VadMachineCfg* d_cfg = nullptr;
    float* d_ratio = nullptr;
    long* d_nf = nullptr;
    float* d_lt = nullptr;
    float* d_rings = nullptr;
    uint32_t* d_count = nullptr;
    fvad_vad_audit* d_audit = nullptr;
    unsigned long long* d_stats = nullptr;
    std::vector<long> nf_l(n_frames, n_frames + S);
    FVAD_HIP(ctx, scratch.alloc(&d_cfg, NC));
    FVAD_HIP(ctx, scratch.alloc(&d_ratio, ratio.size()));
    FVAD_HIP(ctx, scratch.alloc(&d_nf, S));
    // long-term rings in whole blocks of 64 slots plus one block (the exact chain loads one block ahead, past long_len)
    FVAD_HIP(ctx, scratch.alloc(&d_lt, (((size_t)lt_max + 63) / 64 + 1) * 64 * (size_t)M));
    // the short-term and channel-ratio rings of a workgroup's 64 machines in LDS when they fit in 48 KB, else in global memory
    const bool rings_in_lds = (size_t)(st_max + cr_max) * 64 * sizeof(float) <= 48 * 1024;
    if (!rings_in_lds) FVAD_HIP(ctx, scratch.alloc(&d_rings, (size_t)(st_max + cr_max) * (size_t)M));
    FVAD_HIP(ctx, scratch.alloc(&d_count, (size_t)M));
    FVAD_HIP(ctx, scratch.alloc(&d_audit, (size_t)M));
    FVAD_HIP(ctx, scratch.alloc(&d_stats, 2 * (size_t)M));
    FVAD_HIP(ctx, hipMemcpyAsync(d_cfg, hc.data(), NC * sizeof(VadMachineCfg), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(d_ratio, ratio.data(), ratio.size() * sizeof(float), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(d_nf, nf_l.data(), S * sizeof(long), hipMemcpyHostToDevice, st));

    VadMachinesArgs a{};
    a.cfgs = d_cfg;
    a.n_configs = (int)NC;
    a.n_streams = (long)S;
    a.by_config = ctx->tune.vad_lane_map;
    a.n_channels = (int)C;
    a.n_machines = M;
    a.n_lanes = (long)(S * C);
    a.band = d_band;
    a.band_stride = (long)band_stride;
    a.ratio = d_ratio;
    a.ratio_stride = (long)ratio_stride;
    a.n_frames = d_nf;
    a.fft_size = F;
    a.lt_rings = d_lt;
    a.rings = d_rings;
    a.rings_in_lds = rings_in_lds ? 1 : 0;
    a.st_max = (int)st_max;
    a.cr_max = (int)cr_max;
    a.seg_count = d_count;
    a.audits = d_audit;
    a.stats = d_stats;
    // Segment room.  A machine closes a segment only in a CLOSING -> CLOSED step, and the steps since the previous one include a
    // CLOSED -> OPENING, an OPENING -> OPEN and an OPEN -> CLOSING step, one transition per frame (VADMachine.zig:189-233): at most
    // one segment per 4 frames, n_frames / 4 + 1 bounds every machine.  That bound is the room of the first launch when it is
    // small; otherwise the first launch has room for 512 MB of segments over all machines (context option vad_seg_cap: that many
    // per machine instead) and counts past it, and if any machine closed more, a second launch with room for the largest count
    // redoes the run (the machines start fresh in every launch: same results).
    const size_t bound = max_nf / 4 + 1;
    const size_t room = ctx->tune.vad_seg_cap > 0 ? (size_t)ctx->tune.vad_seg_cap
                                                  : std::max<size_t>(256, (512u << 20) / sizeof(fvad_speech_segment) / (size_t)M);
    size_t cap = std::min(bound, room);
    std::vector<uint32_t> count((size_t)M);
    fvad_speech_segment* d_segs = nullptr;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (d_segs) { hipFree(d_segs); scratch.ptrs.pop_back(); d_segs = nullptr; }
        FVAD_HIP(ctx, scratch.alloc(&d_segs, cap * (size_t)M));
        a.segs = d_segs;
        a.seg_cap = (uint32_t)cap;
        time_begin(ctx, "vad_machines");
        const int e = fvad_launch_vad_machines(a, st);
        time_end(ctx);
        if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "fvad_launch_vad_machines");
        FVAD_HIP(ctx, hipMemcpyAsync(count.data(), d_count, (size_t)M * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        FVAD_HIP(ctx, hipStreamSynchronize(st));
        const size_t most = *std::max_element(count.begin(), count.end());
        if (most <= cap) break;
        if (attempt == 1) return set_err(ctx, FVAD_ERR_HIP, "vad machines: segment count changed between two launches");
        cap = most;
    }
    // ---- scoring (kernels_eval.hip): every machine against its stream's labels, on the segments of the final launch
    std::vector<fvad_single_stats> scores;
    if (b->has_refs) {
        const size_t n_ref = b->ref_off[S];
        fvad_segment_sec* d_refs = nullptr;
        float* d_pmax = nullptr;
        unsigned long long* d_roff = nullptr;
        fvad_stat_config* d_scfg = nullptr;
        fvad_single_stats* d_scores = nullptr;
        const std::vector<unsigned long long> roff(b->ref_off.begin(), b->ref_off.end());
        FVAD_HIP(ctx, scratch.alloc(&d_refs, n_ref));
        FVAD_HIP(ctx, scratch.alloc(&d_pmax, n_ref));
        FVAD_HIP(ctx, scratch.alloc(&d_roff, S + 1));
        FVAD_HIP(ctx, scratch.alloc(&d_scfg, NC));
        FVAD_HIP(ctx, scratch.alloc(&d_scores, (size_t)M));
        if (n_ref) {
            FVAD_HIP(ctx, hipMemcpyAsync(d_refs, b->refs.data(), n_ref * sizeof(fvad_segment_sec), hipMemcpyHostToDevice, st));
            FVAD_HIP(ctx, hipMemcpyAsync(d_pmax, b->ref_pmax.data(), n_ref * sizeof(float), hipMemcpyHostToDevice, st));
        }
        FVAD_HIP(ctx, hipMemcpyAsync(d_roff, roff.data(), (S + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        FVAD_HIP(ctx, hipMemcpyAsync(d_scfg, b->stat_cfgs.data(), NC * sizeof(fvad_stat_config), hipMemcpyHostToDevice, st));
        VadScoreArgs sa{};
        sa.segs = d_segs;
        sa.seg_count = d_count;
        sa.seg_cap = (uint32_t)cap;
        sa.n_machines = M;
        sa.n_configs = (int)NC;
        sa.sample_rate_f = (float)b->sample_rate;
        sa.refs = d_refs;
        sa.ref_pmax = d_pmax;
        sa.ref_off = d_roff;
        sa.stat_cfgs = d_scfg;
        sa.out = d_scores;
        time_begin(ctx, "vad_score");
        const int e = fvad_launch_vad_score(sa, st);
        time_end(ctx);
        if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "fvad_launch_vad_score");
        scores.resize((size_t)M);
        FVAD_HIP(ctx, hipMemcpyAsync(scores.data(), d_scores, (size_t)M * sizeof(fvad_single_stats), hipMemcpyDeviceToHost, st));
    }
    // the segments only when the caller keeps them (fvad_vad_batch_set_keep_segments)
    std::vector<fvad_speech_segment> segs(b->keep_segments ? cap * (size_t)M : 0);
    std::vector<fvad_vad_audit> audits((size_t)M);
    std::vector<unsigned long long> stats(2 * (size_t)M);
    if (b->keep_segments)
        FVAD_HIP(ctx, hipMemcpyAsync(segs.data(), d_segs, segs.size() * sizeof(fvad_speech_segment), hipMemcpyDeviceToHost, st));
    FVAD_HIP(ctx, hipMemcpyAsync(audits.data(), d_audit, audits.size() * sizeof(fvad_vad_audit), hipMemcpyDeviceToHost, st));
    FVAD_HIP(ctx, hipMemcpyAsync(stats.data(), d_stats, stats.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    FVAD_HIP(ctx, hipStreamSynchronize(st));
    FVAD_HIP(ctx, hipGetLastError());
    for (long m = 0; m < M; ++m) {
        auto& v = b->segs[(size_t)m];
        if (b->keep_segments) {
            const fvad_speech_segment* sm = segs.data() + (size_t)m * cap;
            v.assign(sm, sm + count[(size_t)m]);
        } else {
            std::vector<fvad_speech_segment>().swap(v);
        }
        b->exact_evals[(size_t)m] = stats[2 * (size_t)m];
        b->lazy_pushes[(size_t)m] = stats[2 * (size_t)m + 1];
    }
    b->audits = std::move(audits);
    b->segs_kept = b->keep_segments;
    b->scored = b->has_refs;
    if (b->has_refs) b->scores = std::move(scores);
    b->machines.clear(); // nothing to continue from: a later fvad_vad_batch_run_part must start at frame 0
    b->next_frame = 0;
    return FVAD_OK;
}

} // extern "C"
