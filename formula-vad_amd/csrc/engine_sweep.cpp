// engine_sweep.cpp -- parameter sweeps on the GPU: several speech bands per K4 pass (fvad_engine_band_sums_device) and every
// (stream, config) VAD machine of a sweep batch at once (fvad_vad_batch_run_device, kernels_vad.hip), scored against the
// streams' labels on the device when the batch has them (kernels_eval.hip); the same machines in parts, their state kept in
// device memory between the parts (fvad_vad_batch_run_device_part, fvad_vad_batch_score_device); parts that do not wait, on the
// context's second stream, their frame ratios from the device's chunk RMS (fvad_vad_batch_run_device_part_async, _part_wait).
#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "host_vad.h"
#include "internal.h"
#include "vad_finish.h"

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

struct DevParts;
// One part between its launch and its results: run_device_part launches it and finish_part brings the results back.  The blocking
// part calls do both in one call; fvad_vad_batch_run_device_part_async leaves it in DevParts::flight for fvad_vad_batch_part_wait.
struct PartFlight {
    DevScratch scratch;            // the part's per-call inputs (frame ratios, frame and chunk counts)
    VadMachinesArgs a{};           // the launch (segs / seg_cap follow the segment buffer)
    hipStream_t st = nullptr;      // the stream it runs on
    std::vector<size_t> n_frames;  // [n_sizes][n_streams]
    std::vector<size_t> P;         // each size's longest stream in the part
    size_t most = 0;               // segments no machine can exceed
    bool keep = false;
    uint64_t first_sample = 0;
    bool finish = false;           // the shared-trigger form's second stage: launch_part launches the finishing kernel
};

// The device state of a batch run in parts (fvad_vad_batch_run_device_part), held by the batch between the parts: the machines
// (kernels_vad.hip's resume form: VadLaneState, the long-term rings, the short-term and channel-ratio rings), their outputs and
// the segment buffer.  Freed with the batch (fvad_vad_batch_destroy) or when a run starts afresh.
struct DevParts {
    int device = 0;
    const fvad_ctx* ctx = nullptr; // the context of the parts (every part runs on it)
    std::vector<void*> ptrs;       // every allocation but the segment buffer
    size_t bytes = 0;              // their size
    VadMachineCfg* cfg = nullptr;
    float* lt = nullptr;
    float* rings = nullptr;
    VadLaneState* state = nullptr;
    uint32_t* count = nullptr;
    fvad_vad_audit* audit = nullptr;
    unsigned long long* stats = nullptr;
    unsigned* paused = nullptr;
    fvad_speech_segment* segs = nullptr; // [machine][seg_cap]
    size_t seg_cap = 0;
    bool rings_in_lds = false;
    int by_config = 0;                   // the lane map of the first part (the rings are laid out by it)
    int size_order = 0;                  // the context's vad_size_order at the first part (a sized batch's lane order)
    uint32_t lt_max = 1, st_max = 1, cr_max = 1;
    uint64_t next_sample = 0;            // where the next part starts (UINT64_MAX: none can follow)
    uint64_t* sizes = nullptr;           // several frame sizes (VadMachinesArgs.sized): the sizes, each config's, the lane order
    uint32_t* size_of = nullptr;
    int* lane_config = nullptr;
    std::vector<int> order;              // lane_config's host copy (empty with one size: lane j of a stream runs config j)
    std::vector<uint8_t> ended;          // streams that got fewer frames than a part's longest
    std::vector<uint32_t> count_h;       // every machine's segment count after the last part
    bool segs_on_device = true;          // every part so far left its segments on the device: they are all in segs
    std::unique_ptr<PartFlight> flight;  // a part launched and not yet waited for (fvad_vad_batch_run_device_part_async)
    // the averages' tables of a part (context option vad_avgs "table"): the min_volume rows and the two tables; they only grow
    float* mv = nullptr;
    double *st_tab = nullptr, *cr_tab = nullptr;
    size_t mv_cap = 0, st_cap = 0, cr_cap = 0; // in elements
    size_t table_bytes() const { return mv_cap * sizeof(float) + (st_cap + cr_cap) * sizeof(double) + bits_cap * sizeof(unsigned long long); }
    // The shared-trigger form (context option vad_trigger "shared").  `shared`: this is the state of a batch whose parts run the
    // finishing kernel over its trigger batch's bits (fvad_vad_batch::trig): no rings, trig_of / finish_order on the device.
    // `emit`: this is a trigger batch's state; bits: the last part's words (they only grow), trig_h / nf_h: their layout and the
    // part's frame counts [n_sizes][n_streams] (fvad_vad_batch_trigger_bits)
    bool shared = false, emit = false;
    uint32_t* trig_of = nullptr;
    int* finish_order = nullptr;
    unsigned long long* bits = nullptr;
    size_t bits_cap = 0;
    std::vector<VadTrigKey> trig_h;
    std::vector<size_t> nf_h;
    ~DevParts()
    {
        hipSetDevice(device);
        if (flight) hipDeviceSynchronize(); // (a batch destroyed with its part in flight: the kernels read what is freed below)
        free_machines();
        hipFree(bits);
    }
    // everything but the bits and their layout (a trigger batch after a one-shot run: no part can follow, fvad_vad_batch_trigger_bits
    // still reads the bits); nothing of this state may be in flight
    void free_machines()
    {
        for (void* p : ptrs) hipFree(p);
        hipFree(segs);
        hipFree(mv);
        hipFree(st_tab);
        hipFree(cr_tab);
        ptrs.clear();
        bytes = 0;
        cfg = nullptr; lt = nullptr; rings = nullptr; state = nullptr; count = nullptr; audit = nullptr; stats = nullptr; paused = nullptr;
        segs = nullptr; sizes = nullptr; size_of = nullptr; lane_config = nullptr; trig_of = nullptr; finish_order = nullptr;
        mv = nullptr; st_tab = nullptr; cr_tab = nullptr;
        seg_cap = mv_cap = st_cap = cr_cap = 0;
        next_sample = UINT64_MAX;
    }
    template <class T> hipError_t grow(T** p, size_t* cap, size_t need) // (the contents are not kept; nothing in flight reads them)
    {
        if (need <= *cap) return hipSuccess;
        hipFree(*p);
        *p = nullptr;
        *cap = 0;
        const hipError_t e = hipMalloc((void**)p, need * sizeof(T));
        if (e == hipSuccess) *cap = need;
        return e;
    }
    template <class T> hipError_t alloc(T** p, size_t n)
    {
        *p = nullptr;
        const size_t nb = std::max<size_t>(n, 1) * sizeof(T);
        const hipError_t e = hipMalloc((void**)p, nb);
        if (e == hipSuccess) { ptrs.push_back(*p); bytes += nb; }
        return e;
    }
};
void free_dev_parts(void* p) { delete static_cast<DevParts*>(p); }

// The lane order of a sized launch by stream (VadMachinesArgs.lane_config): a stream's configs size-major (first-seen order within
// a size), so that a wavefront mostly runs one frame clock; the caller's order with the context option vad_size_order "caller"
std::vector<int> lane_order(const fvad_vad_batch* b, int size_order)
{
    std::vector<int> o(b->cfgs.size());
    for (size_t c = 0; c < o.size(); ++c) o[c] = (int)c;
    if (size_order == 0)
        std::stable_sort(o.begin(), o.end(), [&](int x, int y) { return b->size_of[(size_t)x] < b->size_of[(size_t)y]; });
    return o;
}

// the per-size inputs a launch checks: every (size g, stream s) has n_frames[g * S + s] frames, inside its n_chunks[s] chunks;
// P[g] = the longest of size g.  FVAD_OK or the message of the broken rule.
const char* frame_counts(const fvad_vad_batch* b, const size_t* n_frames, const size_t* n_chunks, size_t chunk_size, std::vector<size_t>* P)
{
    const size_t S = b->n_streams, G = b->sizes.size();
    P->assign(G, 0);
    for (size_t g = 0; g < G; ++g)
        for (size_t s = 0; s < S; ++s) {
            const size_t nf = n_frames[g * S + s];
            if (nf > (n_chunks[s] * chunk_size) / b->sizes[g]) return "a frame without its chunk's ratio";
            (*P)[g] = std::max((*P)[g], nf);
        }
    return nullptr;
}

// every machine of b against its stream's labels on the device (kernels_eval.hip): segment i of machine m at d_segs[m * cap + i],
// d_count[m] of them (at most cap); the scores come back into *out
int score_on_device(fvad_ctx* ctx, const fvad_vad_batch* b, const fvad_speech_segment* d_segs, const uint32_t* d_count, size_t cap,
                    std::vector<fvad_single_stats>* out)
{
    const size_t S = b->n_streams, NC = b->cfgs.size(), M = S * NC;
    hipStream_t st = ctx->stream;
    DevScratch scratch;
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
    FVAD_HIP(ctx, scratch.alloc(&d_scores, M));
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
    sa.n_machines = (long)M;
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
    out->resize(M);
    FVAD_HIP(ctx, hipMemcpyAsync(out->data(), d_scores, M * sizeof(fvad_single_stats), hipMemcpyDeviceToHost, st));
    FVAD_HIP(ctx, hipStreamSynchronize(st)); // (before the scratch is freed)
    return FVAD_OK;
}

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

} // extern "C"

namespace {

// (the shared-trigger form, below: whether a run's first launch takes it; emit: the part of a trigger batch)
bool trigger_wanted(const fvad_ctx* ctx, const fvad_vad_batch* b, const std::vector<size_t>& P);
int run_device_part(fvad_ctx* ctx, fvad_vad_batch* b, const float* d_band, size_t band_stride, const size_t* n_frames,
                    const float* chunk_rms, const float* d_chunk_rms, size_t rms_stride, const size_t* n_chunks, size_t chunk_size,
                    uint64_t first_sample, bool async, bool emit = false);

// the configs' derived constants at their own frame sizes, with their bands; the rings' largest lengths
int derive_cfgs(fvad_ctx* ctx, const fvad_vad_batch* b, std::vector<VadMachineCfg>* hc, uint32_t* lt_max, uint32_t* st_max, uint32_t* cr_max)
{
    const size_t NC = b->cfgs.size();
    hc->resize(NC);
    *lt_max = *st_max = *cr_max = 1;
    for (size_t c = 0; c < NC; ++c) {
        VadMachineCfg& k = (*hc)[c];
        if (vad_machine_cfg(b->cfgs[c], b->sample_rate, b->sizes[b->size_of[c]], &k)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "ring length out of range");
        k.band = b->band_of[c];
        *lt_max = std::max(*lt_max, k.long_len);
        *st_max = std::max(*st_max, k.short_len);
        *cr_max = std::max(*cr_max, k.ratio_len);
    }
    return FVAD_OK;
}

// the frame ratios of every (size g, stream s) row, ratio_stride apart (they do not depend on the config), from frame
// first_sample / F of the size on
std::vector<float> sized_ratios(const fvad_vad_batch* b, const size_t* n_frames, const float* chunk_rms, size_t rms_stride,
                                const size_t* n_chunks, size_t chunk_size, uint64_t first_sample, size_t ratio_stride)
{
    const size_t S = b->n_streams, C = b->n_channels;
    std::vector<float> ratio(b->sizes.size() * S * ratio_stride, 0.0f);
    deal(b->sizes.size() * S, 16, [&](size_t i) {
        const size_t s = i % S, F = b->sizes[i / S];
        sweep_frame_ratios(chunk_rms + s * C * rms_stride, rms_stride, C, n_chunks[s], n_frames[i], F, chunk_size, ratio.data() + i * ratio_stride,
                           first_sample / F);
    });
    return ratio;
}

// The averages' tables of a part (kernels_vadavgs.hip): the keys with their places in the tables, the tables' sizes.  P[g]: the
// part's longest row of size g; by_config / order: the lane map and lane order of the machines whose homes hold the history
struct AvgsPlan {
    std::vector<VadAvgKey> st, cr;
    std::vector<long> tab_frames;      // [n_sizes]
    std::vector<uint64_t> first_frame; // [n_sizes]
    size_t st_elems = 0, cr_elems = 0, mv_elems = 0, mv_stride = 1;
    size_t bytes() const { return mv_elems * sizeof(float) + (st_elems + cr_elems) * sizeof(double); }
};
AvgsPlan plan_avgs(const fvad_vad_batch* b, const std::vector<size_t>& P, uint64_t first_sample, int by_config, const std::vector<int>& order)
{
    const size_t S = b->n_streams, G = b->sizes.size(), NC = b->cfgs.size();
    AvgsPlan pl;
    pl.tab_frames.assign(P.begin(), P.end());
    pl.first_frame.resize(G);
    for (size_t g = 0; g < G; ++g) pl.first_frame[g] = first_sample / b->sizes[g];
    pl.mv_stride = std::max<size_t>(*std::max_element(P.begin(), P.end()), 1);
    pl.mv_elems = (b->bins.size() / 2) * S * pl.mv_stride;
    auto lane_of = [&](size_t c) { // the lane whose place holds config c's rings (place_of)
        if (by_config || order.empty()) return (long)c;
        return (long)(std::find(order.begin(), order.end(), (int)c) - order.begin());
    };
    auto lay = [&](const std::vector<uint32_t>& pairs, const std::vector<uint32_t>& key_of, bool is_st, std::vector<VadAvgKey>* out, size_t* elems) {
        const size_t K = pairs.size() / 2;
        out->resize(K);
        std::vector<uint32_t> nk(G, 0);
        for (size_t j = 0; j < K; ++j) {
            VadAvgKey& k = (*out)[j];
            k.src = pairs[2 * j];
            k.len = pairs[2 * j + 1];
            k.size = is_st ? b->size_of_band[k.src] : k.src;
            k.base = (long)nk[k.size]++; // (its index among its size's keys: the size's first entry is added below)
            k.scalar = 1.0 / (double)k.len; // (vad_machine_cfg's st_scalar / cr_scalar)
            const size_t c = (size_t)(std::find(key_of.begin(), key_of.end(), (uint32_t)j) - key_of.begin());
            k.rep = lane_of(c < NC ? c : 0);
        }
        std::vector<long> first(G, 0);
        size_t n = 0;
        for (size_t g = 0; g < G; ++g) { first[g] = (long)n; n += S * P[g] * nk[g]; }
        for (VadAvgKey& k : *out) { k.nk = nk[k.size]; k.base += first[k.size]; }
        *elems = n;
    };
    lay(b->st_keys, b->st_key, true, &pl.st, &pl.st_elems);
    lay(b->cr_keys, b->cr_key, false, &pl.cr, &pl.cr_elems);
    return pl;
}

// whether a launch with the context's options may use the tables at all (the budget is checked against the plan)
bool avgs_wanted_shape(const fvad_vad_batch* b) // (the grid of the tables' kernels: streams x bands or keys)
{
    return (long)b->n_streams <= kAvgsGridMax && (long)(b->bins.size() / 2) <= kAvgsGridMax &&
           (long)((b->st_keys.size() + b->cr_keys.size()) / 2) <= kAvgsGridMax;
}
bool avgs_wanted(const fvad_ctx* ctx, const fvad_vad_batch* b)
{
    return ctx->tune.vad_avgs == 1 && ctx->tune.vad_chain == 1 && avgs_wanted_shape(b);
}

// Fill the tables of a part on stream st: upload the plan (into scratch, which lives as long as the launches that read it), run
// the two kernels.  ma: the machines' launch (band, ratio, frame counts, homes and lane map are taken from it; its table fields
// are set).  d_mv / d_st / d_cr: buffers of at least the plan's sizes.
int fill_avgs(fvad_ctx* ctx, const fvad_vad_batch* b, const AvgsPlan& pl, DevScratch& scratch, float* d_mv, double* d_st, double* d_cr,
              long max_nf, VadMachinesArgs* ma, hipStream_t st)
{
    const size_t G = b->sizes.size(), NC = b->cfgs.size();
    VadAvgKey *d_stk = nullptr, *d_crk = nullptr;
    uint32_t *d_st_key = nullptr, *d_cr_key = nullptr, *d_sob = nullptr;
    long* d_tf = nullptr;
    uint64_t* d_ff = nullptr;
    FVAD_HIP(ctx, scratch.alloc(&d_stk, pl.st.size()));
    FVAD_HIP(ctx, scratch.alloc(&d_crk, pl.cr.size()));
    FVAD_HIP(ctx, scratch.alloc(&d_st_key, NC));
    FVAD_HIP(ctx, scratch.alloc(&d_cr_key, NC));
    FVAD_HIP(ctx, scratch.alloc(&d_sob, b->size_of_band.size()));
    FVAD_HIP(ctx, scratch.alloc(&d_tf, G));
    FVAD_HIP(ctx, scratch.alloc(&d_ff, G));
    FVAD_HIP(ctx, hipMemcpyAsync(d_stk, pl.st.data(), pl.st.size() * sizeof(VadAvgKey), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(d_crk, pl.cr.data(), pl.cr.size() * sizeof(VadAvgKey), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(d_st_key, b->st_key.data(), NC * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(d_cr_key, b->cr_key.data(), NC * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(d_sob, b->size_of_band.data(), b->size_of_band.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(d_tf, pl.tab_frames.data(), G * sizeof(long), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(d_ff, pl.first_frame.data(), G * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    VadAvgsArgs va{};
    va.band = ma->band;
    va.band_stride = ma->band_stride;
    va.n_lanes = ma->n_lanes;
    va.n_channels = ma->n_channels;
    va.n_bands = (int)(b->bins.size() / 2);
    va.n_sizes = (int)G;
    va.n_streams = ma->n_streams;
    va.size_of_band = d_sob;
    va.n_frames = ma->n_frames;
    va.max_frames = max_nf;
    va.minvol = d_mv;
    va.minvol_stride = (long)pl.mv_stride;
    va.ratio = ma->ratio;
    va.ratio_stride = ma->ratio_stride;
    va.st_keys = d_stk;
    va.cr_keys = d_crk;
    va.n_st_keys = (int)pl.st.size();
    va.n_cr_keys = (int)pl.cr.size();
    va.st_tab = d_st;
    va.cr_tab = d_cr;
    va.tab_frames = d_tf;
    va.first_frame = d_ff;
    va.fresh = pl.first_frame[0] == 0;
    va.rings = ma->rings;
    va.st_max = ma->st_max;
    va.by_config = ma->by_config;
    va.n_configs = ma->n_configs;
    va.n_machines = ma->n_machines;
    const bool timed = st == ctx->stream;
    if (timed) time_begin(ctx, "vad_minvol");
    int e = fvad_launch_vad_minvol(va, st);
    if (timed) time_end(ctx);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "fvad_launch_vad_minvol");
    if (timed) time_begin(ctx, "vad_avgs");
    e = fvad_launch_vad_avgs(va, st);
    if (timed) time_end(ctx);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "fvad_launch_vad_avgs");
    ma->table = 1;
    ma->minvol = d_mv;
    ma->minvol_stride = (long)pl.mv_stride;
    ma->st_tab = d_st;
    ma->cr_tab = d_cr;
    ma->st_keys = d_stk;
    ma->cr_keys = d_crk;
    ma->st_key = d_st_key;
    ma->cr_key = d_cr_key;
    ma->tab_frames = d_tf;
    return FVAD_OK;
}

// one launch of every machine of b (fvad_vad_batch_run_device and _run_device_sized); n_frames [n_sizes][n_streams]
int run_device(fvad_ctx* ctx, fvad_vad_batch* b, const float* d_band, size_t band_stride, const size_t* n_frames,
               const float* chunk_rms, size_t rms_stride, const size_t* n_chunks, size_t chunk_size)
{
    const size_t S = b->n_streams, NC = b->cfgs.size(), C = b->n_channels, G = b->sizes.size();
    std::vector<size_t> P;
    if (const char* msg = frame_counts(b, n_frames, n_chunks, chunk_size, &P)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, msg);
    const size_t max_nf = *std::max_element(P.begin(), P.end());
    if (band_stride < max_nf) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "band_stride < frames of a stream");
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    if (trigger_wanted(ctx, b, P)) {
        // The shared-trigger form: the run is one fresh part of that form -- the emitting machines once, then the finishing kernel,
        // which alone runs again when a machine's segment room overflows -- scored on the device where the part left its segments
        if (const int rc = run_device_part(ctx, b, d_band, band_stride, n_frames, chunk_rms, nullptr, rms_stride, n_chunks, chunk_size, 0, false))
            return rc;
        const DevParts* dp = static_cast<const DevParts*>(b->dev_parts.get());
        if (b->has_refs) {
            std::vector<fvad_single_stats> scores;
            if (const int rc = score_on_device(ctx, b, dp->segs, dp->count, dp->seg_cap, &scores)) return rc;
            b->scores = std::move(scores);
        }
        b->scored = b->has_refs;
        b->dev_parts.reset(); // a run in parts cannot go on after this one; of the trigger batch only the bits stay (fvad_vad_batch_trigger_bits)
        if (b->trig && b->trig->dev_parts) static_cast<DevParts*>(b->trig->dev_parts.get())->free_machines();
        b->next_sample = 0;
        return FVAD_OK;
    }
    b->dev_parts.reset(); // a run in parts cannot go on after this one
    b->trig.reset();
    b->trig_of.clear();
    b->trigger_bytes = 0;

    // ---- host: the frame ratios (one row per (size, stream)) and the configs' derived constants
    const size_t ratio_stride = std::max<size_t>(max_nf, 1);
    const std::vector<float> ratio = sized_ratios(b, n_frames, chunk_rms, rms_stride, n_chunks, chunk_size, 0, ratio_stride);
    std::vector<VadMachineCfg> hc;
    uint32_t lt_max, st_max, cr_max;
    if (const int rc = derive_cfgs(ctx, b, &hc, &lt_max, &st_max, &cr_max)) return rc;

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
    std::vector<long> nf_l(n_frames, n_frames + G * S);
    FVAD_HIP(ctx, scratch.alloc(&d_cfg, NC));
    FVAD_HIP(ctx, scratch.alloc(&d_ratio, ratio.size()));
    FVAD_HIP(ctx, scratch.alloc(&d_nf, G * S));
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
    FVAD_HIP(ctx, hipMemcpyAsync(d_nf, nf_l.data(), G * S * sizeof(long), hipMemcpyHostToDevice, st));

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
    a.fft_size = b->fft_size;
    a.lt_rings = d_lt;
    a.rings = d_rings;
    a.rings_in_lds = rings_in_lds ? 1 : 0;
    a.st_max = (int)st_max;
    a.cr_max = (int)cr_max;
    a.seg_count = d_count;
    a.audits = d_audit;
    a.stats = d_stats;
    std::vector<int> order_h;
    if (G > 1) { // several frame clocks: the sized form of the kernel (one size runs the single-size form, as a create_sweep batch)
        uint64_t* d_sizes = nullptr;
        uint32_t* d_size_of = nullptr;
        int* d_order = nullptr;
        const std::vector<uint64_t> sizes(b->sizes.begin(), b->sizes.end());
        const std::vector<int> order = lane_order(b, ctx->tune.vad_size_order);
        order_h = order;
        FVAD_HIP(ctx, scratch.alloc(&d_sizes, G));
        FVAD_HIP(ctx, scratch.alloc(&d_size_of, NC));
        FVAD_HIP(ctx, scratch.alloc(&d_order, NC));
        FVAD_HIP(ctx, hipMemcpyAsync(d_sizes, sizes.data(), G * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        FVAD_HIP(ctx, hipMemcpyAsync(d_size_of, b->size_of.data(), NC * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        FVAD_HIP(ctx, hipMemcpyAsync(d_order, order.data(), NC * sizeof(int), hipMemcpyHostToDevice, st));
        a.sized = 1;
        a.sizes = d_sizes;
        a.size_of = d_size_of;
        a.lane_config = d_order;
        a.first_sample = 0;
    }
    // Segment room.  A machine closes a segment only in a CLOSING -> CLOSED step, and the steps since the previous one include a
    // CLOSED -> OPENING, an OPENING -> OPEN and an OPEN -> CLOSING step, one transition per frame (VADMachine.zig:189-233): at most
    // one segment per 4 frames, n_frames / 4 + 1 bounds every machine (the largest over the sizes).  That bound is the room of the
    // first launch when it is small; otherwise the first launch has room for 512 MB of segments over all machines (context option
    // vad_seg_cap: that many per machine instead) and counts past it, and if any machine closed more, a second launch with room for
    // the largest count redoes the run (the machines start fresh in every launch: same results).
    // the averages' tables (context option vad_avgs "table" with vad_chain "coop", within vad_avgs_max_bytes): filled once, before
    // the first launch; a second launch for segment room reads them again
    b->avgs_bytes = 0;
    if (avgs_wanted(ctx, b) && max_nf) {
        const AvgsPlan pl = plan_avgs(b, P, 0, a.by_config, order_h);
        if (pl.bytes() <= ctx->tune.vad_avgs_max_bytes) {
            float* d_mv = nullptr;
            double *d_st = nullptr, *d_cr = nullptr;
            FVAD_HIP(ctx, scratch.alloc(&d_mv, pl.mv_elems));
            FVAD_HIP(ctx, scratch.alloc(&d_st, pl.st_elems));
            FVAD_HIP(ctx, scratch.alloc(&d_cr, pl.cr_elems));
            if (const int rc = fill_avgs(ctx, b, pl, scratch, d_mv, d_st, d_cr, (long)max_nf, &a, st)) return rc;
            b->avgs_bytes = pl.bytes();
        }
    }
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
        a.coop = ctx->tune.vad_chain; // (context option vad_chain, read at every launch: the bits do not depend on it)
        time_begin(ctx, "vad_machines");
        const int e = fvad_launch_vad_machines(a, st);
        time_end(ctx);
        if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "fvad_launch_vad_machines");
        b->chain_form = a.coop ? 2 : 1;
        b->avgs_form = a.coop && a.table ? 2 : 1;
        b->trigger_form = 1;
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
        const int rc = score_on_device(ctx, b, d_segs, d_count, cap, &scores);
        if (rc) return rc;
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
    b->state_on_device = true;
    b->next_sample = 0;
    return FVAD_OK;
}

// the segment buffer of dp with room for cap segments per machine (M machines), the old contents kept
int grow_segs(fvad_ctx* ctx, DevParts* dp, size_t M, size_t cap, hipStream_t st)
{
    fvad_speech_segment* d = nullptr;
    FVAD_HIP(ctx, hipMalloc((void**)&d, std::max<size_t>(cap * M, 1) * sizeof(fvad_speech_segment)));
    if (dp->segs && dp->seg_cap) {
        const size_t w = dp->seg_cap * sizeof(fvad_speech_segment);
        const hipError_t e = hipMemcpy2DAsync(d, cap * sizeof(fvad_speech_segment), dp->segs, w, w, M, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) hipStreamSynchronize(st);
        if (e != hipSuccess) { hipFree(d); return hip_fail(ctx, e, "hipMemcpy2DAsync"); }
    }
    hipFree(dp->segs);
    dp->segs = d;
    dp->seg_cap = cap;
    return FVAD_OK;
}

// the machines of a part on its stream (the first launch, and again after a pause); the kernel-time table is the main stream's
int launch_part(fvad_ctx* ctx, fvad_vad_batch* b, DevParts* dp, PartFlight& pf)
{
    pf.a.segs = dp->segs;
    pf.a.seg_cap = (uint32_t)dp->seg_cap;
    pf.a.coop = ctx->tune.vad_chain; // (context option vad_chain, read at every launch: the bits do not depend on it)
    if (pf.a.emit) pf.a.coop = 1;    // (a shared run stays shared: only the cooperative form emits)
    FVAD_HIP(ctx, hipMemsetAsync(dp->paused, 0, sizeof(unsigned), pf.st));
    const bool timed = pf.st == ctx->stream;
    if (pf.finish) { // the shared form's second stage, alone: the bits are the part's, whatever room the segments needed
        if (timed) time_begin(ctx, "vad_finish");
        const int e = fvad_launch_vad_finish(pf.a, pf.st);
        if (timed) time_end(ctx);
        if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "fvad_launch_vad_finish");
        b->trig_finish_launches += 1;
        b->trigger_form = 2;
        return FVAD_OK;
    }
    if (timed) time_begin(ctx, "vad_machines");
    const int e = fvad_launch_vad_machines(pf.a, pf.st);
    if (timed) time_end(ctx);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "fvad_launch_vad_machines");
    b->chain_form = pf.a.coop ? 2 : 1;
    b->avgs_form = pf.a.coop && pf.a.table ? 2 : 1; // (a part that filled its tables and is relaunched as the lane form runs the rings)
    b->trigger_form = 1; // (on a trigger batch: its own machines; the batch that owns it reports 2)
    return FVAD_OK;
}

// the rest of a launched part: wait, go on with more segment room while machines paused, bring the results into b
int finish_part(fvad_ctx* ctx, fvad_vad_batch* b, DevParts* dp, PartFlight& pf)
{
    const size_t S = b->n_streams, NC = b->cfgs.size(), G = b->sizes.size();
    const size_t M = S * NC;
    hipStream_t st = pf.st;
    const bool keep = pf.keep;
    const uint64_t first_sample = pf.first_sample;
    const std::vector<size_t>& P = pf.P;
    // the shared form: the trigger batch's part first (it never pauses); its inputs -- the ratios and frame counts the finishing
    // kernel reads too -- live until this part is done
    std::unique_ptr<PartFlight> trig_flight;
    if (pf.finish) {
        DevParts* tdp = static_cast<DevParts*>(b->trig->dev_parts.get());
        trig_flight = std::move(tdp->flight);
        if (const int rc = finish_part(ctx, b->trig.get(), tdp, *trig_flight)) return rc;
    }
    for (;;) {
        unsigned paused = 0;
        FVAD_HIP(ctx, hipMemcpyAsync(&paused, dp->paused, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        FVAD_HIP(ctx, hipStreamSynchronize(st));
        if (!paused) break;
        // a machine ran out of room: go on from where each machine stopped, with twice the room (no machine needs more than most)
        const size_t cap = std::min(2 * dp->seg_cap, pf.most);
        if (cap <= dp->seg_cap) return set_err(ctx, FVAD_ERR_HIP, "vad machines: more segments than frames allow");
        if (const int rc = grow_segs(ctx, dp, M, cap, st)) return rc;
        pf.a.fresh = 0;
        pf.a.rebase = 0;
        if (const int rc = launch_part(ctx, b, dp, pf)) return rc;
    }

    // ---- results: everything run so far
    std::vector<uint32_t> count(M);
    std::vector<fvad_vad_audit> audits(M);
    std::vector<unsigned long long> stats(2 * M);
    FVAD_HIP(ctx, hipMemcpyAsync(count.data(), dp->count, M * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (pf.finish) { // a config's audit and lazy statistics are its trigger machine's: decide sees only trigger state
        const fvad_vad_batch* tb = b->trig.get();
        const size_t K = tb->cfgs.size();
        for (size_t s = 0; s < S; ++s)
            for (size_t c = 0; c < NC; ++c) {
                const size_t m = s * NC + c, t = s * K + b->trig_of[c];
                audits[m] = tb->audits[t];
                stats[2 * m] = tb->exact_evals[t];
                stats[2 * m + 1] = tb->lazy_pushes[t];
            }
    } else {
        FVAD_HIP(ctx, hipMemcpyAsync(audits.data(), dp->audit, M * sizeof(fvad_vad_audit), hipMemcpyDeviceToHost, st));
        FVAD_HIP(ctx, hipMemcpyAsync(stats.data(), dp->stats, 2 * M * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    FVAD_HIP(ctx, hipStreamSynchronize(st));
    std::vector<fvad_speech_segment> segs;
    size_t used = 0; // the part's segments: machine m's new ones at the start of its row
    if (keep) {
        for (size_t m = 0; m < M; ++m) used = std::max<size_t>(used, count[m] - dp->count_h[m]);
        segs.resize(used * M);
        if (used) {
            const size_t w = used * sizeof(fvad_speech_segment);
            FVAD_HIP(ctx, hipMemcpy2DAsync(segs.data(), w, dp->segs, dp->seg_cap * sizeof(fvad_speech_segment), w, M, hipMemcpyDeviceToHost, st));
            FVAD_HIP(ctx, hipStreamSynchronize(st));
        }
    }
    FVAD_HIP(ctx, hipGetLastError());
    const bool all_kept = keep && (first_sample == 0 || b->segs_kept);
    for (size_t m = 0; m < M; ++m) {
        auto& v = b->segs[m];
        if (all_kept) {
            const fvad_speech_segment* sm = segs.data() + m * used;
            v.insert(v.end(), sm, sm + (count[m] - dp->count_h[m]));
        } else {
            std::vector<fvad_speech_segment>().swap(v);
        }
        b->exact_evals[m] = stats[2 * m];
        b->lazy_pushes[m] = stats[2 * m + 1];
    }
    b->audits = std::move(audits);
    dp->count_h = std::move(count);
    for (size_t g = 0; g < G; ++g)
        for (size_t s = 0; s < S; ++s)
            if (pf.n_frames[g * S + s] < P[g]) dp->ended[s] = 1;
    uint64_t next = first_sample + P[0] * b->sizes[0];
    for (size_t g = 1; g < G; ++g)
        if (first_sample + P[g] * b->sizes[g] != next) next = UINT64_MAX; // (the sizes ended apart: no part can follow)
    dp->next_sample = next;
    b->segs_kept = all_kept;
    b->scored = false; // the scores were of the previous segments
    return FVAD_OK;
}

// the context's second stream and the event that orders it behind the main one (fvad_vad_batch_run_device_part_async)
int part_stream(fvad_ctx* ctx, hipStream_t* out)
{
    if (!ctx->part_stream) FVAD_HIP(ctx, hipStreamCreateWithFlags(&ctx->part_stream, hipStreamNonBlocking));
    if (!ctx->part_ev) FVAD_HIP(ctx, hipEventCreateWithFlags(&ctx->part_ev, hipEventDisableTiming));
    *out = ctx->part_stream;
    return FVAD_OK;
}

// the frame ratios of a part on the device (kernels_vadratio.hip): rows (size, stream) ratio_stride apart, from the device's chunk
// RMS; d_counts holds n_frames [n_sizes][n_streams] and then n_chunks [n_streams]; d_sizes null with one size
int device_ratios(fvad_ctx* ctx, const fvad_vad_batch* b, const uint64_t* d_sizes, const long* d_counts, const float* d_chunk_rms,
                  size_t rms_stride, size_t chunk_size, uint64_t first_sample, float* d_ratio, size_t ratio_stride, size_t max_nf, hipStream_t st)
{
    const size_t S = b->n_streams, G = b->sizes.size();
    VadRatioArgs ra{};
    ra.chunk_rms = d_chunk_rms;
    ra.rms_stride = (long)rms_stride;
    ra.n_channels = (int)b->n_channels;
    ra.n_sizes = (int)G;
    ra.n_streams = (long)S;
    ra.sizes = d_sizes;
    ra.fft_size = b->fft_size;
    ra.n_frames = d_counts;
    ra.n_chunks = d_counts + G * S;
    ra.chunk_size = chunk_size;
    ra.first_sample = first_sample;
    ra.ratio = d_ratio;
    ra.ratio_stride = (long)ratio_stride;
    ra.max_frames = (long)max_nf;
    const bool timed = st == ctx->stream;
    if (timed) time_begin(ctx, "vad_ratios");
    const int e = fvad_launch_vad_frame_ratios(ra, st);
    if (timed) time_end(ctx);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "fvad_launch_vad_frame_ratios");
    return FVAD_OK;
}

// The bits of a part of trigger batch tb (VadMachinesArgs.bits): per size [stream][word][machines of that size], the sizes one
// after the other; keys[c]: machine c's place, words: 64-bit words in all.  P[g]: the part's longest row of size g
struct TrigPlan {
    std::vector<VadTrigKey> keys;
    size_t words = 0;
};
TrigPlan plan_trigger(const fvad_vad_batch* tb, const std::vector<size_t>& P)
{
    const size_t S = tb->n_streams, G = tb->sizes.size(), K = tb->cfgs.size();
    TrigPlan tp;
    tp.keys.resize(K);
    std::vector<uint32_t> nk(G, 0);
    for (size_t c = 0; c < K; ++c) tp.keys[c].base = (long)nk[tb->size_of[c]]++; // (its index among its size's machines)
    std::vector<long> first(G, 0);
    for (size_t g = 0; g < G; ++g) { first[g] = (long)tp.words; tp.words += S * finish_words(P[g]) * nk[g]; }
    for (size_t c = 0; c < K; ++c) {
        const uint32_t g = tb->size_of[c];
        tp.keys[c].base += first[g];
        tp.keys[c].nk = nk[g];
        tp.keys[c].words = (uint32_t)finish_words(P[g]);
    }
    return tp;
}
// the bytes the bits of a part of b's keys would take (the guard of the shared form: computed from shapes)
size_t trigger_bits_bytes(const fvad_vad_batch* b, const std::vector<size_t>& P)
{
    std::vector<size_t> nk(b->sizes.size(), 0);
    for (const uint32_t c : b->trig_rep) nk[b->size_of[c]] += 1;
    size_t words = 0;
    for (size_t g = 0; g < nk.size(); ++g) words += b->n_streams * finish_words(P[g]) * nk[g];
    return words * sizeof(unsigned long long);
}
bool trigger_wanted(const fvad_ctx* ctx, const fvad_vad_batch* b, const std::vector<size_t>& P)
{
    return ctx->tune.vad_trigger == 1 && ctx->tune.vad_chain == 1 && trigger_bits_bytes(b, P) <= ctx->tune.vad_trigger_max_bytes;
}

int run_shared_part(fvad_ctx* ctx, fvad_vad_batch* b, const float* d_band, size_t band_stride, const size_t* n_frames,
                    const float* chunk_rms, const float* d_chunk_rms, size_t rms_stride, const size_t* n_chunks, size_t chunk_size,
                    uint64_t first_sample, bool async, const std::vector<size_t>& P, hipStream_t st);

// one part of every machine of b (fvad_vad_batch_run_device_part, _run_device_part_sized and _run_device_part_async); n_frames
// [n_sizes][n_streams], frames from sample first_sample on.  The blocking calls give the chunk RMS on the host (chunk_rms) and
// return with the results; the async call gives it on the device (d_chunk_rms) and returns once the part is queued on the
// context's second stream, behind everything the main stream holds at that moment.
int run_device_part(fvad_ctx* ctx, fvad_vad_batch* b, const float* d_band, size_t band_stride, const size_t* n_frames,
                    const float* chunk_rms, const float* d_chunk_rms, size_t rms_stride, const size_t* n_chunks, size_t chunk_size,
                    uint64_t first_sample, bool async, bool emit)
{
    const size_t S = b->n_streams, NC = b->cfgs.size(), C = b->n_channels, G = b->sizes.size();
    const size_t M = S * NC;
    std::vector<size_t> P; // each size's longest stream in the part: a stream with fewer frames of some size has ended
    if (const char* msg = frame_counts(b, n_frames, n_chunks, chunk_size, &P)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, msg);
    const size_t max_nf = *std::max_element(P.begin(), P.end());
    if (max_nf && (!d_band || !(async ? d_chunk_rms : chunk_rms))) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null argument");
    if (band_stride < max_nf) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "band_stride < frames of a stream");
    if (first_sample % chunk_size) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a part starts on a chunk boundary");
    for (size_t g = 0; g < G; ++g)
        if (first_sample % b->sizes[g]) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a part starts on a frame of every size");
    DevParts* dp = static_cast<DevParts*>(b->dev_parts.get());
    if (first_sample != 0) {
        if (!dp) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "no device part to continue (a host run or a one-shot device run came between)");
        if (dp->ctx != ctx) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "the parts of a run are on one context");
        if (first_sample != dp->next_sample) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a part starts where the previous one ended");
        for (size_t s = 0; s < S; ++s) {
            bool any = n_chunks[s] != 0;
            for (size_t g = 0; g < G; ++g) any = any || n_frames[g * S + s] != 0;
            if (dp->ended[s] && any) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "frames for a stream that has ended");
        }
    }
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    if (async)
        if (const int rc = part_stream(ctx, &st)) return rc;
    // The form of the run is chosen at its first part and kept: shared when the option asks for it, the launch is cooperative and
    // the part's bits fit the budget; a later part goes on in the form the state has
    if (!emit) {
        const bool shared = first_sample == 0 ? trigger_wanted(ctx, b, P) : dp->shared;
        if (shared)
            return run_shared_part(ctx, b, d_band, band_stride, n_frames, chunk_rms, d_chunk_rms, rms_stride, n_chunks, chunk_size, first_sample,
                                   async, P, st);
        if (first_sample == 0) { b->trig.reset(); b->trig_of.clear(); b->trigger_bytes = 0; }
    }

    // ---- host: the part's frame ratios (the blocking calls) and, for a fresh run, the configs' derived constants
    const size_t ratio_stride = std::max<size_t>(max_nf, 1);
    std::vector<float> ratio;
    if (!async) ratio = sized_ratios(b, n_frames, chunk_rms, rms_stride, n_chunks, chunk_size, first_sample, ratio_stride);
    if (first_sample == 0) { // fresh machines: the state of an earlier run is dropped
        b->dev_parts.reset();
        std::vector<VadMachineCfg> hc;
        uint32_t lt_max, st_max, cr_max;
        if (const int rc = derive_cfgs(ctx, b, &hc, &lt_max, &st_max, &cr_max)) return rc;
        std::unique_ptr<DevParts> fresh(new (std::nothrow) DevParts());
        if (!fresh) return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "device part state");
        dp = fresh.get();
        dp->device = ctx->device;
        dp->ctx = ctx;
        dp->lt_max = lt_max;
        dp->st_max = st_max;
        dp->cr_max = cr_max;
        dp->by_config = ctx->tune.vad_lane_map;
        dp->size_order = ctx->tune.vad_size_order;
        dp->emit = emit;
        // as fvad_vad_batch_run_device: the long-term rings in whole blocks of 64 slots plus one; the short-term and
        // channel-ratio rings in LDS when a workgroup's fit in 48 KB (their home between launches is `rings` either way)
        dp->rings_in_lds = (size_t)(st_max + cr_max) * 64 * sizeof(float) <= 48 * 1024;
        FVAD_HIP(ctx, dp->alloc(&dp->cfg, NC));
        FVAD_HIP(ctx, dp->alloc(&dp->lt, (((size_t)lt_max + 63) / 64 + 1) * 64 * M));
        FVAD_HIP(ctx, dp->alloc(&dp->rings, (size_t)(st_max + cr_max) * M));
        FVAD_HIP(ctx, dp->alloc(&dp->state, M));
        FVAD_HIP(ctx, dp->alloc(&dp->count, M));
        FVAD_HIP(ctx, dp->alloc(&dp->audit, M));
        FVAD_HIP(ctx, dp->alloc(&dp->stats, 2 * M));
        FVAD_HIP(ctx, dp->alloc(&dp->paused, 1));
        FVAD_HIP(ctx, hipMemcpyAsync(dp->cfg, hc.data(), NC * sizeof(VadMachineCfg), hipMemcpyHostToDevice, st));
        if (G > 1) { // the sized form's tables; the lane order is the first part's (the rings are laid out by it)
            const std::vector<uint64_t> sizes(b->sizes.begin(), b->sizes.end());
            dp->order = lane_order(b, dp->size_order);
            const std::vector<int>& order = dp->order;
            FVAD_HIP(ctx, dp->alloc(&dp->sizes, G));
            FVAD_HIP(ctx, dp->alloc(&dp->size_of, NC));
            FVAD_HIP(ctx, dp->alloc(&dp->lane_config, NC));
            FVAD_HIP(ctx, hipMemcpyAsync(dp->sizes, sizes.data(), G * sizeof(uint64_t), hipMemcpyHostToDevice, st));
            FVAD_HIP(ctx, hipMemcpyAsync(dp->size_of, b->size_of.data(), NC * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            FVAD_HIP(ctx, hipMemcpyAsync(dp->lane_config, order.data(), NC * sizeof(int), hipMemcpyHostToDevice, st));
        }
        dp->ended.assign(S, 0);
        dp->count_h.assign(M, 0);
        b->dev_parts = std::unique_ptr<void, DevPartsDeleter>(fresh.release(), DevPartsDeleter{free_dev_parts});
        for (auto& v : b->segs) std::vector<fvad_speech_segment>().swap(v);
    }
    b->machines.clear(); // a host part cannot go on from a device part
    b->state_on_device = true;
    const bool keep = b->keep_segments;
    dp->segs_on_device = dp->segs_on_device && !keep;
    dp->next_sample = UINT64_MAX; // (until this part has run: after an error the run starts again at sample 0)

    // ---- device: the part's per-call inputs
    std::unique_ptr<PartFlight> flight(new (std::nothrow) PartFlight());
    if (!flight) return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "device part");
    PartFlight& pf = *flight;
    pf.st = st;
    pf.keep = keep;
    pf.first_sample = first_sample;
    pf.P = P;
    pf.n_frames.assign(n_frames, n_frames + G * S);
    float* d_ratio = nullptr;
    long* d_nf = nullptr; // the frame counts, and behind them the chunk counts (the ratio kernel's)
    std::vector<long> nf_l(n_frames, n_frames + G * S);
    if (async) nf_l.insert(nf_l.end(), n_chunks, n_chunks + S);
    FVAD_HIP(ctx, pf.scratch.alloc(&d_ratio, G * S * ratio_stride));
    FVAD_HIP(ctx, pf.scratch.alloc(&d_nf, nf_l.size()));
    if (!async) FVAD_HIP(ctx, hipMemcpyAsync(d_ratio, ratio.data(), ratio.size() * sizeof(float), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(d_nf, nf_l.data(), nf_l.size() * sizeof(long), hipMemcpyHostToDevice, st));
    if (async) {
        // behind what the main stream holds now (the band sums and the RMS the part reads); nothing there waits for the part
        FVAD_HIP(ctx, hipEventRecord(ctx->part_ev, ctx->stream));
        FVAD_HIP(ctx, hipStreamWaitEvent(st, ctx->part_ev, 0));
        if (const int rc = device_ratios(ctx, b, dp->sizes, d_nf, d_chunk_rms, rms_stride, chunk_size, first_sample, d_ratio, ratio_stride, max_nf, st))
            return rc;
    }

    // Segment room: at most one segment per 4 frames (fvad_vad_batch_run_device), the largest bound over the sizes.  A part that
    // keeps its segments writes them from the start of the buffer (the earlier ones are on the host); otherwise the buffer holds
    // every segment since the first part.  The buffer has room for at least the part's bound or the one-shot's first room
    // (context option vad_seg_cap, else 512 MB over all machines), whichever is less; a machine that fills it stops before its
    // next frame, the room doubles (the contents kept, never past what the frames allow) and the part goes on from there.  So the
    // room follows the segments, not the length of the run.
    size_t most = 0;
    for (size_t g = 0; g < G; ++g)
        most = std::max(most, keep ? P[g] / 4 + 1 : (size_t)((first_sample / b->sizes[g] + P[g]) / 4 + 1));
    pf.most = most;
    const size_t room = ctx->tune.vad_seg_cap > 0 ? (size_t)ctx->tune.vad_seg_cap
                                                  : std::max<size_t>(256, (512u << 20) / sizeof(fvad_speech_segment) / M);
    const size_t first_room = std::min(max_nf / 4 + 1, room);
    if (!emit && dp->seg_cap < first_room) { // (emitting machines close no segment: no room)
        const int rc = grow_segs(ctx, dp, M, first_room, st);
        if (rc) return rc;
    }

    VadMachinesArgs& a = pf.a;
    a.cfgs = dp->cfg;
    a.n_configs = (int)NC;
    a.n_streams = (long)S;
    a.by_config = dp->by_config;
    a.n_channels = (int)C;
    a.n_machines = (long)M;
    a.n_lanes = (long)(S * C);
    a.band = d_band;
    a.band_stride = (long)band_stride;
    a.ratio = d_ratio;
    a.ratio_stride = (long)ratio_stride;
    a.n_frames = d_nf;
    a.fft_size = b->fft_size;
    a.lt_rings = dp->lt;
    a.rings = dp->rings;
    a.rings_in_lds = dp->rings_in_lds ? 1 : 0;
    a.st_max = (int)dp->st_max;
    a.cr_max = (int)dp->cr_max;
    a.seg_count = dp->count;
    a.audits = dp->audit;
    a.stats = dp->stats;
    a.resume = 1;
    a.fresh = first_sample == 0;
    a.rebase = keep;
    a.first_frame = first_sample / b->fft_size;
    a.state = dp->state;
    a.paused = dp->paused;
    if (G > 1) {
        a.sized = 1;
        a.sizes = dp->sizes;
        a.size_of = dp->size_of;
        a.lane_config = dp->lane_config;
        a.first_sample = first_sample;
    }
    // The averages' tables of the part (context option vad_avgs "table" with vad_chain "coop", within vad_avgs_max_bytes), filled
    // once on the part's stream before its first launch: a relaunch after a pause reads them again, and they do not follow the
    // homes, which every launch that ends rewrites.  Their history comes from the homes as the previous part left them.
    b->avgs_bytes = 0;
    if (avgs_wanted(ctx, b) && max_nf) {
        const AvgsPlan pl = plan_avgs(b, P, first_sample, dp->by_config, dp->order);
        if (pl.bytes() <= ctx->tune.vad_avgs_max_bytes) {
            FVAD_HIP(ctx, dp->grow(&dp->mv, &dp->mv_cap, pl.mv_elems));
            FVAD_HIP(ctx, dp->grow(&dp->st_tab, &dp->st_cap, pl.st_elems));
            FVAD_HIP(ctx, dp->grow(&dp->cr_tab, &dp->cr_cap, pl.cr_elems));
            if (const int rc = fill_avgs(ctx, b, pl, pf.scratch, dp->mv, dp->st_tab, dp->cr_tab, (long)max_nf, &a, st)) return rc;
            b->avgs_bytes = pl.bytes();
        }
    }
    if (emit) { // the bits of the part: per size [stream][word][machines of that size]
        const TrigPlan tp = plan_trigger(b, P);
        VadTrigKey* d_tk = nullptr;
        FVAD_HIP(ctx, pf.scratch.alloc(&d_tk, NC));
        FVAD_HIP(ctx, hipMemcpyAsync(d_tk, tp.keys.data(), NC * sizeof(VadTrigKey), hipMemcpyHostToDevice, st));
        FVAD_HIP(ctx, dp->grow(&dp->bits, &dp->bits_cap, tp.words));
        dp->trig_h = tp.keys;
        dp->nf_h.assign(n_frames, n_frames + G * S);
        a.emit = 1;
        a.bits = dp->bits;
        a.trig_keys = d_tk;
    }
    if (const int rc = launch_part(ctx, b, dp, pf)) return rc;
    if (emit) { // (the batch that owns this one finishes it: finish_part)
        dp->flight = std::move(flight);
        return FVAD_OK;
    }
    if (async) { // fvad_vad_batch_part_wait goes on from here
        dp->flight = std::move(flight);
        b->part_in_flight = true;
        return FVAD_OK;
    }
    return finish_part(ctx, b, dp, pf);
}

// The trigger batch of b (fvad_vad_batch::trig): an ordinary sweep batch of each key's first config, with b's own sizes and bands.
// The first config of a band, of a size or of an averages key is also the first config of its trigger key, so the representatives
// alone give b's sizes, bands and averages keys in b's order: the band blocks and frame counts b's caller passes are the trigger
// batch's too.  That is checked here, not assumed.
int make_trigger_batch(fvad_ctx* ctx, const fvad_vad_batch* b, std::unique_ptr<fvad_vad_batch>* out)
{
    std::unique_ptr<fvad_vad_batch> tb(new (std::nothrow) fvad_vad_batch());
    if (!tb) return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "trigger batch");
    const size_t K = b->trig_rep.size(), S = b->n_streams;
    tb->sample_rate = b->sample_rate; tb->n_channels = b->n_channels; tb->fft_size = b->fft_size; tb->n_streams = S;
    tb->sizes = b->sizes;
    tb->bins = b->bins;
    tb->size_of_band = b->size_of_band;
    for (const uint32_t c : b->trig_rep) {
        tb->cfgs.push_back(b->cfgs[c]);
        tb->band_of.push_back(b->band_of[c]);
        tb->size_of.push_back(b->size_of[c]);
    }
    tb->segs.resize(S * K);
    tb->audits.resize(S * K);
    tb->exact_evals.assign(S * K, 0);
    tb->lazy_pushes.assign(S * K, 0);
    tb->keep_segments = false;
    if (derive_avg_keys(tb.get()) || derive_trigger_keys(tb.get())) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "ring length out of range");
    bool spans = tb->st_keys == b->st_keys && tb->cr_keys == b->cr_keys && tb->trig_rep.size() == K;
    std::vector<uint8_t> band_seen(b->bins.size() / 2, 0), size_seen(b->sizes.size(), 0);
    for (size_t k = 0; k < K; ++k) { band_seen[tb->band_of[k]] = 1; size_seen[tb->size_of[k]] = 1; }
    for (const uint8_t x : band_seen) spans = spans && x;
    for (const uint8_t x : size_seen) spans = spans && x;
    if (!spans) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "internal: trigger keys: the representatives do not span the batch's bands, sizes and averages keys");
    *out = std::move(tb);
    return FVAD_OK;
}

// a stream's lanes in the finishing kernel: configs of one trigger machine side by side (first-seen order within it)
std::vector<int> finish_order(const std::vector<uint32_t>& trig_of)
{
    std::vector<int> o(trig_of.size());
    for (size_t c = 0; c < o.size(); ++c) o[c] = (int)c;
    std::stable_sort(o.begin(), o.end(), [&](int x, int y) { return trig_of[(size_t)x] < trig_of[(size_t)y]; });
    return o;
}

// the state of a shared batch's finishing machines: what the finishing kernel and the retain gather touch, no rings
int alloc_shared_state(fvad_ctx* ctx, const fvad_vad_batch* b, const std::vector<uint32_t>& trig_of, DevParts* dp, hipStream_t st)
{
    const size_t S = b->n_streams, NC = b->cfgs.size(), G = b->sizes.size(), M = S * NC;
    std::vector<VadMachineCfg> hc;
    uint32_t lt_max, st_max, cr_max;
    if (const int rc = derive_cfgs(ctx, b, &hc, &lt_max, &st_max, &cr_max)) return rc;
    dp->shared = true;
    dp->lt_max = dp->st_max = dp->cr_max = 0;
    FVAD_HIP(ctx, dp->alloc(&dp->cfg, NC));
    FVAD_HIP(ctx, dp->alloc(&dp->state, M));
    FVAD_HIP(ctx, dp->alloc(&dp->count, M));
    FVAD_HIP(ctx, dp->alloc(&dp->audit, M)); // (gathered by a retain with the rest; the results' audits are the trigger batch's)
    FVAD_HIP(ctx, dp->alloc(&dp->stats, 2 * M));
    FVAD_HIP(ctx, dp->alloc(&dp->paused, 1));
    FVAD_HIP(ctx, dp->alloc(&dp->trig_of, NC));
    FVAD_HIP(ctx, dp->alloc(&dp->finish_order, NC));
    const std::vector<int> order = finish_order(trig_of);
    FVAD_HIP(ctx, hipMemcpyAsync(dp->cfg, hc.data(), NC * sizeof(VadMachineCfg), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(dp->trig_of, trig_of.data(), NC * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(dp->finish_order, order.data(), NC * sizeof(int), hipMemcpyHostToDevice, st));
    if (G > 1) {
        const std::vector<uint64_t> sizes(b->sizes.begin(), b->sizes.end());
        FVAD_HIP(ctx, dp->alloc(&dp->sizes, G));
        FVAD_HIP(ctx, dp->alloc(&dp->size_of, NC));
        FVAD_HIP(ctx, hipMemcpyAsync(dp->sizes, sizes.data(), G * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        FVAD_HIP(ctx, hipMemcpyAsync(dp->size_of, b->size_of.data(), NC * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    FVAD_HIP(ctx, hipStreamSynchronize(st)); // (the host vectors above end here)
    return FVAD_OK;
}

// A part in the shared-trigger form (run_device_part has checked the arguments): the trigger batch's part -- the ratios, the
// tables if selected and the emitting machines -- and behind it on the same stream the finishing kernel over b's configs.
int run_shared_part(fvad_ctx* ctx, fvad_vad_batch* b, const float* d_band, size_t band_stride, const size_t* n_frames,
                    const float* chunk_rms, const float* d_chunk_rms, size_t rms_stride, const size_t* n_chunks, size_t chunk_size,
                    uint64_t first_sample, bool async, const std::vector<size_t>& P, hipStream_t st)
{
    const size_t S = b->n_streams, NC = b->cfgs.size(), G = b->sizes.size(), M = S * NC;
    const size_t max_nf = *std::max_element(P.begin(), P.end());
    DevParts* dp = static_cast<DevParts*>(b->dev_parts.get());
    if (first_sample == 0) {
        b->dev_parts.reset();
        b->trig.reset();
        std::unique_ptr<fvad_vad_batch> tb;
        if (const int rc = make_trigger_batch(ctx, b, &tb)) return rc;
        std::unique_ptr<DevParts> fresh(new (std::nothrow) DevParts());
        if (!fresh) return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "device part state");
        dp = fresh.get();
        dp->device = ctx->device;
        dp->ctx = ctx;
        if (const int rc = alloc_shared_state(ctx, b, b->trig_key, dp, st)) return rc;
        dp->ended.assign(S, 0);
        dp->count_h.assign(M, 0);
        b->dev_parts = std::unique_ptr<void, DevPartsDeleter>(fresh.release(), DevPartsDeleter{free_dev_parts});
        b->trig = std::move(tb);
        b->trig_of = b->trig_key; // (a fresh trigger batch is in first-seen key order)
        for (auto& v : b->segs) std::vector<fvad_speech_segment>().swap(v);
    }
    fvad_vad_batch* tb = b->trig.get();
    b->machines.clear();
    b->state_on_device = true;
    const bool keep = b->keep_segments;
    dp->segs_on_device = dp->segs_on_device && !keep;
    dp->next_sample = UINT64_MAX;

    // ---- stage one: the trigger batch's part, left in flight on st
    if (const int rc = run_device_part(ctx, tb, d_band, band_stride, n_frames, chunk_rms, d_chunk_rms, rms_stride, n_chunks, chunk_size,
                                       first_sample, async, true))
        return rc;
    DevParts* tdp = static_cast<DevParts*>(tb->dev_parts.get());
    const PartFlight& tpf = *tdp->flight;
    b->trig_machine_launches += 1;
    b->chain_form = tb->chain_form;
    b->avgs_form = tb->avgs_form;
    b->avgs_bytes = tb->avgs_bytes;
    b->trigger_bytes = tdp->bits_cap ? trigger_bits_bytes(b, P) : 0;

    // ---- stage two: the finishing kernel; segment room as in the per-config form
    std::unique_ptr<PartFlight> flight(new (std::nothrow) PartFlight());
    if (!flight) return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "device part");
    PartFlight& pf = *flight;
    pf.st = st;
    pf.keep = keep;
    pf.first_sample = first_sample;
    pf.P = P;
    pf.n_frames.assign(n_frames, n_frames + G * S);
    pf.finish = true;
    size_t most = 0;
    for (size_t g = 0; g < G; ++g)
        most = std::max(most, keep ? P[g] / 4 + 1 : (size_t)((first_sample / b->sizes[g] + P[g]) / 4 + 1));
    pf.most = most;
    const size_t room = ctx->tune.vad_seg_cap > 0 ? (size_t)ctx->tune.vad_seg_cap
                                                  : std::max<size_t>(256, (512u << 20) / sizeof(fvad_speech_segment) / M);
    const size_t first_room = std::min(max_nf / 4 + 1, room);
    if (dp->seg_cap < first_room)
        if (const int rc = grow_segs(ctx, dp, M, first_room, st)) return rc;
    VadMachinesArgs& a = pf.a;
    a.cfgs = dp->cfg;
    a.n_configs = (int)NC;
    a.n_streams = (long)S;
    a.n_machines = (long)M;
    a.ratio = tpf.a.ratio;
    a.ratio_stride = tpf.a.ratio_stride;
    a.n_frames = tpf.a.n_frames;
    a.fft_size = b->fft_size;
    a.seg_count = dp->count;
    a.resume = 1;
    a.fresh = first_sample == 0;
    a.rebase = keep;
    a.first_frame = first_sample / b->fft_size;
    a.state = dp->state;
    a.paused = dp->paused;
    if (G > 1) {
        a.sized = 1;
        a.sizes = dp->sizes;
        a.size_of = dp->size_of;
        a.first_sample = first_sample;
    }
    a.lane_config = dp->finish_order;
    a.bits = tdp->bits;
    a.trig_keys = tpf.a.trig_keys;
    a.trig_of = dp->trig_of;
    if (const int rc = launch_part(ctx, b, dp, pf)) return rc;
    if (async) {
        dp->flight = std::move(flight);
        b->part_in_flight = true;
        return FVAD_OK;
    }
    return finish_part(ctx, b, dp, pf);
}

// The place (kernels_vad.hip: a lane's rings) of machine (s, c) in a batch of S streams and NC configs run with lane map by_config
// and lane order `order` (empty: lane j of a stream runs config j)
long place_of(size_t s, size_t c, size_t S, size_t NC, int by_config, const std::vector<int>& order)
{
    if (by_config) return (long)(c * S + s);
    if (order.empty()) return (long)(s * NC + c);
    const size_t j = (size_t)(std::find(order.begin(), order.end(), (int)c) - order.begin());
    return (long)(s * NC + j);
}

// fvad_vad_batch_retain_configs on a batch with device part state: nb (retain_stage's) gets the kept machines' state in buffers of
// its own size, gathered on the device (kernels_vadretain.hip); b's state is left as it is (retain_commit frees it)
int retain_device(fvad_ctx* ctx, const fvad_vad_batch* b, fvad_vad_batch* nb, const uint32_t* keep, size_t n_keep)
{
    const DevParts* dp = static_cast<const DevParts*>(b->dev_parts.get());
    const size_t S = b->n_streams, NC = b->cfgs.size(), G = nb->sizes.size();
    const size_t M = S * n_keep, M_old = S * NC;
    std::vector<VadMachineCfg> hc;
    uint32_t lt_max, st_max, cr_max;
    if (const int rc = derive_cfgs(ctx, nb, &hc, &lt_max, &st_max, &cr_max)) return rc;
    if (dp->shared) lt_max = st_max = cr_max = 0; // (finishing machines have no rings: only the machines' gather runs)
    // (the survivors' rings are never longer than the batch's were: the new rows are a prefix of the old)
    if (lt_max > dp->lt_max || st_max > dp->st_max || cr_max > dp->cr_max) return set_err(ctx, FVAD_ERR_HIP, "retain: rings grew");
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    std::unique_ptr<DevParts> fresh(new (std::nothrow) DevParts());
    if (!fresh) return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "device part state");
    DevParts* np = fresh.get();
    try {
        np->ended = dp->ended;
        np->count_h.resize(M);
        for (size_t s = 0; s < S; ++s)
            for (size_t c = 0; c < n_keep; ++c) np->count_h[s * n_keep + c] = dp->count_h[s * NC + keep[c]];
        if (G > 1 && !dp->shared) np->order = lane_order(nb, dp->size_order);
    } catch (const std::bad_alloc&) {
        return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "device part state");
    }
    np->device = dp->device;
    np->ctx = dp->ctx;
    np->by_config = dp->by_config;
    np->size_order = dp->size_order;
    np->lt_max = lt_max;
    np->st_max = st_max;
    np->cr_max = cr_max;
    np->rings_in_lds = (size_t)(st_max + cr_max) * 64 * sizeof(float) <= 48 * 1024; // (as run_device_part decides it)
    np->next_sample = dp->next_sample;
    np->segs_on_device = dp->segs_on_device;
    np->shared = dp->shared;
    np->emit = dp->emit;
    const size_t lt_rows = dp->shared ? 0 : ((size_t)lt_max + 63) / 64 * 16 + 16, old_lt_rows = ((size_t)dp->lt_max + 63) / 64 * 16 + 16;
    FVAD_HIP(ctx, np->alloc(&np->cfg, n_keep));
    if (!dp->shared) {
        FVAD_HIP(ctx, np->alloc(&np->lt, lt_rows * 4 * M));
        FVAD_HIP(ctx, np->alloc(&np->rings, (size_t)(st_max + cr_max) * M));
    } else { // the finishing kernel's maps, by the survivors' trigger machines (nb->trig_of: fvad_vad_batch_retain_configs)
        const std::vector<int> order = finish_order(nb->trig_of);
        FVAD_HIP(ctx, np->alloc(&np->trig_of, n_keep));
        FVAD_HIP(ctx, np->alloc(&np->finish_order, n_keep));
        FVAD_HIP(ctx, hipMemcpyAsync(np->trig_of, nb->trig_of.data(), n_keep * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        FVAD_HIP(ctx, hipMemcpyAsync(np->finish_order, order.data(), n_keep * sizeof(int), hipMemcpyHostToDevice, st));
        FVAD_HIP(ctx, hipStreamSynchronize(st));
    }
    FVAD_HIP(ctx, np->alloc(&np->state, M));
    FVAD_HIP(ctx, np->alloc(&np->count, M));
    FVAD_HIP(ctx, np->alloc(&np->audit, M));
    FVAD_HIP(ctx, np->alloc(&np->stats, 2 * M));
    FVAD_HIP(ctx, np->alloc(&np->paused, 1));
    FVAD_HIP(ctx, hipMalloc((void**)&np->segs, std::max<size_t>(dp->seg_cap * M, 1) * sizeof(fvad_speech_segment)));
    np->seg_cap = dp->seg_cap;
    FVAD_HIP(ctx, hipMemcpyAsync(np->cfg, hc.data(), n_keep * sizeof(VadMachineCfg), hipMemcpyHostToDevice, st));
    if (G > 1) {
        const std::vector<uint64_t> sizes(nb->sizes.begin(), nb->sizes.end());
        FVAD_HIP(ctx, np->alloc(&np->sizes, G));
        FVAD_HIP(ctx, np->alloc(&np->size_of, n_keep));
        FVAD_HIP(ctx, hipMemcpyAsync(np->sizes, sizes.data(), G * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        FVAD_HIP(ctx, hipMemcpyAsync(np->size_of, nb->size_of.data(), n_keep * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (!dp->shared) {
            FVAD_HIP(ctx, np->alloc(&np->lane_config, n_keep));
            FVAD_HIP(ctx, hipMemcpyAsync(np->lane_config, np->order.data(), n_keep * sizeof(int), hipMemcpyHostToDevice, st));
        }
    }
    // new place -> old place, new machine -> old machine (the lane map is the first part's; the lane orders are each batch's own)
    std::vector<long> place_src(M), machine_src(M);
    for (size_t s = 0; s < S; ++s)
        for (size_t c = 0; c < n_keep; ++c) {
            machine_src[s * n_keep + c] = (long)(s * NC + keep[c]);
            place_src[(size_t)place_of(s, c, S, n_keep, dp->by_config, np->order)] = place_of(s, keep[c], S, NC, dp->by_config, dp->order);
        }
    DevScratch scratch;
    long *d_place = nullptr, *d_machine = nullptr;
    FVAD_HIP(ctx, scratch.alloc(&d_place, M));
    FVAD_HIP(ctx, scratch.alloc(&d_machine, M));
    FVAD_HIP(ctx, hipMemcpyAsync(d_place, place_src.data(), M * sizeof(long), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(d_machine, machine_src.data(), M * sizeof(long), hipMemcpyHostToDevice, st));
    VadRetainArgs a{};
    a.n_places = (long)M;
    a.old_places = (long)M_old;
    a.place_src = d_place;
    a.machine_src = d_machine;
    a.lt_src = reinterpret_cast<const float4*>(dp->lt);
    a.lt_dst = reinterpret_cast<float4*>(np->lt);
    a.lt_rows = (long)std::min(lt_rows, old_lt_rows);
    a.rings_src = dp->rings;
    a.rings_dst = np->rings;
    a.st = dp->shared ? 0 : (int)st_max;
    a.cr = dp->shared ? 0 : (int)cr_max;
    a.old_st = (int)dp->st_max;
    a.state_src = dp->state;
    a.state_dst = np->state;
    a.count_src = dp->count;
    a.count_dst = np->count;
    a.audit_src = dp->audit;
    a.audit_dst = np->audit;
    a.stats_src = dp->stats;
    a.stats_dst = np->stats;
    a.segs_src = dp->segs;
    a.segs_dst = np->segs;
    a.seg_cap = (uint32_t)dp->seg_cap;
    time_begin(ctx, "vad_retain");
    const int e = fvad_launch_vad_retain(a, st);
    time_end(ctx);
    if (e != (int)hipSuccess) return hip_fail(ctx, (hipError_t)e, "fvad_launch_vad_retain");
    FVAD_HIP(ctx, hipStreamSynchronize(st)); // (before the old state and the maps are freed)
    nb->dev_parts = std::unique_ptr<void, DevPartsDeleter>(fresh.release(), DevPartsDeleter{free_dev_parts});
    return FVAD_OK;
}

} // namespace

extern "C" {

int fvad_vad_batch_run_device(fvad_ctx* ctx, fvad_vad_batch* b, const float* d_band, size_t band_stride, const size_t* n_frames,
                              const float* chunk_rms, size_t rms_stride, const size_t* n_chunks, size_t chunk_size)
{
    if (!ctx) return no_ctx();
    if (!b || !d_band || !n_frames || !n_chunks || !chunk_rms || chunk_size == 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null argument");
    if (b->part_in_flight) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a device part is in flight: fvad_vad_batch_part_wait first");
    if (b->sizes.size() != 1) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "several frame sizes: fvad_vad_batch_run_device_sized");
    return run_device(ctx, b, d_band, band_stride, n_frames, chunk_rms, rms_stride, n_chunks, chunk_size);
}

int fvad_vad_batch_run_device_sized(fvad_ctx* ctx, fvad_vad_batch* b, const float* d_band, size_t band_stride, const size_t* n_frames,
                                    const float* chunk_rms, size_t rms_stride, const size_t* n_chunks, size_t chunk_size)
{
    if (!ctx) return no_ctx();
    if (!b || !d_band || !n_frames || !n_chunks || !chunk_rms || chunk_size == 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null argument");
    if (b->part_in_flight) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a device part is in flight: fvad_vad_batch_part_wait first");
    return run_device(ctx, b, d_band, band_stride, n_frames, chunk_rms, rms_stride, n_chunks, chunk_size);
}

int fvad_vad_batch_chain_form(const fvad_vad_batch* b, int* form)
{
    if (!b || !form) return FVAD_ERR_INVALID_ARGUMENT;
    *form = b->chain_form;
    return FVAD_OK;
}

int fvad_vad_batch_avgs_form(const fvad_vad_batch* b, int* form)
{
    if (!b || !form) return FVAD_ERR_INVALID_ARGUMENT;
    *form = b->avgs_form;
    return FVAD_OK;
}

size_t fvad_vad_batch_avgs_bytes(const fvad_vad_batch* b) { return b ? b->avgs_bytes : 0; }

int fvad_vad_batch_trigger_form(const fvad_vad_batch* b, int* form)
{
    if (!b || !form) return FVAD_ERR_INVALID_ARGUMENT;
    *form = b->trigger_form;
    return FVAD_OK;
}

size_t fvad_vad_batch_trigger_bytes(const fvad_vad_batch* b) { return b ? b->trigger_bytes : 0; }

int fvad_vad_batch_trigger_launches(const fvad_vad_batch* b, uint64_t* machines, uint64_t* finish)
{
    if (!b) return FVAD_ERR_INVALID_ARGUMENT;
    if (machines) *machines = b->trig_machine_launches;
    if (finish) *finish = b->trig_finish_launches;
    return FVAD_OK;
}

int fvad_vad_batch_trigger_bits(fvad_ctx* ctx, const fvad_vad_batch* b, uint64_t* out, size_t row_stride)
{
    if (!ctx) return no_ctx();
    if (!b || !out) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null argument");
    if (b->part_in_flight) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a device part is in flight: fvad_vad_batch_part_wait first");
    const fvad_vad_batch* tb = b->trig.get();
    const DevParts* tdp = tb ? static_cast<const DevParts*>(tb->dev_parts.get()) : nullptr;
    if (!tdp || tdp->trig_h.empty() || b->trig_of.size() != b->cfgs.size())
        return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "no bits: the last device launch was not a shared part");
    if (tdp->ctx != ctx) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "the parts ran on another context");
    const size_t S = b->n_streams, K = b->trig_rep.size();
    size_t total = 0;
    for (const VadTrigKey& k : tdp->trig_h) total = std::max(total, (size_t)k.base + ((S * k.words ? S * k.words - 1 : 0)) * k.nk + 1);
    for (const VadTrigKey& k : tdp->trig_h)
        if (k.words > row_stride) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "row_stride < words of a stream");
    total = std::min(total, tdp->bits_cap);
    hipSetDevice(ctx->device);
    std::vector<unsigned long long> h(total);
    if (total) FVAD_HIP(ctx, hipMemcpy(h.data(), tdp->bits, total * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t j = 0; j < K; ++j) {
        const size_t t = b->trig_of[b->trig_rep[j]];
        const VadTrigKey& k = tdp->trig_h[t];
        for (size_t s = 0; s < S; ++s) {
            const size_t nw = finish_words(tdp->nf_h[(size_t)tb->size_of[t] * S + s]); // (the stream's own words: the rest were not written)
            for (size_t w = 0; w < row_stride; ++w)
                out[(j * S + s) * row_stride + w] = w < nw ? h[(size_t)k.base + (s * k.words + w) * k.nk] : 0;
        }
    }
    return FVAD_OK;
}

int fvad_vad_batch_averages_device(fvad_ctx* ctx, const fvad_vad_batch* b, const float* d_band, size_t band_stride, const size_t* n_frames,
                                   const float* chunk_rms, size_t rms_stride, const size_t* n_chunks, size_t chunk_size,
                                   uint64_t first_sample, double* st_avg, double* cr_avg, size_t row_stride)
{
    if (!ctx) return no_ctx();
    if (!b || !n_frames || !n_chunks || chunk_size == 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null argument");
    if (b->part_in_flight) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a device part is in flight: fvad_vad_batch_part_wait first");
    const size_t S = b->n_streams, NC = b->cfgs.size(), C = b->n_channels, G = b->sizes.size();
    std::vector<size_t> P;
    if (const char* msg = frame_counts(b, n_frames, n_chunks, chunk_size, &P)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, msg);
    const size_t max_nf = *std::max_element(P.begin(), P.end());
    if (max_nf == 0) return FVAD_OK;
    if (!d_band || !chunk_rms || !st_avg || !cr_avg) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null argument");
    if (band_stride < max_nf || row_stride < max_nf) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a stride < frames of a stream");
    if (first_sample % chunk_size) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a part starts on a chunk boundary");
    for (size_t g = 0; g < G; ++g)
        if (first_sample % b->sizes[g]) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a part starts on a frame of every size");
    if (!avgs_wanted_shape(b)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "more streams, bands or keys than the tables' kernels take");
    const DevParts* dp = static_cast<const DevParts*>(b->dev_parts.get());
    if (first_sample != 0) { // the history is the part state's: the rings' homes as the last part left them
        if (!dp) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "no device part state to read the earlier frames from");
        if (dp->ctx != ctx) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "the parts of a run are on one context");
        if (first_sample != dp->next_sample) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a part starts where the previous one ended");
    }
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const size_t ratio_stride = max_nf;
    const std::vector<float> ratio = sized_ratios(b, n_frames, chunk_rms, rms_stride, n_chunks, chunk_size, first_sample, ratio_stride);
    const std::vector<long> nf_l(n_frames, n_frames + G * S);
    std::vector<int> order;
    if (first_sample != 0) order = dp->order;
    const int by_config = first_sample != 0 ? dp->by_config : ctx->tune.vad_lane_map;
    const AvgsPlan pl = plan_avgs(b, P, first_sample, by_config, order);
    DevScratch scratch;
    float *d_ratio = nullptr, *d_mv = nullptr;
    long* d_nf = nullptr;
    double *d_st = nullptr, *d_cr = nullptr;
    FVAD_HIP(ctx, scratch.alloc(&d_ratio, ratio.size()));
    FVAD_HIP(ctx, scratch.alloc(&d_nf, nf_l.size()));
    FVAD_HIP(ctx, scratch.alloc(&d_mv, pl.mv_elems));
    FVAD_HIP(ctx, scratch.alloc(&d_st, pl.st_elems));
    FVAD_HIP(ctx, scratch.alloc(&d_cr, pl.cr_elems));
    FVAD_HIP(ctx, hipMemcpyAsync(d_ratio, ratio.data(), ratio.size() * sizeof(float), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(d_nf, nf_l.data(), nf_l.size() * sizeof(long), hipMemcpyHostToDevice, st));
    VadMachinesArgs a{}; // (only what fill_avgs reads of a launch)
    a.n_configs = (int)NC;
    a.n_streams = (long)S;
    a.by_config = by_config;
    a.n_channels = (int)C;
    a.n_machines = (long)(S * NC);
    a.n_lanes = (long)(S * C);
    a.band = d_band;
    a.band_stride = (long)band_stride;
    a.ratio = d_ratio;
    a.ratio_stride = (long)ratio_stride;
    a.n_frames = d_nf;
    a.rings = first_sample != 0 ? dp->rings : nullptr;
    a.st_max = first_sample != 0 ? (int)dp->st_max : 0;
    if (const int rc = fill_avgs(ctx, b, pl, scratch, d_mv, d_st, d_cr, (long)max_nf, &a, st)) return rc;
    std::vector<double> h_st(pl.st_elems), h_cr(pl.cr_elems);
    FVAD_HIP(ctx, hipMemcpyAsync(h_st.data(), d_st, h_st.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    FVAD_HIP(ctx, hipMemcpyAsync(h_cr.data(), d_cr, h_cr.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    FVAD_HIP(ctx, hipStreamSynchronize(st));
    FVAD_HIP(ctx, hipGetLastError());
    auto gather = [&](const std::vector<VadAvgKey>& keys, const std::vector<double>& tab, double* out) {
        for (size_t j = 0; j < keys.size(); ++j) {
            const VadAvgKey& k = keys[j];
            for (size_t s = 0; s < S; ++s)
                for (size_t f = 0; f < n_frames[k.size * S + s]; ++f)
                    out[(j * S + s) * row_stride + f] = tab[(size_t)k.base + (s * P[k.size] + f) * k.nk];
        }
    };
    gather(pl.st, h_st, st_avg);
    gather(pl.cr, h_cr, cr_avg);
    return FVAD_OK;
}

size_t fvad_vad_batch_device_bytes(const fvad_vad_batch* b)
{
    if (!b) return 0;
    const DevParts* dp = static_cast<const DevParts*>(b->dev_parts.get());
    const size_t own = dp ? dp->bytes + dp->table_bytes() + dp->seg_cap * b->n_streams * b->cfgs.size() * sizeof(fvad_speech_segment) : 0;
    // a shared run: the trigger machines and their bits (after a one-shot run the bits alone are still held)
    return own + (b->trig ? fvad_vad_batch_device_bytes(b->trig.get()) : 0);
}

int fvad_vad_batch_run_device_part(fvad_ctx* ctx, fvad_vad_batch* b, const float* d_band, size_t band_stride, const size_t* n_frames,
                                   const float* chunk_rms, size_t rms_stride, const size_t* n_chunks, size_t chunk_size,
                                   uint64_t first_frame)
{
    if (!ctx) return no_ctx();
    if (!b || !n_frames || !n_chunks || chunk_size == 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null argument");
    if (b->part_in_flight) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a device part is in flight: fvad_vad_batch_part_wait first");
    if (b->sizes.size() != 1) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "several frame sizes: fvad_vad_batch_run_device_part_sized");
    if (first_frame > UINT64_MAX / b->fft_size) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "first_frame out of range");
    return run_device_part(ctx, b, d_band, band_stride, n_frames, chunk_rms, nullptr, rms_stride, n_chunks, chunk_size, first_frame * b->fft_size, false);
}

int fvad_vad_batch_run_device_part_sized(fvad_ctx* ctx, fvad_vad_batch* b, const float* d_band, size_t band_stride, const size_t* n_frames,
                                         const float* chunk_rms, size_t rms_stride, const size_t* n_chunks, size_t chunk_size,
                                         uint64_t first_sample)
{
    if (!ctx) return no_ctx();
    if (!b || !n_frames || !n_chunks || chunk_size == 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null argument");
    if (b->part_in_flight) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a device part is in flight: fvad_vad_batch_part_wait first");
    return run_device_part(ctx, b, d_band, band_stride, n_frames, chunk_rms, nullptr, rms_stride, n_chunks, chunk_size, first_sample, false);
}

int fvad_vad_batch_run_device_part_async(fvad_ctx* ctx, fvad_vad_batch* b, const float* d_band, size_t band_stride, const size_t* n_frames,
                                         const float* d_chunk_rms, size_t rms_stride, const size_t* n_chunks, size_t chunk_size,
                                         uint64_t first_sample)
{
    if (!ctx) return no_ctx();
    if (!b || !n_frames || !n_chunks || chunk_size == 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null argument");
    if (b->part_in_flight) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a device part is in flight: fvad_vad_batch_part_wait first");
    return run_device_part(ctx, b, d_band, band_stride, n_frames, nullptr, d_chunk_rms, rms_stride, n_chunks, chunk_size, first_sample, true);
}

int fvad_vad_batch_part_wait(fvad_ctx* ctx, fvad_vad_batch* b)
{
    if (!b) return ctx ? set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null batch") : FVAD_ERR_INVALID_ARGUMENT;
    if (!b->part_in_flight) return FVAD_OK;
    if (!ctx) return no_ctx();
    DevParts* dp = static_cast<DevParts*>(b->dev_parts.get());
    if (dp->ctx != ctx) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "the part runs on another context");
    hipSetDevice(ctx->device);
    const std::unique_ptr<PartFlight> flight = std::move(dp->flight); // (its inputs are freed when the part is done, either way)
    b->part_in_flight = false;
    const int rc = finish_part(ctx, b, dp, *flight);
    if (rc) hipStreamSynchronize(flight->st);
    return rc;
}

int fvad_vad_batch_frame_ratios_device(fvad_ctx* ctx, const fvad_vad_batch* b, const float* d_chunk_rms, size_t rms_stride,
                                       const size_t* n_frames, const size_t* n_chunks, size_t chunk_size, uint64_t first_sample,
                                       float* d_ratio, size_t ratio_stride)
{
    if (!ctx) return no_ctx();
    if (!b || !n_frames || !n_chunks || chunk_size == 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null argument");
    const size_t S = b->n_streams, G = b->sizes.size();
    std::vector<size_t> P;
    if (const char* msg = frame_counts(b, n_frames, n_chunks, chunk_size, &P)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, msg);
    const size_t max_nf = *std::max_element(P.begin(), P.end());
    if (max_nf == 0) return FVAD_OK;
    if (!d_chunk_rms || !d_ratio) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null argument");
    if (ratio_stride < max_nf) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "ratio_stride < frames of a stream");
    if (first_sample % chunk_size) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a part starts on a chunk boundary");
    for (size_t g = 0; g < G; ++g)
        if (first_sample % b->sizes[g]) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a part starts on a frame of every size");
    for (size_t s = 0; s < S; ++s)
        if (n_chunks[s] > rms_stride) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "rms_stride < chunks of a stream");
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    DevScratch scratch;
    uint64_t* d_sizes = nullptr;
    long* d_counts = nullptr;
    const std::vector<uint64_t> sizes(b->sizes.begin(), b->sizes.end());
    std::vector<long> counts(n_frames, n_frames + G * S);
    counts.insert(counts.end(), n_chunks, n_chunks + S);
    FVAD_HIP(ctx, scratch.alloc(&d_sizes, G));
    FVAD_HIP(ctx, scratch.alloc(&d_counts, counts.size()));
    FVAD_HIP(ctx, hipMemcpyAsync(d_sizes, sizes.data(), G * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    FVAD_HIP(ctx, hipMemcpyAsync(d_counts, counts.data(), counts.size() * sizeof(long), hipMemcpyHostToDevice, st));
    if (const int rc = device_ratios(ctx, b, d_sizes, d_counts, d_chunk_rms, rms_stride, chunk_size, first_sample, d_ratio, ratio_stride, max_nf, st))
        return rc;
    FVAD_HIP(ctx, hipStreamSynchronize(st));
    FVAD_HIP(ctx, hipGetLastError());
    return FVAD_OK;
}

int fvad_vad_batch_score_device(fvad_ctx* ctx, fvad_vad_batch* b)
{
    if (!ctx) return no_ctx();
    if (!b) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "null batch");
    if (b->part_in_flight) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "a device part is in flight: fvad_vad_batch_part_wait first");
    const DevParts* dp = static_cast<const DevParts*>(b->dev_parts.get());
    if (!b->has_refs) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "no references to score against");
    if (!dp) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "no device parts run");
    if (dp->ctx != ctx) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "the parts ran on another context");
    if (!dp->segs_on_device) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "the segments are on the host (a part kept them): fvad_vad_batch_score");
    hipSetDevice(ctx->device);
    std::vector<fvad_single_stats> scores;
    const int rc = score_on_device(ctx, b, dp->segs, dp->count, dp->seg_cap, &scores);
    if (rc) return rc;
    b->scores = std::move(scores);
    b->scored = true;
    return FVAD_OK;
}

int fvad_vad_batch_retain_configs(fvad_ctx* ctx, fvad_vad_batch* b, const uint32_t* keep, size_t n_keep)
{
    auto fail = [&](int rc, const char* msg) { return ctx ? set_err(ctx, rc, msg) : rc; };
    if (!b || !keep) return fail(FVAD_ERR_INVALID_ARGUMENT, "null argument");
    if (b->part_in_flight) return fail(FVAD_ERR_INVALID_ARGUMENT, "a device part is in flight: fvad_vad_batch_part_wait first");
    const DevParts* dp = static_cast<const DevParts*>(b->dev_parts.get());
    if (dp && dp->ctx != ctx) return fail(FVAD_ERR_INVALID_ARGUMENT, "the batch's device parts ran on another context");
    std::unique_ptr<fvad_vad_batch> nb(new (std::nothrow) fvad_vad_batch());
    if (!nb) return fail(FVAD_ERR_ALLOC_FAILED, "retain");
    if (const int rc = retain_stage(b, keep, n_keep, nb.get()))
        return fail(rc, rc == FVAD_ERR_ALLOC_FAILED ? "retain" : "keep: a strictly increasing list of config indices, not empty");
    if (dp && dp->shared) {
        // A shared run: the trigger machines are retained to the survivors' keys with the same gather (their rings shrink as
        // ever), then the finishing state config by config.  The trigger batch keeps its own order (the old one, thinned out):
        // the keys fvad_vad_batch_trigger_keys reports are first-seen over the survivors, trig_of maps between the two.
        const fvad_vad_batch* tb = b->trig.get();
        std::vector<uint32_t> keep_t;
        for (size_t c = 0; c < n_keep; ++c) keep_t.push_back(b->trig_of[keep[c]]);
        std::sort(keep_t.begin(), keep_t.end());
        keep_t.erase(std::unique(keep_t.begin(), keep_t.end()), keep_t.end());
        std::unique_ptr<fvad_vad_batch> ntb(new (std::nothrow) fvad_vad_batch());
        if (!ntb) return fail(FVAD_ERR_ALLOC_FAILED, "retain");
        if (const int rc = retain_stage(tb, keep_t.data(), keep_t.size(), ntb.get())) return fail(rc, "retain: trigger batch");
        // the trigger batch numbers sizes and bands as the batch does (the caller's band blocks and frame counts are the batch's)
        nb->trig_of.resize(n_keep);
        ntb->sizes = nb->sizes;
        ntb->bins = nb->bins;
        ntb->size_of_band = nb->size_of_band;
        ntb->fft_size = nb->fft_size;
        for (size_t c = 0; c < n_keep; ++c) {
            const size_t t = (size_t)(std::lower_bound(keep_t.begin(), keep_t.end(), b->trig_of[keep[c]]) - keep_t.begin());
            nb->trig_of[c] = (uint32_t)t;
            ntb->band_of[t] = nb->band_of[c];
            ntb->size_of[t] = nb->size_of[c];
        }
        if (derive_avg_keys(ntb.get()) || derive_trigger_keys(ntb.get())) return fail(FVAD_ERR_INVALID_ARGUMENT, "retain: trigger batch");
        if (const int rc = retain_device(ctx, tb, ntb.get(), keep_t.data(), keep_t.size())) return rc;
        if (const int rc = retain_device(ctx, b, nb.get(), keep, n_keep)) return rc;
        nb->trig = std::move(ntb);
    } else if (dp) {
        if (const int rc = retain_device(ctx, b, nb.get(), keep, n_keep)) return rc;
    }
    retain_commit(b, keep, n_keep, nb.get());
    return FVAD_OK;
}

} // extern "C"
