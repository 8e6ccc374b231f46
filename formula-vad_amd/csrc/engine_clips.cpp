// engine_clips.cpp -- the batch Recorder: fvad_clips_plan / _from_segments (host only) and every fvad_clips_export*, which run
// kernels_clips*.hip over device-resident lanes.  The reference finalises one AudioBuffer per completed segment, the quietest
// channel over [sample_from, sample_to) (Recorder.zig:74-164); here every clip of a call is picked and packed in three launches
// and only the packed clips leave the device.
//
// One engine for every form.  Written once: the tables a launch searches (build_tables, over a description per clip), the one
// allocation that holds them beside the form's own parts, its uploads, the ClipArgs, RMS and pick, the read-back and the scatter
// to the caller's arrays (run_clips, over either source), and the host-output wrapper (via_staging).  A form supplies its check,
// its rows, its parts and its launches:
// - fvad_clips_export*: a clip's channel is one run of a lane; rules in check_export, reported as "fvad_clips_export: ..."
// - fvad_clips_export_split*: a head piece in buffer A followed by a body piece in buffer B; rules in fvad_clips_split_check's
//   order (host_clips_split.cpp), reported as "<the entry point>: ..."
//   Both in four forms (ClipForm of clips_rules.h): full rate, strided (kernels_clips_strided.hip), filtered
//   (kernels_clips_fir.hip) and resampled (kernels_clips_resample.hip); the form's part is its taps as the gather walks them.
// - fvad_clips_export_mel* and fvad_clips_export_fbank*: log-mel or Kaldi-style filter-bank features of the picked channel's
//   strided stream (kernels_clips_mel.hip) in place of a gather, one form over a family and over either source (features_device,
//   features_host; fvad_clips_export_split_mel*, _split_fbank*: the split source's rows, tables and ClipSplitArgs); rules
//   in clips_features.h, shared with the host-only fvad_clips_mel_check and fvad_clips_fbank_check; parts: window, matrix and
//   the family's own two (the tiles' and clips' maxima, or the tiles' sums and the means).
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "clips_features.h"
#include "clips_split.h"
#include "internal.h"

using namespace fvad;

static_assert(kClipSrcTile == (uint64_t)kClipTile, "clips_rules.h and host_clips_split.cpp count the kernels' tiles");
static_assert(kStridedSrcTile == (uint64_t)kClipTile && FVAD_CLIP_STEP_MAX == kClipStepMax, "clips_strided.h counts the kernels' tiles");
static_assert(kFirSrcTile == (uint64_t)kClipTile && FVAD_CLIP_FIR_TAPS_MAX == kClipFirTapsMax, "clips_fir.h counts the kernels' tiles");
static_assert(kResampledWindow == (uint64_t)kClipTile, "clips_resample.h counts the kernels' window");
static_assert(FVAD_CLIP_MEL_NFFT_MAX == kClipMelNfftMax && FVAD_CLIP_MEL_BANDS_MAX == kClipMelBandsMax, "fvad.h states the kernels' limits");

namespace {

// ------------------------------------------------------------------ what every form shares

// one clip as the tables see it: its samples (src_off, or the pieces of a split clip), its slot and its gather tiles
struct ClipDesc {
    uint64_t len, n_channels, src_off, out_off, gather_tiles;
    uint32_t skip;
    ClipSplit split;
};

// one job per clip and the two prefix tables the workgroups search; splits only for a split source
struct ClipTables {
    std::vector<ClipJob> jobs;
    std::vector<ClipSplit> splits;
    std::vector<uint32_t> unit_prefix, tile_prefix;
    uint64_t units = 0, tiles = 0;
};

// false: more than 2^31 - 1 RMS units or gather tiles
template <typename Desc>
bool build_tables(size_t n_clips, bool split, Desc desc, ClipTables& t)
{
    t.jobs.resize(n_clips);
    t.splits.resize(split ? n_clips : 0);
    t.unit_prefix.resize(n_clips + 1);
    t.tile_prefix.resize(n_clips + 1);
    for (size_t i = 0; i < n_clips; ++i) {
        const ClipDesc c = desc(i);
        const uint64_t nt = (c.len + kClipTile - 1) / kClipTile;
        t.unit_prefix[i] = (uint32_t)t.units;
        t.tile_prefix[i] = (uint32_t)t.tiles;
        ClipJob& j = t.jobs[i];
        j.src_off = c.src_off;
        j.len = c.len;
        j.out_off = c.out_off;
        j.first_unit = (uint32_t)t.units;
        j.n_tiles = (uint32_t)nt;
        j.n_channels = (uint32_t)c.n_channels;
        j.skip = c.skip;
        if (split) t.splits[i] = c.split;
        t.units += nt * c.n_channels;
        t.tiles += c.gather_tiles;
        if (t.units > 0x7fffffffull || t.tiles > 0x7fffffffull) return false;
    }
    t.unit_prefix[n_clips] = (uint32_t)t.units;
    t.tile_prefix[n_clips] = (uint32_t)t.tiles;
    return true;
}

// what a call reports per clip; each may be NULL
struct ClipReport {
    int32_t* best_channel;
    float *best_rms, *runner_up_rms;
    uint64_t* out_offsets;
};

// a part of the call's one allocation: uploaded from `up` before the launches and read back into `down` after them (either
// may be NULL); dev is where run_clips put it
struct Part {
    const void* up;
    void* down;
    size_t bytes;
    char* dev;
};

// the source's share of the arguments; run_clips fills in the tables
ClipArgs source_args(const void* src, size_t lane_stride, int src_format, int out_format, void* d_out)
{
    ClipArgs c{};
    c.src = src;
    c.out = d_out;
    c.lane_stride = lane_stride;
    c.src_i16 = src_format == FVAD_CLIP_PCM16;
    c.out_i16 = out_format == FVAD_CLIP_PCM16;
    return c;
}

ClipArgs& base(ClipArgs& a) { return a; }
ClipArgs& base(ClipSplitArgs& a) { return a.c; }
const ClipArgs& base(const ClipArgs& a) { return a; }
const ClipArgs& base(const ClipSplitArgs& a) { return a.c; }
template <typename B> constexpr bool kSplit = std::is_same<B, ClipSplitArgs>::value;

// The device work of a call over source B: one allocation for the tables, the partials, the infos and the form's extra parts
// (every part 16-byte aligned), the uploads, RMS and pick, then gather(a, x) -- the form's launches, x its parts in place --,
// the read-back, the free on every path and the scatter to the caller's arrays.
template <typename B, typename Gather>
int run_clips(fvad_ctx* ctx, const std::string& who, B a, const ClipTables& t, const std::vector<Part>& extras, Gather gather, const ClipReport& rep)
{
    const size_t n_clips = t.jobs.size();
    std::vector<ClipInfo> infos(n_clips);
    enum { kJobs, kSplits, kUnitPrefix, kTilePrefix, kPartials, kInfos, kExtras };
    std::vector<Part> parts = {{t.jobs.data(), nullptr, n_clips * sizeof(ClipJob), nullptr},
                               {t.splits.data(), nullptr, t.splits.size() * sizeof(ClipSplit), nullptr},
                               {t.unit_prefix.data(), nullptr, (n_clips + 1) * 4, nullptr},
                               {t.tile_prefix.data(), nullptr, (n_clips + 1) * 4, nullptr},
                               {nullptr, nullptr, t.units * sizeof(double), nullptr},
                               {nullptr, infos.data(), n_clips * sizeof(ClipInfo), nullptr}};
    parts.insert(parts.end(), extras.begin(), extras.end());
    auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    size_t bytes = 0;
    for (const Part& p : parts) bytes += up16(p.bytes);
    char* d = nullptr;
    if (hipMalloc((void**)&d, bytes) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, who + ": hipMalloc of the clip tables failed"); }
    bytes = 0;
    for (Part& p : parts) { p.dev = d + bytes; bytes += up16(p.bytes); }
    auto run = [&]() -> int {
        for (const Part& p : parts)
            if (p.up && p.bytes) FVAD_HIP(ctx, hipMemcpyAsync(p.dev, p.up, p.bytes, hipMemcpyHostToDevice, ctx->stream));
        ClipArgs& c = base(a);
        c.jobs = reinterpret_cast<const ClipJob*>(parts[kJobs].dev);
        c.unit_prefix = reinterpret_cast<const uint32_t*>(parts[kUnitPrefix].dev);
        c.tile_prefix = reinterpret_cast<const uint32_t*>(parts[kTilePrefix].dev);
        c.partials = reinterpret_cast<double*>(parts[kPartials].dev);
        c.infos = reinterpret_cast<ClipInfo*>(parts[kInfos].dev);
        c.n_clips = (uint32_t)n_clips;
        c.n_units = (uint32_t)t.units;
        c.n_tiles = (uint32_t)t.tiles;
        if constexpr (kSplit<B>) a.splits = reinterpret_cast<const ClipSplit*>(parts[kSplits].dev);
        time_begin(ctx, kSplit<B> ? "clip_rms_split" : "clip_rms");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_rms(a, ctx->stream));
        time_end(ctx);
        time_begin(ctx, "clip_pick");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_pick(c, ctx->stream));
        time_end(ctx);
        const int rc = gather(a, parts.data() + kExtras);
        if (rc != FVAD_OK) return rc;
        for (const Part& p : parts)
            if (p.down && p.bytes) FVAD_HIP(ctx, hipMemcpyAsync(p.down, p.dev, p.bytes, hipMemcpyDeviceToHost, ctx->stream));
        FVAD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FVAD_OK;
    };
    const int rc = run();
    if (rc != FVAD_OK) (void)hipStreamSynchronize(ctx->stream);
    hipFree(d);
    if (rc != FVAD_OK) return rc;
    for (size_t i = 0; i < n_clips; ++i) {
        if (rep.best_channel) rep.best_channel[i] = infos[i].best_channel;
        if (rep.best_rms) rep.best_rms[i] = infos[i].best_rms;
        if (rep.runner_up_rms) rep.runner_up_rms[i] = infos[i].runner_up_rms;
        if (rep.out_offsets) rep.out_offsets[i] = infos[i].out_offset;
    }
    return FVAD_OK;
}

// The host-output form of a call whose rules held against the caller's own buffer: a device staging buffer of the plan's
// `bytes` (hipMalloc returns 256-byte aligned memory), device(d_out), one copy back, then freed.  who names the entry point,
// family the export's family in what a failed memset or copy says.
template <typename Device>
int via_staging(fvad_ctx* ctx, const std::string& who, const std::string& family, void* out, size_t bytes, Device device)
{
    hipSetDevice(ctx->device);
    void* d_out = nullptr;
    if (hipMalloc(&d_out, bytes) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, who + ": hipMalloc of the staging buffer failed"); }
    // the padding between slots is never written by the kernels: zero it, so that the host gets no stale device memory
    hipError_t e = hipMemsetAsync(d_out, 0, bytes, ctx->stream);
    int rc = e == hipSuccess ? device(d_out) : hip_fail(ctx, e, (family + ": hipMemsetAsync").c_str());
    if (rc == FVAD_OK) {
        e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = hip_fail(ctx, e, (family + ": copy back").c_str());
    }
    hipFree(d_out);
    return rc;
}

// ------------------------------------------------------------------ the four sample forms, over either source

// run_clips with the form's part -- the taps as the gather walks them: branch by branch (fir) or [j][o mod up] (resampled) --
// and its gather
template <typename B>
int run_form(fvad_ctx* ctx, const std::string& who, const B& src, const ClipTables& t, const ClipForm& f, const ClipReport& rep)
{
    // a step of 1 keeps every sample: the full-rate gather, whose tiles are the strided gather's
    const uint32_t step = f.strided ? f.strided->step : 1, tile_out = (uint32_t)form_tile_out(f);
    const std::vector<float> taps = f.rs ? resample_table(Taps{f.rs->taps, f.rs->n_taps}, Ratio{f.rs->up, f.rs->down}) : f.fir ? fir_branches(*f.fir, step) : std::vector<float>();
    auto gather = [&](const B& a, const Part* x) -> int {
        const float* d_taps = reinterpret_cast<const float*>(x[0].dev);
        if (f.rs) {
            time_begin(ctx, kSplit<B> ? "clip_gather_resampled_split" : "clip_gather_resampled");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_gather_resampled(ClipResampleArgs<B>{a, d_taps, f.rs->up, f.rs->down, tile_out, f.rs->n_taps}, ctx->stream));
        } else if (f.fir) {
            time_begin(ctx, kSplit<B> ? "clip_gather_fir_split" : "clip_gather_fir");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_gather_fir(ClipFirArgs<B>{a, d_taps, step, tile_out, f.fir->n_taps, 0}, ctx->stream));
        } else if (step == 1) {
            time_begin(ctx, kSplit<B> ? "clip_gather_split" : "clip_gather");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_gather(a, ctx->stream));
        } else {
            time_begin(ctx, kSplit<B> ? "clip_gather_strided_split" : "clip_gather_strided");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_clip_gather_strided(ClipStridedArgs<B>{a, step, tile_out}, ctx->stream));
        }
        time_end(ctx);
        return FVAD_OK;
    };
    return run_clips(ctx, who, src, t, {Part{taps.data(), nullptr, taps.size() * sizeof(float), nullptr}}, gather, rep);
}

// where a call's samples go: the caller's buffer (device or host memory), its capacity in samples of `format`, and the report
struct ClipOut {
    int format;
    void* p;
    size_t capacity;
    ClipReport rep;
};

// ------------------------------------------------------------------ fvad_clips_export*: a clip's channel is one run

struct Lanes {
    const void* d_src;
    int format;
    size_t n_lanes, lane_stride, n_samples;
    const uint64_t* clips;
    size_t n_clips;
};

struct ClipRow { uint64_t first_lane, n_channels, sample_from, sample_to; };
ClipRow row(const uint64_t* clips, size_t i)
{
    const uint64_t* r = clips + i * FVAD_CLIP_FIELDS;
    return {r[0], r[1], r[2], r[3]};
}
// a row's length, 0 for a row that breaks its own rules
uint64_t row_len(const uint64_t* clips, size_t i)
{
    const ClipRow c = row(clips, i);
    return c.sample_to <= c.sample_from || c.n_channels == 0 ? 0 : c.sample_to - c.sample_from;
}

// Every rule of fvad_clips_export*(_device), in one order for both outputs: arguments, then every clip's own rules and the
// form's (clip_slots of clips_rules.h), then its range and lanes, then the capacity.  Fills offsets and total.
int check_export(const fvad_ctx* ctx, const Lanes& s, const ClipOut& o, bool device_out, const ClipForm& form, std::vector<uint64_t>& offsets, uint64_t& total)
{
    if (!s.d_src || !s.clips || !o.p) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: NULL argument");
    if (!format_ok(s.format) || !format_ok(o.format)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: unknown sample format");
    if (device_out && (uintptr_t)o.p % 16 != 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: the output must be 16-byte aligned");
    if ((uintptr_t)s.d_src % format_bytes(s.format) != 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: the source is not aligned to its samples");
    if (s.n_lanes > 1 && s.lane_stride < s.n_samples) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: lane_stride < n_samples");
    offsets.resize(s.n_clips);
    const char *family = "", *why = "";
    if (!clip_slots(form, s.n_clips, [&](size_t i) { return row_len(s.clips, i); }, "", 16 / format_bytes(o.format), offsets.data(), &total, &family, &why))
        return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, *family ? std::string("fvad_clips_export_") + family + ": " + why
                                                               : std::string("fvad_clips_export: a clip with sample_to <= sample_from or no channels"));
    for (size_t i = 0; i < s.n_clips; ++i) {
        const ClipRow c = row(s.clips, i);
        if (c.sample_to > s.n_samples) return set_err(ctx, FVAD_ERR_OUT_OF_RANGE, "fvad_clips_export: a clip ends past n_samples");
        if (c.first_lane >= s.n_lanes || c.n_channels > s.n_lanes - c.first_lane)
            return set_err(ctx, FVAD_ERR_OUT_OF_RANGE, "fvad_clips_export: a clip's lanes end past n_lanes");
    }
    if (total > o.capacity) return set_err(ctx, FVAD_ERR_BUFFER_TOO_SMALL, "fvad_clips_export: out_capacity is below fvad_clips_plan's total");
    return FVAD_OK;
}

int export_device(fvad_ctx* ctx, const Lanes& s, const ClipOut& o, const ClipForm& form)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (s.n_clips == 0) return FVAD_OK;
    std::vector<uint64_t> offsets;
    uint64_t total = 0;
    const int bad = check_export(ctx, s, o, true, form, offsets, total);
    if (bad != FVAD_OK) return bad;
    ClipTables t;
    const auto desc = [&](size_t i) {
        const ClipRow c = row(s.clips, i);
        const uint64_t len = c.sample_to - c.sample_from;
        return ClipDesc{len, c.n_channels, c.first_lane * (uint64_t)s.lane_stride + c.sample_from, offsets[i], form_gather_tiles(form, i, len), form_skip(form, i), {}};
    };
    if (!build_tables(s.n_clips, false, desc, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_clips_export: more than 2^31 tiles in one call: export in batches");
    hipSetDevice(ctx->device);
    return run_form(ctx, "fvad_clips_export", source_args(s.d_src, s.lane_stride, s.format, o.format, o.p), t, form, o.rep);
}

int export_host(fvad_ctx* ctx, const Lanes& s, const ClipOut& o, const ClipForm& form)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (s.n_clips == 0) return FVAD_OK;
    std::vector<uint64_t> offsets;
    uint64_t total = 0;
    const int bad = check_export(ctx, s, o, false, form, offsets, total);
    if (bad != FVAD_OK) return bad;
    return via_staging(ctx, "fvad_clips_export", "fvad_clips_export", o.p, (size_t)total * format_bytes(o.format),
                       [&](void* d_out) { return export_device(ctx, s, ClipOut{o.format, d_out, (size_t)total, o.rep}, form); });
}

// ------------------------------------------------------------------ fvad_clips_export_split*: a head piece in A, a body piece in B

struct SplitLanes {
    const void* d_a;
    size_t a_lanes, a_stride, a_samples;
    const void* d_b;
    size_t b_lanes, b_stride, b_samples;
    int format;
    const uint64_t* clips;
    size_t n_clips;
};

// row c's pieces as the kernels address them (a piece of no samples is never addressed)
ClipSplit split_of(const SplitLanes& s, const SplitRow& c)
{
    return ClipSplit{c.a_len ? c.a_lane * (uint64_t)s.a_stride + c.a_from : 0, c.a_len, c.b_len ? c.b_lane * (uint64_t)s.b_stride + c.b_from : 0, 0};
}

// the source's share of a split call's arguments
ClipSplitArgs split_source_args(const SplitLanes& s, int out_format, void* d_out)
{
    return ClipSplitArgs{source_args(s.d_a, s.a_stride, s.format, out_format, d_out), s.d_b, s.b_stride, nullptr};
}

int check_split(const fvad_ctx* ctx, const char* who, const SplitLanes& s, const ClipOut& o, bool device_out, const ClipForm& form,
                std::vector<uint64_t>& offsets, uint64_t& total)
{
    offsets.resize(s.n_clips);
    const char* why = "";
    const int rc = clips_split_check(s.d_a, s.a_lanes, s.a_stride, s.a_samples, s.d_b, s.b_lanes, s.b_stride, s.b_samples, s.format, s.clips, s.n_clips,
                                     o.format, o.p, o.capacity, device_out, offsets.data(), &total, &why, form);
    return rc == FVAD_OK ? rc : set_err(ctx, rc, std::string(who) + ": " + why);
}

int export_split_device(fvad_ctx* ctx, const char* who, const SplitLanes& s, const ClipOut& o, const ClipForm& form)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (s.n_clips == 0) return FVAD_OK;
    std::vector<uint64_t> offsets;
    uint64_t total = 0;
    const int bad = check_split(ctx, who, s, o, true, form, offsets, total);
    if (bad != FVAD_OK) return bad;
    ClipTables t;
    const auto desc = [&](size_t i) {
        const SplitRow c = split_row(s.clips, i);
        const uint64_t len = c.a_len + c.b_len;
        return ClipDesc{len, c.n_channels, 0, offsets[i], form_gather_tiles(form, i, len), form_skip(form, i), split_of(s, c)};
    };
    if (!build_tables(s.n_clips, true, desc, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, std::string(who) + ": more than 2^31 tiles in one call: export in batches"); // (the check has bounded both)
    hipSetDevice(ctx->device);
    return run_form(ctx, who, split_source_args(s, o.format, o.p), t, form, o.rep);
}

int export_split_host(fvad_ctx* ctx, const char* who, const SplitLanes& s, const ClipOut& o, const ClipForm& form)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (s.n_clips == 0) return FVAD_OK;
    std::vector<uint64_t> offsets;
    uint64_t total = 0;
    const int bad = check_split(ctx, who, s, o, false, form, offsets, total);
    if (bad != FVAD_OK) return bad;
    return via_staging(ctx, who, "fvad_clips_export_split", o.p, (size_t)total * format_bytes(o.format),
                       [&](void* d_out) { return export_split_device(ctx, who, s, ClipOut{o.format, d_out, (size_t)total, o.rep}, form); });
}

// ------------------------------------------------------------------ fvad_clips_export_mel*, fvad_clips_export_fbank*: features in place of samples

// one call of either family (f.snip: the filter-bank one)
struct FeatCall {
    const char* who; // the family's entry point, as error strings name it
    Feat f;
    const float* window;
    const float* matrix;
    FeatCond c;
    uint64_t* n_frames; // what the call reports per clip beside ClipReport; each may be NULL
    float* per_clip;    // feat_max [n_clips] (log-mel) or means [n_clips][n_mels] (filter-bank)
};

// one timed launch of a family's list, over the tile kernels' arguments A of the call's source (ClipFeatOf of kernels.h)
template <typename A> struct FeatLaunch {
    const char* label;
    int (*fn)(const A&, hipStream_t);
    const char* what; // the call as FVAD_HIP would report it
    bool on;
};
#define FEAT_LAUNCH(label, fn, on) {label, fn, "(hipError_t)" #fn "(a, ctx->stream)", on}
// the launches that read tables and features only serve either source on its ClipFeatArgs
template <int (*Fn)(const ClipFeatArgs&, hipStream_t)> int feat_plain(const ClipFeatArgs& a, hipStream_t s) { return Fn(a, s); }
template <int (*Fn)(const ClipFeatArgs&, hipStream_t)> int feat_plain(const ClipFeatSplitArgs& a, hipStream_t s) { return Fn(a.f, s); }
#define FEAT_PLAIN(label, fn, on) {label, feat_plain<fn>, "(hipError_t)" #fn "(a, ctx->stream)", on}
ClipFeatArgs with_source(const ClipFeatArgs& a, const ClipArgs&) { return a; }
ClipFeatSplitArgs with_source(const ClipFeatArgs& a, const ClipSplitArgs& s) { return ClipFeatSplitArgs{a, s.b, s.b_stride, s.splits}; }

// the matrix as the kernels read it: [bin][band]
std::vector<float> bands_transposed(const float* matrix, uint32_t n_mels, uint32_t n_bins)
{
    std::vector<float> t((size_t)n_bins * n_mels);
    for (uint32_t b = 0; b < n_mels; ++b)
        for (uint32_t k = 0; k < n_bins; ++k) t[(size_t)k * n_mels + b] = matrix[(size_t)b * n_bins + k];
    return t;
}

// the tables of a feature call: one gather tile per tf frames of a clip
bool feature_tables(const Lanes& s, const uint32_t* skips, const std::vector<uint64_t>& offsets, const std::vector<uint64_t>& frames, uint32_t tf, ClipTables& t)
{
    const auto desc = [&](size_t i) {
        const ClipRow c = row(s.clips, i);
        return ClipDesc{c.sample_to - c.sample_from, c.n_channels, c.first_lane * (uint64_t)s.lane_stride + c.sample_from, offsets[i], (frames[i] + tf - 1) / tf, skips ? skips[i] : 0, {}};
    };
    return build_tables(s.n_clips, false, desc, t);
}

bool feature_tables(const SplitLanes& s, const uint32_t* skips, const std::vector<uint64_t>& offsets, const std::vector<uint64_t>& frames, uint32_t tf, ClipTables& t)
{
    const auto desc = [&](size_t i) {
        const SplitRow c = split_row(s.clips, i);
        return ClipDesc{c.a_len + c.b_len, c.n_channels, 0, offsets[i], (frames[i] + tf - 1) / tf, skips ? skips[i] : 0, split_of(s, c)};
    };
    return build_tables(s.n_clips, true, desc, t);
}

int check_features(const Lanes& s, const ClipOut& o, int device_out, const FeatCall& fc, uint64_t* n_frames, uint64_t* offsets, uint64_t* total, const char** why)
{
    return feat_check(s.d_src, s.format, s.n_lanes, s.lane_stride, s.n_samples, s.clips, s.n_clips, o.format, o.p, o.capacity, device_out, fc.f, fc.window,
                      fc.matrix, fc.c, n_frames, offsets, total, why);
}

int check_features(const SplitLanes& s, const ClipOut& o, int device_out, const FeatCall& fc, uint64_t* n_frames, uint64_t* offsets, uint64_t* total, const char** why)
{
    return feat_split_check(s.d_a, s.a_lanes, s.a_stride, s.a_samples, s.d_b, s.b_lanes, s.b_stride, s.b_samples, s.format, s.clips, s.n_clips, o.format, o.p,
                            o.capacity, device_out, fc.f, fc.window, fc.matrix, fc.c, n_frames, offsets, total, why);
}

ClipArgs feature_source(const Lanes& s, const ClipOut& o) { return source_args(s.d_src, s.lane_stride, s.format, o.format, o.p); }
ClipSplitArgs feature_source(const SplitLanes& s, const ClipOut& o) { return split_source_args(s, o.format, o.p); }

// A family supplies its parameters (fc.f, fc.c), its two own parts -- a float per tile and per clip (the tiles' and the clips'
// maxima) or n_mels of each (the tiles' sums and the clips' means) --, its launch list and, through the clip part, what it scatters.
// One form over either source (Src: Lanes or SplitLanes), which supplies its check, its tables and its share of the arguments.
template <typename Src>
int features_device(fvad_ctx* ctx, const Src& s, const ClipOut& o, const FeatCall& fc)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (s.n_clips == 0) return FVAD_OK;
    std::vector<uint64_t> offsets(s.n_clips), frames(s.n_clips);
    uint64_t total = 0;
    const char* why = "";
    const int bad = check_features(s, o, 1, fc, frames.data(), offsets.data(), &total, &why);
    if (bad != FVAD_OK) return set_err(ctx, bad, std::string(fc.who) + ": " + why);
    const Feat& f = fc.f;
    const uint32_t tf = feat_tile_frames(f.taps, f.hop), n_bins = f.n_fft / 2 + 1;
    ClipTables t;
    if (!feature_tables(s, f.skips, offsets, frames, tf, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, std::string(fc.who) + ": more than 2^31 tiles in one call: export in batches"); // (the check has bounded both)
    const std::vector<float> matrix_t = bands_transposed(fc.matrix, f.n_mels, n_bins);

    hipSetDevice(ctx->device);
    ClipFeatArgs a{};
    // the transform's tables (twiddles, un-mixing factors, radices), cached per context and size
    { const int rc = get_vad_plan(ctx, f.n_fft, &a.pl, true); if (rc != FVAD_OK) return rc; }
    const size_t cells = f.snip ? f.n_mels : 1;
    std::vector<float> per_clip(s.n_clips * cells);
    enum { kWindow, kMatrix, kPerTile, kPerClip };
    const std::vector<Part> parts = {{fc.window, nullptr, f.taps * sizeof(float), nullptr},
                                     {matrix_t.data(), nullptr, matrix_t.size() * sizeof(float), nullptr},
                                     {nullptr, nullptr, t.tiles * cells * sizeof(float), nullptr},
                                     {nullptr, per_clip.data(), per_clip.size() * sizeof(float), nullptr}};
    auto features = [&](const auto& src, const Part* x) -> int {
        using A = typename ClipFeatOf<std::decay_t<decltype(src)>>::type;
        a.c = base(src);
        a.window = reinterpret_cast<const float*>(x[kWindow].dev);
        a.matrix_t = reinterpret_cast<const float*>(x[kMatrix].dev);
        a.step = f.step;
        a.hop = f.hop;
        a.n_mels = f.n_mels;
        a.tile_frames = tf;
        a.floor = fc.c.floor;
        float* const per_tile_dev = reinterpret_cast<float*>(x[kPerTile].dev);
        float* const per_clip_dev = reinterpret_cast<float*>(x[kPerClip].dev);
        if (f.snip) {
            a.log_floor = (float)std::log((double)fc.c.floor);
            a.tile_sum = per_tile_dev;
            a.means = per_clip_dev;
            a.win = f.taps;
            a.scale = fc.c.scale;
            a.preemph = fc.c.preemph;
            a.remove_dc = fc.c.remove_dc;
        } else {
            a.log_floor = (float)std::log10((double)fc.c.floor);
            a.tile_max = per_tile_dev;
            a.feat_max = per_clip_dev;
            if (fc.c.norm) { a.norm_range = fc.c.norm[0]; a.norm_offset = fc.c.norm[1]; a.norm_scale = fc.c.norm[2]; }
            a.fft400 = f.n_fft == 400 && !ctx->tune.clip_mel_generic;
        }
        const A sa = with_source(a, src);
        const FeatLaunch<A> mel[] = {FEAT_LAUNCH(a.fft400 ? "clip_mel400" : "clip_mel", fvad_launch_clip_mel, true),
                                     FEAT_PLAIN("clip_mel_max", fvad_launch_clip_mel_max, true),
                                     FEAT_PLAIN("clip_mel_norm", fvad_launch_clip_mel_norm, fc.c.norm != nullptr)};
        const FeatLaunch<A> fbank[] = {FEAT_LAUNCH("clip_fbank", fvad_launch_clip_fbank, true),
                                       FEAT_PLAIN("clip_fbank_mean", fvad_launch_clip_fbank_mean, true),
                                       FEAT_PLAIN("clip_fbank_sub", fvad_launch_clip_fbank_sub, fc.c.cmn != 0)};
        for (const FeatLaunch<A>& l : f.snip ? fbank : mel) {
            if (!l.on) continue;
            time_begin(ctx, l.label);
            const hipError_t e = (hipError_t)l.fn(sa, ctx->stream);
            if (e != hipSuccess) return hip_fail(ctx, e, l.what);
            time_end(ctx);
        }
        return FVAD_OK;
    };
    const int rc = run_clips(ctx, fc.who, feature_source(s, o), t, parts, features, o.rep);
    if (rc != FVAD_OK) return rc;
    if (fc.n_frames) std::copy(frames.begin(), frames.end(), fc.n_frames);
    if (fc.per_clip) std::copy(per_clip.begin(), per_clip.end(), fc.per_clip);
    return FVAD_OK;
}

template <typename Src>
int features_host(fvad_ctx* ctx, const Src& s, const ClipOut& o, const FeatCall& fc)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (s.n_clips == 0) return FVAD_OK;
    // every rule against the caller's own buffer first
    uint64_t total = 0;
    const char* why = "";
    const int bad = check_features(s, o, 0, fc, nullptr, nullptr, &total, &why);
    if (bad != FVAD_OK) return set_err(ctx, bad, std::string(fc.who) + ": " + why);
    return via_staging(ctx, fc.who, fc.who, o.p, (size_t)total * sizeof(float),
                       [&](void* d_out) { return features_device(ctx, s, ClipOut{o.format, d_out, (size_t)total, o.rep}, fc); });
}

// the two families' calls
FeatCall mel_call(const char* who, uint32_t step, const uint32_t* skips, uint32_t n_fft, uint32_t hop, const float* window, uint32_t n_mels, const float* matrix,
                  float floor, const float* norm, uint64_t* n_frames, float* feat_max)
{
    return FeatCall{who, Feat{step, skips, n_fft, n_fft, hop, n_mels, false}, window, matrix, FeatCond{floor, norm, 0.0f, 0.0f, 0, 0}, n_frames, feat_max};
}

FeatCall fbank_call(const char* who, uint32_t step, const uint32_t* skips, uint32_t win_length, uint32_t n_fft, uint32_t hop, const float* window, uint32_t n_mels,
                    const float* matrix, float scale, float preemph, int remove_dc, float floor, int cmn, uint64_t* n_frames, float* means)
{
    return FeatCall{who, Feat{step, skips, win_length, n_fft, hop, n_mels, true}, window, matrix, FeatCond{floor, nullptr, scale, preemph, remove_dc, cmn}, n_frames, means};
}

// the argument rules of fvad_clips_plan: the full-rate slots
int plan_clips(const uint64_t* clips, size_t n, int out_format, uint64_t* offsets, uint64_t* total)
{
    const char *family, *why;
    uint64_t at = 0;
    if (!clip_slots(ClipForm{}, n, [&](size_t i) { return row_len(clips, i); }, "", 16 / format_bytes(out_format), offsets, &at, &family, &why)) return FVAD_ERR_INVALID_ARGUMENT;
    *total = at;
    return FVAD_OK;
}

} // namespace

// ------------------------------------------------------------------ the entry points

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
    return export_device(ctx, Lanes{d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips},
                         ClipOut{out_format, d_out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                         ClipForm{});
}

int fvad_clips_export(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                      const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity,
                      int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets)
{
    return export_host(ctx, Lanes{d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips},
                       ClipOut{out_format, out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                       ClipForm{});
}

int fvad_clips_export_strided_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride,
                                     size_t n_samples, const uint64_t* clips, size_t n_clips, int out_format, void* d_out,
                                     size_t out_capacity, int32_t* best_channel, float* best_rms, float* runner_up_rms,
                                     uint64_t* out_offsets, uint32_t step, const uint32_t* skips)
{
    const Strided s{step, skips};
    return export_device(ctx, Lanes{d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips},
                         ClipOut{out_format, d_out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                         ClipForm{&s, nullptr, nullptr});
}

int fvad_clips_export_strided(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                              const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity,
                              int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step,
                              const uint32_t* skips)
{
    const Strided s{step, skips};
    return export_host(ctx, Lanes{d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips},
                       ClipOut{out_format, out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                       ClipForm{&s, nullptr, nullptr});
}

int fvad_clips_export_fir_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                 const uint64_t* clips, size_t n_clips, int out_format, void* d_out, size_t out_capacity,
                                 int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step,
                                 const uint32_t* skips, const float* taps, uint32_t n_taps)
{
    const Strided s{step, skips};
    const Fir f{taps, n_taps};
    return export_device(ctx, Lanes{d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips},
                         ClipOut{out_format, d_out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                         ClipForm{&s, &f, nullptr});
}

int fvad_clips_export_fir(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                          const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity, int32_t* best_channel,
                          float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step, const uint32_t* skips,
                          const float* taps, uint32_t n_taps)
{
    const Strided s{step, skips};
    const Fir f{taps, n_taps};
    return export_host(ctx, Lanes{d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips},
                       ClipOut{out_format, out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                       ClipForm{&s, &f, nullptr});
}

int fvad_clips_export_resampled_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride,
                                       size_t n_samples, const uint64_t* clips, size_t n_clips, int out_format, void* d_out,
                                       size_t out_capacity, int32_t* best_channel, float* best_rms, float* runner_up_rms,
                                       uint64_t* out_offsets, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps)
{
    const Resampled r{up, down, taps, n_taps};
    return export_device(ctx, Lanes{d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips},
                         ClipOut{out_format, d_out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                         ClipForm{nullptr, nullptr, &r});
}

int fvad_clips_export_resampled(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity,
                                int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t up,
                                uint32_t down, const float* taps, uint32_t n_taps)
{
    const Resampled r{up, down, taps, n_taps};
    return export_host(ctx, Lanes{d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips},
                       ClipOut{out_format, out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                       ClipForm{nullptr, nullptr, &r});
}

int fvad_clips_export_split_device(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                   size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips,
                                   size_t n_clips, int out_format, void* d_out, size_t out_capacity, int32_t* best_channel,
                                   float* best_rms, float* runner_up_rms, uint64_t* out_offsets)
{
    return export_split_device(ctx, "fvad_clips_export_split", SplitLanes{d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips},
                               ClipOut{out_format, d_out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                               ClipForm{});
}

int fvad_clips_export_split(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                            size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips,
                            int out_format, void* out, size_t out_capacity, int32_t* best_channel, float* best_rms,
                            float* runner_up_rms, uint64_t* out_offsets)
{
    return export_split_host(ctx, "fvad_clips_export_split", SplitLanes{d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips},
                             ClipOut{out_format, out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                             ClipForm{});
}

int fvad_clips_export_split_strided_device(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                           const void* d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                           const uint64_t* clips, size_t n_clips, int out_format, void* d_out, size_t out_capacity,
                                           int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets,
                                           uint32_t step, const uint32_t* skips)
{
    const Strided s{step, skips};
    return export_split_device(ctx, "fvad_clips_export_split_strided", SplitLanes{d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips},
                               ClipOut{out_format, d_out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                               ClipForm{&s, nullptr, nullptr});
}

int fvad_clips_export_split_strided(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                    size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips,
                                    size_t n_clips, int out_format, void* out, size_t out_capacity, int32_t* best_channel,
                                    float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step, const uint32_t* skips)
{
    const Strided s{step, skips};
    return export_split_host(ctx, "fvad_clips_export_split_strided", SplitLanes{d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips},
                             ClipOut{out_format, out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                             ClipForm{&s, nullptr, nullptr});
}

int fvad_clips_export_split_fir_device(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                       size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips,
                                       size_t n_clips, int out_format, void* d_out, size_t out_capacity, int32_t* best_channel,
                                       float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step, const uint32_t* skips,
                                       const float* taps, uint32_t n_taps)
{
    const Strided s{step, skips};
    const Fir f{taps, n_taps};
    return export_split_device(ctx, "fvad_clips_export_split_fir", SplitLanes{d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips},
                               ClipOut{out_format, d_out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                               ClipForm{&s, &f, nullptr});
}

int fvad_clips_export_split_fir(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips,
                                int out_format, void* out, size_t out_capacity, int32_t* best_channel, float* best_rms,
                                float* runner_up_rms, uint64_t* out_offsets, uint32_t step, const uint32_t* skips, const float* taps,
                                uint32_t n_taps)
{
    const Strided s{step, skips};
    const Fir f{taps, n_taps};
    return export_split_host(ctx, "fvad_clips_export_split_fir", SplitLanes{d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips},
                             ClipOut{out_format, out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                             ClipForm{&s, &f, nullptr});
}

int fvad_clips_export_split_resampled_device(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                             const void* d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                             const uint64_t* clips, size_t n_clips, int out_format, void* d_out, size_t out_capacity,
                                             int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets,
                                             uint32_t up, uint32_t down, const float* taps, uint32_t n_taps)
{
    const Resampled r{up, down, taps, n_taps};
    return export_split_device(ctx, "fvad_clips_export_split_resampled", SplitLanes{d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips},
                               ClipOut{out_format, d_out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                               ClipForm{nullptr, nullptr, &r});
}

int fvad_clips_export_split_resampled(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                      size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips,
                                      size_t n_clips, int out_format, void* out, size_t out_capacity, int32_t* best_channel,
                                      float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t up, uint32_t down,
                                      const float* taps, uint32_t n_taps)
{
    const Resampled r{up, down, taps, n_taps};
    return export_split_host(ctx, "fvad_clips_export_split_resampled", SplitLanes{d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips},
                             ClipOut{out_format, out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                             ClipForm{nullptr, nullptr, &r});
}

int fvad_clips_export_mel_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                 const uint64_t* clips, size_t n_clips, int out_format, void* d_out, size_t out_capacity,
                                 int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step,
                                 const uint32_t* skips, uint32_t n_fft, uint32_t hop, const float* window, uint32_t n_mels,
                                 const float* matrix, float floor, const float* norm, uint64_t* n_frames, float* feat_max)
{
    return features_device(ctx, Lanes{d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips},
                      ClipOut{out_format, d_out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                      mel_call("fvad_clips_export_mel", step, skips, n_fft, hop, window, n_mels, matrix, floor, norm, n_frames, feat_max));
}

int fvad_clips_export_mel(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                          const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity, int32_t* best_channel,
                          float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step, const uint32_t* skips,
                          uint32_t n_fft, uint32_t hop, const float* window, uint32_t n_mels, const float* matrix, float floor,
                          const float* norm, uint64_t* n_frames, float* feat_max)
{
    return features_host(ctx, Lanes{d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips},
                    ClipOut{out_format, out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                    mel_call("fvad_clips_export_mel", step, skips, n_fft, hop, window, n_mels, matrix, floor, norm, n_frames, feat_max));
}

int fvad_clips_export_fbank_device(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                   const uint64_t* clips, size_t n_clips, int out_format, void* d_out, size_t out_capacity,
                                   int32_t* best_channel, float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step,
                                   const uint32_t* skips, uint32_t win_length, uint32_t n_fft, uint32_t hop, const float* window,
                                   uint32_t n_mels, const float* matrix, float scale, float preemph, int remove_dc, float floor, int cmn,
                                   uint64_t* n_frames, float* means)
{
    return features_device(ctx, Lanes{d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips},
                        ClipOut{out_format, d_out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                        fbank_call("fvad_clips_export_fbank", step, skips, win_length, n_fft, hop, window, n_mels, matrix, scale, preemph, remove_dc, floor, cmn, n_frames, means));
}

int fvad_clips_export_fbank(fvad_ctx* ctx, const void* d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                            const uint64_t* clips, size_t n_clips, int out_format, void* out, size_t out_capacity, int32_t* best_channel,
                            float* best_rms, float* runner_up_rms, uint64_t* out_offsets, uint32_t step, const uint32_t* skips,
                            uint32_t win_length, uint32_t n_fft, uint32_t hop, const float* window, uint32_t n_mels, const float* matrix,
                            float scale, float preemph, int remove_dc, float floor, int cmn, uint64_t* n_frames, float* means)
{
    return features_host(ctx, Lanes{d_src, src_format, n_lanes, lane_stride, n_samples, clips, n_clips},
                      ClipOut{out_format, out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                      fbank_call("fvad_clips_export_fbank", step, skips, win_length, n_fft, hop, window, n_mels, matrix, scale, preemph, remove_dc, floor, cmn, n_frames, means));
}

int fvad_clips_export_split_mel_device(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                       size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips,
                                       int out_format, void* d_out, size_t out_capacity, int32_t* best_channel, float* best_rms, float* runner_up_rms,
                                       uint64_t* out_offsets, uint32_t step, const uint32_t* skips, uint32_t n_fft, uint32_t hop, const float* window,
                                       uint32_t n_mels, const float* matrix, float floor, const float* norm, uint64_t* n_frames, float* feat_max)
{
    return features_device(ctx, SplitLanes{d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips},
                ClipOut{out_format, d_out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                mel_call("fvad_clips_export_split_mel", step, skips, n_fft, hop, window, n_mels, matrix, floor, norm, n_frames, feat_max));
}

int fvad_clips_export_split_mel(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips,
                                int out_format, void* out, size_t out_capacity, int32_t* best_channel, float* best_rms, float* runner_up_rms,
                                uint64_t* out_offsets, uint32_t step, const uint32_t* skips, uint32_t n_fft, uint32_t hop, const float* window,
                                uint32_t n_mels, const float* matrix, float floor, const float* norm, uint64_t* n_frames, float* feat_max)
{
    return features_host(ctx, SplitLanes{d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips},
                ClipOut{out_format, out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                mel_call("fvad_clips_export_split_mel", step, skips, n_fft, hop, window, n_mels, matrix, floor, norm, n_frames, feat_max));
}

int fvad_clips_export_split_fbank_device(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                         size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips,
                                         int out_format, void* d_out, size_t out_capacity, int32_t* best_channel, float* best_rms, float* runner_up_rms,
                                         uint64_t* out_offsets, uint32_t step, const uint32_t* skips, uint32_t win_length, uint32_t n_fft, uint32_t hop,
                                         const float* window, uint32_t n_mels, const float* matrix, float scale, float preemph, int remove_dc, float floor,
                                         int cmn, uint64_t* n_frames, float* means)
{
    return features_device(ctx, SplitLanes{d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips},
                ClipOut{out_format, d_out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                fbank_call("fvad_clips_export_split_fbank", step, skips, win_length, n_fft, hop, window, n_mels, matrix, scale, preemph, remove_dc, floor, cmn, n_frames, means));
}

int fvad_clips_export_split_fbank(fvad_ctx* ctx, const void* d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void* d_b,
                                  size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t* clips, size_t n_clips,
                                  int out_format, void* out, size_t out_capacity, int32_t* best_channel, float* best_rms, float* runner_up_rms,
                                  uint64_t* out_offsets, uint32_t step, const uint32_t* skips, uint32_t win_length, uint32_t n_fft, uint32_t hop,
                                  const float* window, uint32_t n_mels, const float* matrix, float scale, float preemph, int remove_dc, float floor,
                                  int cmn, uint64_t* n_frames, float* means)
{
    return features_host(ctx, SplitLanes{d_a, a_lanes, a_stride, a_samples, d_b, b_lanes, b_stride, b_samples, src_format, clips, n_clips},
                ClipOut{out_format, out, out_capacity, {best_channel, best_rms, runner_up_rms, out_offsets}},
                fbank_call("fvad_clips_export_split_fbank", step, skips, win_length, n_fft, hop, window, n_mels, matrix, scale, preemph, remove_dc, floor, cmn, n_frames, means));
}

} // extern "C"

