// engine_ingest.cpp -- fvad_ingest_device / fvad_ingest: a corpus's interleaved bytes into planar device lanes with
// kernels_ingest.hip; behind them fvad_ingest_resample_device / fvad_ingest_resample, the same two forms for files at another
// rate (kernels_ingest_resample.hip, the rules in resample.h).  The argument rules are fvad_ingest_check's (host_ingest.cpp); here are the tables a launch searches and,
// for bytes in host memory, the two-slot page-locked ring that carries them to the device.
#include <algorithm>
#include <cstring>
#include <vector>

#include "internal.h"
#include "resample.h"

using namespace fvad;

namespace {

struct Source { uint64_t byte_offset, n_frames, n_channels, format, first_lane, dst_offset, fill_to; };
Source row(const uint64_t* sources, size_t i)
{
    const uint64_t* r = sources + i * FVAD_INGEST_FIELDS;
    return {r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
}
uint64_t sample_bytes(uint64_t format) { return format == FVAD_INGEST_PCM16 ? 2 : format == FVAD_INGEST_PCM24 ? 3 : 4; }
size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// The tables of one call or batch: per source format (a launch decodes one) the jobs and their unit prefix, laid out in ONE
// blob whose parts start on 16-byte boundaries, so that one copy carries them to the device.
struct Tables {
    struct Set { size_t o_jobs = 0, o_prefix = 0; uint32_t n_jobs = 0, n_units = 0; } set[3];
    std::vector<char> blob;
};

// A launch is one workgroup of 256 lanes per unit; HIP runtimes refuse a grid of 2^32 threads or more, so a launch takes fewer
// than 2^24 units (about 270 GB of source bytes: the ring never gets near it, fvad_ingest_device only with a buffer of HBM's size).
constexpr uint64_t kMaxUnits = (1ull << 24) - 1;

// false: more than kMaxUnits units in one launch
bool build_tables(const std::vector<Source>& src, size_t lane_stride, Tables& t)
{
    t.blob.clear();
    for (int f = 0; f < 3; ++f) {
        std::vector<IngestJob> jobs;
        std::vector<uint32_t> prefix;
        uint64_t units = 0;
        for (const Source& s : src) {
            if ((int)s.format != f) continue;
            IngestJob j{};
            const uint64_t frame_bytes = s.n_channels * sample_bytes(s.format);
            j.tile_frames = (uint32_t)(kIngestTileBytes / frame_bytes / 4 * 4); // >= 64: a frame is at most 256 bytes
            j.src_off = s.byte_offset;
            j.n_frames = s.n_frames;
            j.dst_off = s.first_lane * (uint64_t)lane_stride + s.dst_offset;
            j.fill_len = s.fill_to - (s.dst_offset + s.n_frames);
            const uint64_t nd = (s.n_frames + j.tile_frames - 1) / j.tile_frames, nf = (j.fill_len + kIngestFillTile - 1) / kIngestFillTile;
            if (nd + nf * s.n_channels == 0) continue; // writes nothing
            if (nd > kMaxUnits || nf > kMaxUnits / kIngestMaxChannels) return false;
            j.n_data_tiles = (uint32_t)nd;
            j.n_fill_tiles = (uint32_t)nf;
            j.n_channels = (uint32_t)s.n_channels;
            prefix.push_back((uint32_t)units);
            jobs.push_back(j);
            units += nd + nf * s.n_channels;
            if (units > kMaxUnits) return false;
        }
        Tables::Set& set = t.set[f];
        set.n_jobs = (uint32_t)jobs.size();
        set.n_units = (uint32_t)units;
        if (jobs.empty()) continue;
        prefix.push_back((uint32_t)units);
        set.o_jobs = t.blob.size();
        set.o_prefix = set.o_jobs + up16(jobs.size() * sizeof(IngestJob));
        t.blob.resize(set.o_prefix + up16(prefix.size() * 4));
        memcpy(t.blob.data() + set.o_jobs, jobs.data(), jobs.size() * sizeof(IngestJob));
        memcpy(t.blob.data() + set.o_prefix, prefix.data(), prefix.size() * 4);
    }
    return true;
}

// the launches of one set of tables whose blob is at d_blob (queued on ctx->stream)
int launch_tables(fvad_ctx* ctx, const Tables& t, const char* d_blob, const void* d_raw, int out_format, void* d_lanes, size_t lane_stride)
{
    for (int f = 0; f < 3; ++f) {
        const Tables::Set& set = t.set[f];
        if (!set.n_units) continue;
        IngestArgs a{};
        a.raw = static_cast<const uint8_t*>(d_raw);
        a.lanes = d_lanes;
        a.lane_stride = lane_stride;
        a.jobs = reinterpret_cast<const IngestJob*>(d_blob + set.o_jobs);
        a.unit_prefix = reinterpret_cast<const uint32_t*>(d_blob + set.o_prefix);
        a.n_jobs = set.n_jobs;
        a.n_units = set.n_units;
        a.src_format = f;
        a.out_i16 = out_format == FVAD_INGEST_PCM16;
        time_begin(ctx, "ingest");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_ingest(a, ctx->stream));
        time_end(ctx);
    }
    return FVAD_OK;
}

int check_call(const fvad_ctx* ctx, const char* who, const uint64_t* sources, size_t n_sources, uint64_t raw_bytes, int out_format,
               const void* d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    const int rc = fvad_ingest_check(sources, n_sources, raw_bytes, out_format, n_lanes, lane_stride, n_samples);
    if (rc != FVAD_OK) return set_err(ctx, rc, std::string(who) + (rc == FVAD_ERR_OUT_OF_RANGE ? ": a source's lanes, fill_to or bytes are out of range"
                                                                                                 : ": a bad argument or source (fvad_ingest_check)"));
    if ((uintptr_t)d_lanes % (out_format == FVAD_INGEST_PCM16 ? 2 : 4) != 0)
        return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, std::string(who) + ": the lanes are not aligned to their samples");
    return FVAD_OK;
}

// the ring of fvad_ingest: two slots of `raw` bytes plus room for the tables of kBatchSources sources.  Its own, not
// fvad_engine_run's ring_in: that one is 32 slots of 8 MB filled by copy threads under a per-block event protocol, and a batch
// here must be ONE contiguous device image (the kernel indexes it by byte offset) with its tables behind it.
constexpr size_t kBatchSources = 4096;
constexpr size_t kTableBytes = 3 * 32 + kBatchSources * sizeof(IngestJob) + (kBatchSources + 3) * 4 + 3 * 16;
int ensure_ring(fvad_ctx* ctx, size_t raw)
{
    Workspace::IngestRing& r = ctx->ws.ingest;
    const size_t bytes = up16(raw) + up16(kTableBytes);
    if (r.bytes == bytes) return FVAD_OK;
    for (int k = 0; k < 2; ++k) {
        if (r.pin[k]) hipHostFree(r.pin[k]);
        if (r.dev[k]) hipFree(r.dev[k]);
        r.pin[k] = r.dev[k] = nullptr;
    }
    r.bytes = 0;
    for (int k = 0; k < 2; ++k) {
        if (!r.ev[k]) FVAD_HIP(ctx, hipEventCreateWithFlags(&r.ev[k], hipEventDisableTiming));
        FVAD_HIP(ctx, hipHostMalloc((void**)&r.pin[k], bytes, hipHostMallocDefault));
        FVAD_HIP(ctx, hipMalloc((void**)&r.dev[k], bytes));
    }
    r.bytes = bytes;
    return FVAD_OK;
}

} // namespace

int fvad::ingest_ring_ensure(fvad_ctx* ctx, size_t raw, size_t* table_bytes)
{
    *table_bytes = kTableBytes;
    return ensure_ring(ctx, raw);
}

extern "C" {

int fvad_ingest_device(fvad_ctx* ctx, const void* d_raw, uint64_t raw_bytes, const uint64_t* sources, size_t n_sources,
                       int out_format, void* d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sources && (!d_raw || !d_lanes)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest_device: NULL argument");
    const int bad = check_call(ctx, "fvad_ingest_device", sources, n_sources, raw_bytes, out_format, d_lanes, n_lanes, lane_stride, n_samples);
    if (bad != FVAD_OK) return bad;
    if (n_sources == 0) return FVAD_OK;
    std::vector<Source> src(n_sources);
    for (size_t i = 0; i < n_sources; ++i) src[i] = row(sources, i);
    Tables t;
    if (!build_tables(src, lane_stride, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest_device: more than 2^24 tiles in one call: ingest in batches");
    if (t.blob.empty()) return FVAD_OK; // nothing to write
    hipSetDevice(ctx->device);
    char* d = nullptr;
    if (hipMalloc((void**)&d, t.blob.size()) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "fvad_ingest_device: hipMalloc of the source tables failed"); }
    auto run = [&]() -> int {
        FVAD_HIP(ctx, hipMemcpyAsync(d, t.blob.data(), t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
        const int rc = launch_tables(ctx, t, d, d_raw, out_format, d_lanes, lane_stride);
        if (rc != FVAD_OK) return rc;
        FVAD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FVAD_OK;
    };
    const int rc = run();
    if (rc != FVAD_OK) (void)hipStreamSynchronize(ctx->stream);
    hipFree(d);
    return rc;
}

// Batches of at most ring_bytes raw bytes: the sources' bytes are copied one after the other (each piece on a 16-byte boundary)
// into a page-locked slot, the batch's tables behind them, one DMA takes both to the slot's device image and the kernels run on
// it -- while this thread fills the other slot with the next batch.  A source that does not fit what is left of a batch is cut
// at a multiple of 4 frames; a piece is a source of its own (its frames, then -- the last piece only -- the fill), so the lanes
// get the same bits however the sources are cut.
// The size (Tuning::ingest_ring_bytes, 32 MB): a batch's fixed costs -- a DMA, up to three launches, an event -- are tens of
// microseconds, against about a millisecond of PCIe time for 32 MB, and only the first batch's host copy is not overlapped;
// two slots of 32 MB of page-locked memory per context is a quarter of what fvad_engine_run's rings hold.  Computed from
// shapes, not tuned.
int fvad_ingest(fvad_ctx* ctx, const void* const* src_host, const uint64_t* sources, size_t n_sources, int out_format,
                void* d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sources && (!src_host || !d_lanes)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest: NULL argument");
    const int bad = check_call(ctx, "fvad_ingest", sources, n_sources, UINT64_MAX, out_format, d_lanes, n_lanes, lane_stride, n_samples);
    if (bad != FVAD_OK) return bad;
    for (size_t i = 0; i < n_sources; ++i)
        if (!src_host[i] && row(sources, i).n_frames) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest: a source with frames and no bytes");
    if (n_sources == 0) return FVAD_OK;
    hipSetDevice(ctx->device);
    const size_t cap = (size_t)ctx->tune.ingest_ring_bytes;
    const int rc0 = ensure_ring(ctx, cap);
    if (rc0 != FVAD_OK) return rc0;
    Workspace::IngestRing& ring = ctx->ws.ingest;
    const size_t o_tables = up16(cap);

    std::vector<Source> batch;                               // the pieces of the batch being filled, byte_offset within the slot
    struct Copy { size_t at; const char* from; size_t bytes; };
    std::vector<Copy> copies;
    size_t used = 0;
    int slot = 0;
    Tables t;
    auto flush = [&]() -> int {
        if (batch.empty()) return FVAD_OK;
        if (!build_tables(batch, lane_stride, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest: more than 2^24 tiles in one batch");
        if (!t.blob.empty()) {
            FVAD_HIP(ctx, hipEventSynchronize(ring.ev[slot])); // the slot's previous batch has been read (a fresh event is complete)
            for (const Copy& c : copies) memcpy(ring.pin[slot] + c.at, c.from, c.bytes);
            memcpy(ring.pin[slot] + o_tables, t.blob.data(), t.blob.size());
            // the raw bytes and the tables: one copy when the gap between them is small, else two
            if (o_tables - used <= (1u << 20)) {
                FVAD_HIP(ctx, hipMemcpyAsync(ring.dev[slot], ring.pin[slot], o_tables + t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
            } else {
                if (used) FVAD_HIP(ctx, hipMemcpyAsync(ring.dev[slot], ring.pin[slot], used, hipMemcpyHostToDevice, ctx->stream));
                FVAD_HIP(ctx, hipMemcpyAsync(ring.dev[slot] + o_tables, ring.pin[slot] + o_tables, t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
            }
            const int rc = launch_tables(ctx, t, ring.dev[slot] + o_tables, ring.dev[slot], out_format, d_lanes, lane_stride);
            if (rc != FVAD_OK) return rc;
            FVAD_HIP(ctx, hipEventRecord(ring.ev[slot], ctx->stream));
            slot ^= 1;
        }
        batch.clear();
        copies.clear();
        used = 0;
        return FVAD_OK;
    };
    auto run = [&]() -> int {
        for (size_t i = 0; i < n_sources; ++i) {
            const Source s = row(sources, i);
            const uint64_t frame_bytes = s.n_channels * sample_bytes(s.format);
            uint64_t done = 0;
            do {
                size_t at = up16(used);
                uint64_t fit = at < cap ? (cap - at) / frame_bytes / 4 * 4 : 0; // frames that fit, cut at multiples of 4
                if ((fit == 0 && s.n_frames - done > 0 && !batch.empty()) || batch.size() == kBatchSources) {
                    const int rc = flush();
                    if (rc != FVAD_OK) return rc;
                    at = 0;
                    fit = cap / frame_bytes / 4 * 4; // >= 4: the ring holds at least 1 KB, a frame is at most 256 bytes
                }
                const uint64_t n = std::min<uint64_t>(s.n_frames - done, fit);
                Source piece = s;
                piece.byte_offset = at;
                piece.n_frames = n;
                piece.dst_offset = s.dst_offset + done;
                piece.fill_to = done + n == s.n_frames ? s.fill_to : piece.dst_offset + n;
                batch.push_back(piece);
                if (n) {
                    copies.push_back({at, static_cast<const char*>(src_host[i]) + s.byte_offset + done * frame_bytes, (size_t)(n * frame_bytes)});
                    used = at + (size_t)(n * frame_bytes);
                }
                done += n;
            } while (done < s.n_frames);
        }
        const int rc = flush();
        if (rc != FVAD_OK) return rc;
        FVAD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FVAD_OK;
    };
    const int rc = run();
    if (rc != FVAD_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

} // extern "C"

// ------------------------------------------------------------------ the resampling ingest
namespace {

struct RSource { uint64_t byte_offset, n_frames, n_channels, format, first_lane, dst_offset, fill_to, frame_base, file_frames, out_from, n_out; };
RSource rrow(const uint64_t* sources, size_t i)
{
    const uint64_t* r = sources + i * FVAD_RESAMPLE_FIELDS;
    return {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10]};
}

// build_tables' blob for resample jobs; lds: the largest window a tile of the set stages, + 16
struct RTables {
    struct Set { size_t o_jobs = 0, o_prefix = 0; uint32_t n_jobs = 0, n_units = 0, lds = 0; } set[3];
    std::vector<char> blob;
};

// the ring's table room (kTableBytes, sized for fvad_ingest's jobs) holds this many of the larger resample jobs
constexpr size_t kRBatchSources = 2048;
static_assert(3 * 32 + kRBatchSources * sizeof(IngestResampleJob) + (kRBatchSources + 3) * 4 + 3 * 16 <= kTableBytes, "the ring's table room");

bool build_rtables(const std::vector<RSource>& src, size_t lane_stride, const Ratio& q, uint32_t n_taps, RTables& t)
{
    t.blob.clear();
    for (int f = 0; f < 3; ++f) {
        std::vector<IngestResampleJob> jobs;
        std::vector<uint32_t> prefix;
        uint64_t units = 0, lds = 0;
        for (const RSource& s : src) {
            if ((int)s.format != f) continue;
            IngestResampleJob j{};
            const uint64_t frame_bytes = s.n_channels * sample_bytes(s.format);
            j.tile_out = (uint32_t)resample_tile(q, n_taps, s.n_channels, s.format); // >= 4: the check refused 0
            j.src_off = s.byte_offset;
            j.frame_base = s.frame_base;
            j.file_frames = s.file_frames;
            j.out_from = s.out_from;
            j.n_out = s.n_out;
            j.dst_off = s.first_lane * (uint64_t)lane_stride + s.dst_offset;
            j.fill_len = s.fill_to - (s.dst_offset + s.n_out);
            const uint64_t nd = (s.n_out + j.tile_out - 1) / j.tile_out, nf = (j.fill_len + kIngestFillTile - 1) / kIngestFillTile;
            if (nd + nf * s.n_channels == 0) continue; // writes nothing
            if (nd > kMaxUnits || nf > kMaxUnits / kIngestMaxChannels) return false;
            j.n_data_tiles = (uint32_t)nd;
            j.n_fill_tiles = (uint32_t)nf;
            j.n_channels = (uint32_t)s.n_channels;
            if (nd) lds = std::max<uint64_t>(lds, (uint64_t)resample_reach(q, n_taps, j.tile_out) * frame_bytes);
            prefix.push_back((uint32_t)units);
            jobs.push_back(j);
            units += nd + nf * s.n_channels;
            if (units > kMaxUnits) return false;
        }
        RTables::Set& set = t.set[f];
        set.n_jobs = (uint32_t)jobs.size();
        set.n_units = (uint32_t)units;
        set.lds = (uint32_t)up16(lds + 16);
        if (jobs.empty()) continue;
        prefix.push_back((uint32_t)units);
        set.o_jobs = t.blob.size();
        set.o_prefix = set.o_jobs + up16(jobs.size() * sizeof(IngestResampleJob));
        t.blob.resize(set.o_prefix + up16(prefix.size() * 4));
        memcpy(t.blob.data() + set.o_jobs, jobs.data(), jobs.size() * sizeof(IngestResampleJob));
        memcpy(t.blob.data() + set.o_prefix, prefix.data(), prefix.size() * 4);
    }
    return true;
}

int launch_rtables(fvad_ctx* ctx, const RTables& t, const char* d_blob, const void* d_raw, const float* d_table, const Ratio& q,
                   uint32_t n_taps, void* d_lanes, size_t lane_stride)
{
    for (int f = 0; f < 3; ++f) {
        const RTables::Set& set = t.set[f];
        if (!set.n_units) continue;
        IngestResampleArgs a{};
        a.raw = static_cast<const uint8_t*>(d_raw);
        a.lanes = static_cast<float*>(d_lanes);
        a.lane_stride = lane_stride;
        a.jobs = reinterpret_cast<const IngestResampleJob*>(d_blob + set.o_jobs);
        a.unit_prefix = reinterpret_cast<const uint32_t*>(d_blob + set.o_prefix);
        a.table = d_table;
        a.n_jobs = set.n_jobs;
        a.n_units = set.n_units;
        a.up = q.up;
        a.down = q.down;
        a.n_taps = n_taps;
        a.src_format = f;
        a.lds_bytes = set.lds;
        time_begin(ctx, "ingest_resample");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_ingest_resample(a, ctx->stream));
        time_end(ctx);
    }
    return FVAD_OK;
}

int check_rcall(const fvad_ctx* ctx, const char* who, const uint64_t* sources, size_t n_sources, uint64_t raw_bytes, uint32_t up, uint32_t down,
                const float* taps, uint32_t n_taps, const void* d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    const int rc = fvad_ingest_resample_check(sources, n_sources, raw_bytes, up, down, taps, n_taps, FVAD_INGEST_F32, n_lanes, lane_stride, n_samples);
    if (rc != FVAD_OK) return set_err(ctx, rc, std::string(who) + (rc == FVAD_ERR_OUT_OF_RANGE ? ": a source's lanes, fill_to or bytes are out of range"
                                                                                                 : ": a bad argument, ratio, tap or source (fvad_ingest_resample_check)"));
    if ((uintptr_t)d_lanes % 4 != 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, std::string(who) + ": the lanes are not aligned to their samples");
    return FVAD_OK;
}

} // namespace

extern "C" {

int fvad_ingest_resample_device(fvad_ctx* ctx, const void* d_raw, uint64_t raw_bytes, const uint64_t* sources, size_t n_sources, uint32_t up,
                                uint32_t down, const float* taps, uint32_t n_taps, void* d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sources && (!d_raw || !d_lanes)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest_resample_device: NULL argument");
    const int bad = check_rcall(ctx, "fvad_ingest_resample_device", sources, n_sources, raw_bytes, up, down, taps, n_taps, d_lanes, n_lanes, lane_stride, n_samples);
    if (bad != FVAD_OK) return bad;
    if (n_sources == 0) return FVAD_OK;
    const Ratio q{up, down};
    std::vector<RSource> src(n_sources);
    for (size_t i = 0; i < n_sources; ++i) src[i] = rrow(sources, i);
    RTables t;
    if (!build_rtables(src, lane_stride, q, n_taps, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest_resample_device: more than 2^24 tiles in one call: ingest in batches");
    if (t.blob.empty()) return FVAD_OK; // nothing to write
    const std::vector<float> table = resample_table(Taps{taps, n_taps}, q);
    const size_t o_blob = up16(table.size() * 4);
    hipSetDevice(ctx->device);
    char* d = nullptr; // the tap table, then the source tables
    if (hipMalloc((void**)&d, o_blob + t.blob.size()) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "fvad_ingest_resample_device: hipMalloc of the tables failed"); }
    auto run = [&]() -> int {
        FVAD_HIP(ctx, hipMemcpyAsync(d, table.data(), table.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_blob, t.blob.data(), t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
        const int rc = launch_rtables(ctx, t, d + o_blob, d_raw, reinterpret_cast<const float*>(d), q, n_taps, d_lanes, lane_stride);
        if (rc != FVAD_OK) return rc;
        FVAD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FVAD_OK;
    };
    const int rc = run();
    if (rc != FVAD_OK) (void)hipStreamSynchronize(ctx->stream);
    hipFree(d);
    return rc;
}

// fvad_ingest's ring, cut in OUTPUT coordinates: a batch takes as many outputs of a source (in fours) as have their window in
// what is left of the slot, and the window's frames are what is copied -- so neighbouring pieces of a source overlap by the
// filter's reach, each piece's given frames cover its window, and by the check's rule the pieces' outputs are the file's.  A
// ring smaller than the window of 4 outputs of the call's widest source is enlarged to it for this call.
int fvad_ingest_resample(fvad_ctx* ctx, const void* const* src_host, const uint64_t* sources, size_t n_sources, uint32_t up, uint32_t down,
                         const float* taps, uint32_t n_taps, void* d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sources && (!src_host || !d_lanes)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest_resample: NULL argument");
    const int bad = check_rcall(ctx, "fvad_ingest_resample", sources, n_sources, UINT64_MAX, up, down, taps, n_taps, d_lanes, n_lanes, lane_stride, n_samples);
    if (bad != FVAD_OK) return bad;
    const Ratio q{up, down};
    size_t cap = (size_t)ctx->tune.ingest_ring_bytes;
    for (size_t i = 0; i < n_sources; ++i) {
        const RSource s = rrow(sources, i);
        if (!src_host[i] && s.n_frames) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest_resample: a source with frames and no bytes");
        cap = std::max(cap, up16((size_t)resample_reach(q, n_taps, 4) * (size_t)(s.n_channels * sample_bytes(s.format)))); // (at most 64 KB: the tile rule)
    }
    if (n_sources == 0) return FVAD_OK;
    hipSetDevice(ctx->device);
    const int rc0 = ensure_ring(ctx, cap);
    if (rc0 != FVAD_OK) return rc0;
    Workspace::IngestRing& ring = ctx->ws.ingest;
    const size_t o_tables = up16(cap);
    const std::vector<float> table = resample_table(Taps{taps, n_taps}, q);
    float* d_table = nullptr;
    if (hipMalloc((void**)&d_table, table.size() * 4) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "fvad_ingest_resample: hipMalloc of the tap table failed"); }

    std::vector<RSource> batch; // the pieces of the batch being filled, byte_offset within the slot
    struct Copy { size_t at; const char* from; size_t bytes; };
    std::vector<Copy> copies;
    size_t used = 0;
    int slot = 0;
    RTables t;
    auto flush = [&]() -> int {
        if (batch.empty()) return FVAD_OK;
        if (!build_rtables(batch, lane_stride, q, n_taps, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest_resample: more than 2^24 tiles in one batch");
        if (!t.blob.empty()) {
            FVAD_HIP(ctx, hipEventSynchronize(ring.ev[slot])); // the slot's previous batch has been read (a fresh event is complete)
            for (const Copy& c : copies) memcpy(ring.pin[slot] + c.at, c.from, c.bytes);
            memcpy(ring.pin[slot] + o_tables, t.blob.data(), t.blob.size());
            if (o_tables - used <= (1u << 20)) {
                FVAD_HIP(ctx, hipMemcpyAsync(ring.dev[slot], ring.pin[slot], o_tables + t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
            } else {
                if (used) FVAD_HIP(ctx, hipMemcpyAsync(ring.dev[slot], ring.pin[slot], used, hipMemcpyHostToDevice, ctx->stream));
                FVAD_HIP(ctx, hipMemcpyAsync(ring.dev[slot] + o_tables, ring.pin[slot] + o_tables, t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
            }
            const int rc = launch_rtables(ctx, t, ring.dev[slot] + o_tables, ring.dev[slot], d_table, q, n_taps, d_lanes, lane_stride);
            if (rc != FVAD_OK) return rc;
            FVAD_HIP(ctx, hipEventRecord(ring.ev[slot], ctx->stream));
            slot ^= 1;
        }
        batch.clear();
        copies.clear();
        used = 0;
        return FVAD_OK;
    };
    auto run = [&]() -> int {
        FVAD_HIP(ctx, hipMemcpyAsync(d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        for (size_t i = 0; i < n_sources; ++i) {
            const RSource s = rrow(sources, i);
            const uint64_t frame_bytes = s.n_channels * sample_bytes(s.format);
            uint64_t done = 0; // outputs
            do {
                size_t at = up16(used);
                uint64_t fit = at < cap ? resample_fit(q, n_taps, frame_bytes, cap - at, UINT64_MAX / 2) : 0; // outputs whose window fits, in fours
                if ((fit == 0 && s.n_out - done > 0 && !batch.empty()) || batch.size() == kRBatchSources) {
                    const int rc = flush();
                    if (rc != FVAD_OK) return rc;
                    at = 0;
                    fit = resample_fit(q, n_taps, frame_bytes, cap, UINT64_MAX / 2); // >= 4: cap holds the window of 4 outputs
                }
                const uint64_t n = std::min<uint64_t>(s.n_out - done, fit);
                RSource piece = s;
                piece.out_from = s.out_from + done;
                piece.n_out = n;
                uint64_t lo, hi;
                resample_window(q, n_taps, s.file_frames, piece.out_from, n, &lo, &hi);
                piece.byte_offset = at;
                piece.frame_base = lo;
                piece.n_frames = hi - lo;
                piece.dst_offset = s.dst_offset + done;
                piece.fill_to = done + n == s.n_out ? s.fill_to : piece.dst_offset + n;
                batch.push_back(piece);
                if (hi > lo) { // (the check: the source's given frames cover [lo, hi))
                    copies.push_back({at, static_cast<const char*>(src_host[i]) + s.byte_offset + (lo - s.frame_base) * frame_bytes, (size_t)((hi - lo) * frame_bytes)});
                    used = at + (size_t)((hi - lo) * frame_bytes);
                }
                done += n;
            } while (done < s.n_out);
        }
        const int rc = flush();
        if (rc != FVAD_OK) return rc;
        FVAD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FVAD_OK;
    };
    const int rc = run();
    if (rc != FVAD_OK) (void)hipStreamSynchronize(ctx->stream);
    hipFree(d_table);
    return rc;
}

} // extern "C"
