// engine_ingest.cpp -- the ingest calls, each in a device form (bytes in device memory) and a host form (bytes in host memory):
// the interleaved bytes of files' data chunks into planar device lanes.
//   fvad_ingest*           frames as they are (kernels_ingest.hip; the rules are fvad_ingest_check's, host_ingest.cpp)
//   fvad_ingest_resample*  files at another rate resampled to the lanes' (kernels_ingest_resample.hip; host_resample.cpp; the
//                          window, the tile and the tap table are resample.h's)
// What the forms share is written once: the tables a launch searches and the device form's upload-launch-wait (io_tables.h,
// shared with engine_egress.cpp) and, for bytes in host memory, the batches through the two-slot page-locked ring (host_form
// below, with the ring itself).  A form supplies its row, how a row is cut, the job of a row and the launch of one source
// format's jobs.
#include <algorithm>
#include <cstring>
#include <vector>

#include "internal.h"
#include "io_tables.h"
#include "resample.h"

using namespace fvad;

namespace {

// The rows of the two table layouts, field for field (fvad.h), so that a row is decoded by a copy (row<Row>).  Each begins
// with ingest_rules.h's seven fields; a resampled row counts outputs (n_out) where a plain one counts frames.
struct Source { uint64_t byte_offset, n_frames, n_channels, format, first_lane, dst_offset, fill_to; };
struct RSource { uint64_t byte_offset, n_frames, n_channels, format, first_lane, dst_offset, fill_to, frame_base, file_frames, out_from, n_out; };
static_assert(sizeof(Source) == FVAD_INGEST_FIELDS * 8 && sizeof(RSource) == FVAD_RESAMPLE_FIELDS * 8, "fvad.h's rows");

// What the jobs of both forms share: where a row writes, the zeros behind its `count` samples, and its units -- data tiles of
// `tile` samples of every channel, then fill tiles lane by lane.  A row with no frames may still fill, so it is the UNITS that
// say whether a row writes anything.  More than a launch takes in either kind of tile: UINT64_MAX, which build_tables refuses.
template <typename Row, typename Job>
uint64_t place(const Row& s, size_t lane_stride, uint64_t count, uint32_t tile, Job& j)
{
    j.dst_off = s.first_lane * (uint64_t)lane_stride + s.dst_offset;
    j.fill_len = s.fill_to - (s.dst_offset + count);
    const uint64_t nd = (count + tile - 1) / tile, nf = (j.fill_len + kIngestFillTile - 1) / kIngestFillTile;
    if (nd > kMaxUnits || nf > kMaxUnits / kIngestMaxChannels) return UINT64_MAX;
    j.n_data_tiles = (uint32_t)nd;
    j.n_fill_tiles = (uint32_t)nf;
    j.n_channels = (uint32_t)s.n_channels;
    return nd + nf * s.n_channels;
}

// The refusal of a form's check in the call's words (`range` and `invalid` end the message), then what no check sees: the
// lanes aligned to their samples.
int check_call(const fvad_ctx* ctx, const std::string& who, int rc, const char* range, const char* invalid, const void* d_lanes, size_t sample_bytes)
{
    if (rc != FVAD_OK) return set_err(ctx, rc, who + (rc == FVAD_ERR_OUT_OF_RANGE ? range : invalid));
    if ((uintptr_t)d_lanes % sample_bytes != 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": the lanes are not aligned to their samples");
    return FVAD_OK;
}
const char* const kOutOfRange = ": a source's lanes, fill_to or bytes are out of range";

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

// The host form behind its check.  Batches of at most ring_bytes raw bytes: the sources' bytes are copied one after the other
// (each piece on a 16-byte boundary) into a page-locked slot, the batch's tables behind them, one DMA takes both to the slot's
// device image and the kernels run on it -- while this thread fills the other slot with the next batch.  A source that does
// not fit what is left of a batch is cut at a multiple of 4 samples of its count; a piece is a source of its own (what it
// writes, then -- the last piece only -- the fill), so the lanes get the same bits however the sources are cut.
// The size (Tuning::ingest_ring_bytes, 32 MB): a batch's fixed costs -- a DMA, up to three launches, an event -- are tens of
// microseconds, against about a millisecond of PCIe time for 32 MB, and only the first batch's host copy is not overlapped;
// two slots of 32 MB of page-locked memory per context is a quarter of what fvad_engine_run's rings hold.  Computed from
// shapes, not tuned.
// A form F has: Row and Job; count, the Row's field that counts what it writes; kBatch, the pieces a batch holds at most (its
// tables fit the ring's table room); slot_min(frame_bytes), the slot a source of such frames needs at least (a smaller ring is
// enlarged to it for this call); fit(frame_bytes, bytes), the most samples of the count, in fours, whose bytes fit; cut(piece,
// s, done, n), which makes `piece` (a copy of s) the n samples from s's sample `done` on but for its place in the slot and in
// the lanes, and returns where in s's buffer its bytes lie; table, the tap table (uploaded once per call) or none; make and
// launch(t, d_blob, d_table, d_raw), the job of a row and a batch's kernels.
struct Bytes { uint64_t from; size_t n; };
template <typename F>
int host_form(fvad_ctx* ctx, const std::string& who, const void* const* src_host, const uint64_t* sources, size_t n_sources, F& form)
{
    using Row = typename F::Row;
    size_t cap = (size_t)ctx->tune.ingest_ring_bytes;
    for (size_t i = 0; i < n_sources; ++i) {
        const Row s = row<Row>(sources, i);
        if (!src_host[i] && s.n_frames) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": a source with frames and no bytes");
        cap = std::max(cap, form.slot_min(s.n_channels * sample_bytes_of(s.format)));
    }
    if (n_sources == 0) return FVAD_OK;
    hipSetDevice(ctx->device);
    const int rc0 = ensure_ring(ctx, cap);
    if (rc0 != FVAD_OK) return rc0;
    Workspace::IngestRing& ring = ctx->ws.ingest;
    const size_t o_tables = up16(cap);
    float* d_table = nullptr;
    if (!form.table.empty() && hipMalloc((void**)&d_table, form.table.size() * 4) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, who + ": hipMalloc of the tap table failed"); }

    std::vector<Row> batch; // the pieces of the batch being filled, byte_offset within the slot
    struct Copy { size_t at; const char* from; size_t bytes; };
    std::vector<Copy> copies;
    size_t used = 0;
    int slot = 0;
    Tables t;
    auto flush = [&]() -> int {
        if (batch.empty()) return FVAD_OK;
        if (!build_tables<typename F::Job>(batch, [&](const Row& s, typename F::Job& j) { return form.make(s, j); }, t))
            return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": more than 2^24 tiles in one batch");
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
            const int rc = form.launch(t, ring.dev[slot] + o_tables, d_table, ring.dev[slot]);
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
        if (d_table) FVAD_HIP(ctx, hipMemcpyAsync(d_table, form.table.data(), form.table.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        for (size_t i = 0; i < n_sources; ++i) {
            const Row s = row<Row>(sources, i);
            const uint64_t frame_bytes = s.n_channels * sample_bytes_of(s.format), total = s.*F::count;
            uint64_t done = 0;
            do { // (at least once: a source that writes no sample still queues its fill)
                size_t at = up16(used);
                uint64_t fit = at < cap ? form.fit(frame_bytes, cap - at) : 0;
                if ((fit == 0 && total - done > 0 && !batch.empty()) || batch.size() == F::kBatch) {
                    const int rc = flush();
                    if (rc != FVAD_OK) return rc;
                    at = 0;
                    fit = form.fit(frame_bytes, cap); // >= 4: the ring holds at least 1 KB and slot_min, a frame is at most 256 bytes
                }
                const uint64_t n = std::min<uint64_t>(total - done, fit);
                Row piece = s;
                const Bytes b = form.cut(piece, s, done, n);
                piece.byte_offset = at;
                piece.dst_offset = s.dst_offset + done;
                piece.fill_to = done + n == total ? s.fill_to : piece.dst_offset + n;
                batch.push_back(piece);
                if (b.n) {
                    copies.push_back({at, static_cast<const char*>(src_host[i]) + b.from, b.n});
                    used = at + b.n;
                }
                done += n;
            } while (done < total);
        }
        const int rc = flush();
        if (rc != FVAD_OK) return rc;
        FVAD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FVAD_OK;
    };
    const int rc = run();
    if (rc != FVAD_OK) (void)hipStreamSynchronize(ctx->stream);
    if (d_table) hipFree(d_table);
    return rc;
}

// ------------------------------------------------------------------ fvad_ingest*
struct Plain {
    using Row = Source;
    using Job = IngestJob;
    static constexpr uint64_t Source::*count = &Source::n_frames;
    static constexpr size_t kBatch = kBatchSources;
    fvad_ctx* ctx;
    int out_format;
    void* d_lanes;
    size_t lane_stride;
    std::vector<float> table; // none

    size_t slot_min(uint64_t) const { return 0; }
    uint64_t fit(uint64_t frame_bytes, size_t bytes) const { return bytes / frame_bytes / 4 * 4; } // frames, cut at multiples of 4
    Bytes cut(Source& piece, const Source& s, uint64_t done, uint64_t n) const
    {
        const uint64_t frame_bytes = s.n_channels * sample_bytes_of(s.format);
        piece.n_frames = n;
        return {s.byte_offset + done * frame_bytes, (size_t)(n * frame_bytes)};
    }
    uint64_t make(const Source& s, IngestJob& j) const
    {
        const uint64_t frame_bytes = s.n_channels * sample_bytes_of(s.format);
        j.tile_frames = (uint32_t)(kIngestTileBytes / frame_bytes / 4 * 4); // >= 64: a frame is at most 256 bytes
        j.src_off = s.byte_offset;
        j.n_frames = s.n_frames;
        return place(s, lane_stride, s.n_frames, j.tile_frames, j);
    }
    int launch(const Tables& t, const char* d_blob, const float*, const void* d_raw) const
    {
        return launch_tables(t, [&](int f, const Tables::Set& set) -> int {
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
            return FVAD_OK;
        });
    }
};

int check_plain(const fvad_ctx* ctx, const char* who, const uint64_t* sources, size_t n_sources, uint64_t raw_bytes, int out_format, const void* d_lanes,
                size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    return check_call(ctx, who, fvad_ingest_check(sources, n_sources, raw_bytes, out_format, n_lanes, lane_stride, n_samples), kOutOfRange,
                      ": a bad argument or source (fvad_ingest_check)", d_lanes, sample_bytes_of((uint64_t)out_format));
}

// ------------------------------------------------------------------ fvad_ingest_resample*
// The ring is cut in OUTPUT coordinates: a batch takes as many outputs of a source (in fours) as have their window in what is
// left of the slot, and the window's frames are what is copied -- so neighbouring pieces of a source overlap by the filter's
// reach, each piece's given frames cover its window, and by the check's rule the pieces' outputs are the file's.  A ring
// smaller than the window of 4 outputs of the call's widest source is enlarged to it for this call.
struct Resampled {
    using Row = RSource;
    using Job = IngestResampleJob;
    static constexpr uint64_t RSource::*count = &RSource::n_out;
    static constexpr size_t kBatch = 2048; // the ring's table room (kTableBytes, sized for fvad_ingest's jobs) holds this many of the larger resample jobs
    fvad_ctx* ctx;
    Ratio q;
    uint32_t n_taps;
    void* d_lanes;
    size_t lane_stride;
    std::vector<float> table;
    uint64_t window[3] = {0, 0, 0}; // per source format, the largest window a tile of the jobs made since its last launch stages (bytes)

    size_t slot_min(uint64_t frame_bytes) const { return up16((size_t)resample_reach(q, n_taps, 4) * (size_t)frame_bytes); } // (at most 64 KB: the tile rule)
    uint64_t fit(uint64_t frame_bytes, size_t bytes) const { return resample_fit(q, n_taps, frame_bytes, bytes, UINT64_MAX / 2); } // outputs whose window fits, in fours
    Bytes cut(RSource& piece, const RSource& s, uint64_t done, uint64_t n) const
    {
        const uint64_t frame_bytes = s.n_channels * sample_bytes_of(s.format);
        piece.out_from = s.out_from + done;
        piece.n_out = n;
        uint64_t lo, hi;
        resample_window(q, n_taps, s.file_frames, piece.out_from, n, &lo, &hi);
        piece.frame_base = lo;
        piece.n_frames = hi - lo;
        if (hi == lo) return {0, 0};
        return {s.byte_offset + (lo - s.frame_base) * frame_bytes, (size_t)((hi - lo) * frame_bytes)}; // (the check: the source's given frames cover [lo, hi))
    }
    uint64_t make(const RSource& s, IngestResampleJob& j)
    {
        j.tile_out = (uint32_t)resample_tile(q, n_taps, s.n_channels, s.format); // >= 4: the check refused 0
        j.src_off = s.byte_offset;
        j.frame_base = s.frame_base;
        j.file_frames = s.file_frames;
        j.out_from = s.out_from;
        j.n_out = s.n_out;
        if (s.n_out) window[s.format] = std::max<uint64_t>(window[s.format], (uint64_t)resample_reach(q, n_taps, j.tile_out) * (s.n_channels * sample_bytes_of(s.format)));
        return place(s, lane_stride, s.n_out, j.tile_out, j);
    }
    // (a launch asks for its format's largest window + 16 of LDS and clears it: the next batch's jobs start from none)
    int launch(const Tables& t, const char* d_blob, const float* d_table, const void* d_raw)
    {
        return launch_tables(t, [&](int f, const Tables::Set& set) -> int {
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
            a.lds_bytes = (uint32_t)up16(window[f] + 16);
            window[f] = 0;
            time_begin(ctx, "ingest_resample");
            FVAD_HIP(ctx, (hipError_t)fvad_launch_ingest_resample(a, ctx->stream));
            time_end(ctx);
            return FVAD_OK;
        });
    }
};
static_assert(3 * 32 + Resampled::kBatch * sizeof(IngestResampleJob) + (Resampled::kBatch + 3) * 4 + 3 * 16 <= kTableBytes, "the ring's table room");

int check_resampled(const fvad_ctx* ctx, const char* who, const uint64_t* sources, size_t n_sources, uint64_t raw_bytes, uint32_t up, uint32_t down,
                    const float* taps, uint32_t n_taps, const void* d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    return check_call(ctx, who, fvad_ingest_resample_check(sources, n_sources, raw_bytes, up, down, taps, n_taps, FVAD_INGEST_F32, n_lanes, lane_stride, n_samples),
                      kOutOfRange, ": a bad argument, ratio, tap or source (fvad_ingest_resample_check)", d_lanes, 4);
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
    const int bad = check_plain(ctx, "fvad_ingest_device", sources, n_sources, raw_bytes, out_format, d_lanes, n_lanes, lane_stride, n_samples);
    if (bad != FVAD_OK) return bad;
    if (n_sources == 0) return FVAD_OK;
    const Plain form{ctx, out_format, d_lanes, lane_stride, {}};
    return device_form<Source, IngestJob>(ctx, "fvad_ingest_device", "ingest in batches", "source tables", sources, n_sources, form.table,
                                          [&](const Source& s, IngestJob& j) { return form.make(s, j); },
                                          [&](const Tables& t, const char* d_blob, const float* d_table) { return form.launch(t, d_blob, d_table, d_raw); });
}

int fvad_ingest(fvad_ctx* ctx, const void* const* src_host, const uint64_t* sources, size_t n_sources, int out_format,
                void* d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sources && (!src_host || !d_lanes)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest: NULL argument");
    const int bad = check_plain(ctx, "fvad_ingest", sources, n_sources, UINT64_MAX, out_format, d_lanes, n_lanes, lane_stride, n_samples);
    if (bad != FVAD_OK) return bad;
    Plain form{ctx, out_format, d_lanes, lane_stride, {}};
    return host_form(ctx, "fvad_ingest", src_host, sources, n_sources, form);
}

int fvad_ingest_resample_device(fvad_ctx* ctx, const void* d_raw, uint64_t raw_bytes, const uint64_t* sources, size_t n_sources, uint32_t up,
                                uint32_t down, const float* taps, uint32_t n_taps, void* d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sources && (!d_raw || !d_lanes)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest_resample_device: NULL argument");
    const int bad = check_resampled(ctx, "fvad_ingest_resample_device", sources, n_sources, raw_bytes, up, down, taps, n_taps, d_lanes, n_lanes, lane_stride, n_samples);
    if (bad != FVAD_OK) return bad;
    if (n_sources == 0) return FVAD_OK;
    Resampled form{ctx, Ratio{up, down}, n_taps, d_lanes, lane_stride, resample_table(Taps{taps, n_taps}, Ratio{up, down})};
    return device_form<RSource, IngestResampleJob>(ctx, "fvad_ingest_resample_device", "ingest in batches", "tables", sources, n_sources, form.table,
                                                   [&](const RSource& s, IngestResampleJob& j) { return form.make(s, j); },
                                                   [&](const Tables& t, const char* d_blob, const float* d_table) { return form.launch(t, d_blob, d_table, d_raw); });
}

int fvad_ingest_resample(fvad_ctx* ctx, const void* const* src_host, const uint64_t* sources, size_t n_sources, uint32_t up, uint32_t down,
                         const float* taps, uint32_t n_taps, void* d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sources && (!src_host || !d_lanes)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_ingest_resample: NULL argument");
    const int bad = check_resampled(ctx, "fvad_ingest_resample", sources, n_sources, UINT64_MAX, up, down, taps, n_taps, d_lanes, n_lanes, lane_stride, n_samples);
    if (bad != FVAD_OK) return bad;
    Resampled form{ctx, Ratio{up, down}, n_taps, d_lanes, lane_stride, resample_table(Taps{taps, n_taps}, Ratio{up, down})};
    return host_form(ctx, "fvad_ingest_resample", src_host, sources, n_sources, form);
}

} // extern "C"
