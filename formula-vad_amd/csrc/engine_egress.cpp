// engine_egress.cpp -- the egress calls, each in a device form (bytes into device memory) and a host form (bytes into host
// memory): planar device lanes into the interleaved bytes of files' data chunks.
//   fvad_egress*                   lanes as they are (kernels_egress.hip; the rules are fvad_egress_check's, host_egress.cpp)
//   fvad_egress_resample*          48 kHz lanes resampled to another rate (kernels_egress_resample.hip; host_egress_resample.cpp;
//                                  the tile is egress_resample.h's)
//   fvad_egress_resample_strided*  the same over a stream that lies src_step apart in its lanes (host_egress_strided.cpp)
//   fvad_egress_mix*               two sets of f32 lanes, weighted and summed (kernels_egress_mix.hip; host_egress_mix.cpp)
// What the forms share is written once: the tables a launch searches and the device form's upload-launch-wait (io_tables.h,
// shared with engine_ingest.cpp) and, for bytes in host memory, the batches through the two-slot page-locked ring (host_form
// below).  A form supplies its row, how a row is cut, the job of a row and the launch of one file format's jobs.
// The ring is fvad_ingest's own (Workspace::IngestRing, sized by the context option ingest_ring_bytes), SHARED, not a second
// one: every one of these calls returns only when its last batch is done, so the ring is idle whenever one starts, a slot of
// it is what a call here needs as well -- one contiguous device image, its page-locked twin and room for a batch's tables
// behind them -- and a context that reads and writes a corpus keeps 2 x 32 MB of page-locked memory instead of 4 x.  ev[s] here
// means: slot s's bytes have arrived in its page-locked buffer.
#include <algorithm>
#include <cstring>
#include <vector>

#include "egress_mix.h"
#include "egress_strided.h"
#include "internal.h"
#include "io_tables.h"

using namespace fvad;

namespace {

static_assert(kEgressResampleTileBytes == (uint64_t)kIngestTileBytes && kEgressResampleWindow == (uint64_t)kClipTile, "egress_resample.h restates the kernel's tile");

// The rows of the three table layouts, field for field (fvad.h), so that a row is decoded by a copy (row<Row>).  Each begins
// byte_offset, its count (the frames it writes), n_channels, format; the job of a row without frames has 0 tiles, so it gets none.
struct Sink { uint64_t byte_offset, n_frames, n_channels, format, first_lane, src_offset; };
struct ResampleRow { uint64_t byte_offset, n_out, n_channels, format, first_lane, src_offset, frame_base, n_frames, stream_frames, out_from; };
struct MixSink { uint64_t byte_offset, n_frames, n_channels, format, first_lane, src_offset, orig_offset, orig_zeros; };
static_assert(sizeof(Sink) == FVAD_EGRESS_FIELDS * 8 && sizeof(ResampleRow) == FVAD_EGRESS_RESAMPLE_FIELDS * 8 && sizeof(MixSink) == FVAD_EGRESS_MIX_FIELDS * 8, "fvad.h's rows");

// The rules of a host form see every row's bytes at their absolute host address: two rows of one file, or of overlapping
// buffers, overlap there.  An address that wraps is saturated, which the range rule then refuses.
std::vector<uint64_t> placed_rows(const uint64_t* sinks, size_t n_sinks, size_t n_fields, void* const* dst_host)
{
    std::vector<uint64_t> placed(sinks, sinks + n_sinks * n_fields);
    for (size_t i = 0; i < n_sinks; ++i) {
        uint64_t& at = placed[i * n_fields];
        const uint64_t base = (uint64_t)(uintptr_t)dst_host[i];
        at = at > UINT64_MAX - base ? UINT64_MAX : base + at;
    }
    return placed;
}

// a row that writes something has somewhere to write it
bool rows_have_bytes(const uint64_t* sinks, size_t n_sinks, size_t n_fields, void* const* dst_host)
{
    for (size_t i = 0; i < n_sinks; ++i)
        if (!dst_host[i] && sinks[i * n_fields + 1]) return false;
    return true;
}

// The host form behind its refusals.  Batches of at most ring_bytes output bytes: the rows' pieces are given places one after
// the other in a slot's device image (each on a 16-byte boundary), the batch's tables go up behind them, the kernels write the
// image, one DMA brings it to the slot's page-locked twin -- and while the device works on that, this thread moves the OTHER
// slot's batch from its page-locked buffer to where the caller wants it (memcpy: a mapped file's pages are written by the host
// alone).  A row that does not fit what is left of a batch is cut at a multiple of 4 frames; a piece is a row of its own --
// the row at its place in the slot, with the piece's frames and what advance(piece, done) changes for a piece that starts at
// the row's frame `done` --, so the bytes are the same however the rows are cut.  The bytes between two pieces of a slot are
// never copied out.  A batch holds at most batch_cap pieces (its tables fit the ring's table room); the tap table of a form
// that has one goes up once per call, and launch(t, d_blob, d_table, d_out) queues a batch's kernels.
template <typename Row, typename Job, typename Advance, typename Make, typename Launch>
int host_form(fvad_ctx* ctx, const std::string& who, const uint64_t* sinks, size_t n_sinks, void* const* dst_host, uint64_t Row::*count,
              size_t batch_cap, const std::vector<float>& table, Advance advance, Make make, Launch launch)
{
    hipSetDevice(ctx->device);
    const size_t cap = (size_t)ctx->tune.ingest_ring_bytes;
    size_t table_room = 0;
    const int rc0 = ingest_ring_ensure(ctx, cap, &table_room);
    if (rc0 != FVAD_OK) return rc0;
    Workspace::IngestRing& ring = ctx->ws.ingest;
    const size_t o_tables = up16(cap);
    float* d_table = nullptr;
    if (!table.empty() && hipMalloc((void**)&d_table, table.size() * 4) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, who + ": hipMalloc of the tap table failed"); }

    std::vector<Row> batch;                               // the pieces of the batch being planned, byte_offset within the slot
    struct Move { size_t at; char* to; size_t bytes; };
    std::vector<Move> moves, pending[2];                  // pending[s]: what slot s's page-locked buffer holds for the caller
    size_t used = 0;
    int slot = 0;
    Tables t;
    auto drain = [&](int s) -> int {
        if (pending[s].empty()) return FVAD_OK;
        FVAD_HIP(ctx, hipEventSynchronize(ring.ev[s])); // the slot's bytes have arrived
        for (const Move& m : pending[s]) memcpy(m.to, ring.pin[s] + m.at, m.bytes);
        pending[s].clear();
        return FVAD_OK;
    };
    auto flush = [&]() -> int {
        if (batch.empty()) return FVAD_OK;
        if (!build_tables<Job>(batch, make, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": more than 2^24 tiles in one batch");
        if (t.blob.size() > table_room) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": a batch's tables outgrew the ring"); // (batch_cap keeps them inside)
        // the slot is free: the batch it held was drained while the other slot's was in flight
        memcpy(ring.pin[slot] + o_tables, t.blob.data(), t.blob.size());
        FVAD_HIP(ctx, hipMemcpyAsync(ring.dev[slot] + o_tables, ring.pin[slot] + o_tables, t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
        const int rc = launch(t, ring.dev[slot] + o_tables, d_table, ring.dev[slot]);
        if (rc != FVAD_OK) return rc;
        FVAD_HIP(ctx, hipMemcpyAsync(ring.pin[slot], ring.dev[slot], used, hipMemcpyDeviceToHost, ctx->stream));
        FVAD_HIP(ctx, hipEventRecord(ring.ev[slot], ctx->stream));
        pending[slot].swap(moves);
        const int rc1 = drain(slot ^ 1); // the previous batch, while the device works on this one
        if (rc1 != FVAD_OK) return rc1;
        slot ^= 1;
        batch.clear();
        moves.clear();
        used = 0;
        return FVAD_OK;
    };
    auto run = [&]() -> int {
        if (d_table) FVAD_HIP(ctx, hipMemcpyAsync(d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        for (size_t i = 0; i < n_sinks; ++i) {
            const Row s = row<Row>(sinks, i);
            const uint64_t frame_bytes = s.n_channels * sample_bytes_of(s.format);
            uint64_t done = 0;
            while (done < s.*count) {
                size_t at = up16(used);
                uint64_t fit = at < cap ? (cap - at) / frame_bytes / 4 * 4 : 0; // frames that fit, cut at multiples of 4
                if ((fit == 0 && !batch.empty()) || batch.size() == batch_cap) {
                    const int rc = flush();
                    if (rc != FVAD_OK) return rc;
                    at = 0;
                    fit = cap / frame_bytes / 4 * 4; // >= 4: the ring holds at least 1 KB, a frame is at most 256 bytes
                }
                const uint64_t n = std::min<uint64_t>(s.*count - done, fit);
                Row piece = s;
                piece.byte_offset = at;
                piece.*count = n;
                advance(piece, done);
                batch.push_back(piece);
                moves.push_back({at, static_cast<char*>(dst_host[i]) + s.byte_offset + done * frame_bytes, (size_t)(n * frame_bytes)});
                used = at + (size_t)(n * frame_bytes);
                done += n;
            }
        }
        const int rc = flush();
        if (rc != FVAD_OK) return rc;
        const int rc1 = drain(slot); // (empty unless a flush failed half-way; the older batch first)
        if (rc1 != FVAD_OK) return rc1;
        return drain(slot ^ 1);
    };
    const int rc = run();
    (void)hipStreamSynchronize(ctx->stream); // the ring is idle when the call returns, whatever happened
    if (d_table) hipFree(d_table);
    return rc;
}

// the pieces a batch holds at most: the ring's table room is sized for 4096 IngestJobs in three sets
constexpr size_t kBatchSinks = 4096; // fvad_egress, fvad_egress_mix
constexpr size_t kBatchRows = 2048;  // fvad_egress_resample*
static_assert(sizeof(EgressJob) <= sizeof(IngestJob) && sizeof(EgressMixJob) <= sizeof(IngestJob), "the ring's table room");
static_assert(kBatchRows * sizeof(EgressResampleJob) <= 4096 * sizeof(IngestJob), "the ring's table room");

// ------------------------------------------------------------------ fvad_egress*
// the lanes of a call
struct Lanes { const void* d; int src_format; size_t lane_stride; };

int check_plain(const fvad_ctx* ctx, const std::string& who, const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, const Lanes& l, size_t n_lanes,
                size_t n_samples)
{
    const int rc = fvad_egress_check(sinks, n_sinks, out_bytes, l.src_format, n_lanes, l.lane_stride, n_samples);
    if (rc != FVAD_OK) return set_err(ctx, rc, who + (rc == FVAD_ERR_OUT_OF_RANGE ? ": a sink's lanes, samples or bytes are out of range"
                                                                                    : ": a bad argument or sink (fvad_egress_check)"));
    if ((uintptr_t)l.d % (l.src_format == FVAD_INGEST_PCM16 ? 2 : 4) != 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": the lanes are not aligned to their samples");
    return FVAD_OK;
}

// a piece from frame `done` on reads its lanes from there
void advance_plain(Sink& piece, uint64_t done) { piece.src_offset += done; }

auto make_plain(const Lanes& l)
{
    return [l](const Sink& s, EgressJob& j) -> uint64_t {
        const uint64_t frame_bytes = s.n_channels * sample_bytes_of(s.format);
        j.tile_frames = (uint32_t)(kIngestTileBytes / frame_bytes / 4 * 4); // >= 64: a frame is at most 256 bytes
        j.dst_off = s.byte_offset;
        j.n_frames = s.n_frames;
        j.src_off = s.first_lane * (uint64_t)l.lane_stride + s.src_offset;
        const uint64_t nt = (s.n_frames + j.tile_frames - 1) / j.tile_frames;
        j.n_tiles = (uint32_t)nt; // (more than kMaxUnits are refused)
        j.n_channels = (uint32_t)s.n_channels;
        return nt;
    };
}

int launch_plain(fvad_ctx* ctx, const Lanes& l, const Tables& t, const char* d_blob, void* d_out)
{
    return launch_tables(t, [&](int f, const Tables::Set& set) -> int {
        EgressArgs a{};
        a.lanes = l.d;
        a.lane_stride = l.lane_stride;
        a.out = static_cast<uint8_t*>(d_out);
        a.jobs = reinterpret_cast<const EgressJob*>(d_blob + set.o_jobs);
        a.unit_prefix = reinterpret_cast<const uint32_t*>(d_blob + set.o_prefix);
        a.n_jobs = set.n_jobs;
        a.n_units = set.n_units;
        a.src_format = l.src_format;
        a.file_format = f;
        time_begin(ctx, "egress");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_egress(a, ctx->stream));
        time_end(ctx);
        return FVAD_OK;
    });
}

// ------------------------------------------------------------------ fvad_egress_resample* and fvad_egress_resample_strided*
// the lanes, the filter and the step of a call (step 0: a plain entry, which launches the kernel over contiguous lanes)
struct Resampled { const void* d; size_t lane_stride; Ratio q; const float* taps; uint32_t n_taps; bool strided; uint32_t step; };

int check_resampled(const fvad_ctx* ctx, const std::string& who, const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, const Resampled& r, int src_format,
                    size_t n_lanes, size_t n_samples)
{
    const int rc = egress_resample_check(sinks, n_sinks, out_bytes, r.q.up, r.q.down, r.taps, r.n_taps, r.strided, r.step, src_format, n_lanes, r.lane_stride, n_samples);
    if (rc != FVAD_OK) return set_err(ctx, rc, who + (rc == FVAD_ERR_OUT_OF_RANGE ? ": a row's lanes, samples or bytes are out of range"
                                                      : r.strided                  ? ": a bad argument, ratio, step, tap or row (fvad_egress_resample_strided_check)"
                                                                                    : ": a bad argument, ratio, tap or row (fvad_egress_resample_check)"));
    if ((uintptr_t)r.d % 4 != 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": the lanes are not aligned to their samples");
    return FVAD_OK;
}

// Cut in OUTPUT frames: a piece is the row with out_from advanced and the SAME given frames -- they cover the row's window, so
// they cover the piece's, and the lanes are on the device already: nothing of the window is copied and the bytes cannot depend
// on the cut.
void advance_resampled(ResampleRow& piece, uint64_t done) { piece.out_from += done; }

auto make_resampled(const Resampled& r)
{
    return [r](const ResampleRow& s, EgressResampleJob& j) -> uint64_t {
        j.tile_out = (uint32_t)egress_resample_tile(r.q, r.n_taps, s.n_channels, s.format); // >= 4: the check refused 0
        j.dst_off = s.byte_offset;
        j.out_from = s.out_from;
        j.n_out = s.n_out;
        j.src_off = s.first_lane * (uint64_t)r.lane_stride + s.src_offset;
        j.frame_base = s.frame_base;
        j.stream_frames = s.stream_frames;
        const uint64_t nt = (s.n_out + j.tile_out - 1) / j.tile_out;
        j.n_tiles = (uint32_t)nt; // (more than kMaxUnits are refused)
        j.n_channels = (uint32_t)s.n_channels;
        return nt;
    };
}

int launch_resampled(fvad_ctx* ctx, const Resampled& r, const Tables& t, const char* d_blob, const float* d_table, void* d_out)
{
    return launch_tables(t, [&](int f, const Tables::Set& set) -> int {
        EgressResampleArgs a{};
        a.lanes = static_cast<const float*>(r.d);
        a.lane_stride = r.lane_stride;
        a.out = static_cast<uint8_t*>(d_out);
        a.jobs = reinterpret_cast<const EgressResampleJob*>(d_blob + set.o_jobs);
        a.unit_prefix = reinterpret_cast<const uint32_t*>(d_blob + set.o_prefix);
        a.table = d_table;
        a.n_jobs = set.n_jobs;
        a.n_units = set.n_units;
        a.up = r.q.up;
        a.down = r.q.down;
        a.n_taps = r.n_taps;
        a.file_format = f;
        time_begin(ctx, r.step ? "egress_strided" : "egress_resample");
        FVAD_HIP(ctx, (hipError_t)(r.step ? fvad_launch_egress_strided(EgressStridedArgs{a, r.step}, ctx->stream) : fvad_launch_egress_resample(a, ctx->stream)));
        time_end(ctx);
        return FVAD_OK;
    });
}

// the device form of both entries (strided: `step` is the caller's, checked below; otherwise 0)
int resampled_device(fvad_ctx* ctx, const std::string& who, const Resampled& r, int src_format, size_t n_lanes, size_t n_samples, const uint64_t* sinks,
                     size_t n_sinks, void* d_out, uint64_t out_bytes)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks && (!r.d || !d_out)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": NULL argument");
    const int bad = check_resampled(ctx, who, sinks, n_sinks, out_bytes, r, src_format, n_lanes, n_samples);
    if (bad != FVAD_OK) return bad;
    if (n_sinks == 0) return FVAD_OK;
    return device_form<ResampleRow, EgressResampleJob>(ctx, who, "write in batches", "tables", sinks, n_sinks, resample_table(Taps{r.taps, r.n_taps}, r.q), make_resampled(r),
                                                       [&](const Tables& t, const char* d_blob, const float* d_table) { return launch_resampled(ctx, r, t, d_blob, d_table, d_out); });
}

int resampled_host(fvad_ctx* ctx, const std::string& who, const Resampled& r, int src_format, size_t n_lanes, size_t n_samples, const uint64_t* sinks,
                   size_t n_sinks, void* const* dst_host)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks && (!dst_host || !r.d)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": NULL argument");
    if (n_sinks && !sinks) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": NULL sinks");
    const int bad = check_resampled(ctx, who, placed_rows(sinks, n_sinks, FVAD_EGRESS_RESAMPLE_FIELDS, dst_host).data(), n_sinks, UINT64_MAX, r, src_format, n_lanes, n_samples);
    if (bad != FVAD_OK) return bad;
    if (!rows_have_bytes(sinks, n_sinks, FVAD_EGRESS_RESAMPLE_FIELDS, dst_host)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": a row with outputs and no bytes");
    if (n_sinks == 0) return FVAD_OK;
    return host_form<ResampleRow, EgressResampleJob>(ctx, who, sinks, n_sinks, dst_host, &ResampleRow::n_out, kBatchRows, resample_table(Taps{r.taps, r.n_taps}, r.q), advance_resampled,
                                                     make_resampled(r), [&](const Tables& t, const char* d_blob, const float* d_table, void* d_out) {
                                                         return launch_resampled(ctx, r, t, d_blob, d_table, d_out);
                                                     });
}

// ------------------------------------------------------------------ fvad_egress_mix*
// the two lane sets and the weights of a call
struct Mixed {
    const void *d_orig, *d_den;
    size_t orig_stride, orig_samples, den_stride, den_samples, n_lanes;
    float w_orig, w_den;
};

// the check, then what it cannot see: the lanes of a source whose weight is not zero are there and aligned to their samples
int check_mixed(const fvad_ctx* ctx, const std::string& who, const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, int src_format, const Mixed& l)
{
    const int rc = fvad_egress_mix_check(sinks, n_sinks, out_bytes, src_format, l.w_orig, l.w_den, l.n_lanes, l.orig_stride, l.orig_samples,
                                         l.den_stride, l.den_samples);
    if (rc != FVAD_OK) return set_err(ctx, rc, who + (rc == FVAD_ERR_OUT_OF_RANGE ? ": a sink's lanes, samples or bytes are out of range"
                                                                                    : ": a bad argument or sink (fvad_egress_mix_check)"));
    if (n_sinks && ((l.w_orig != 0.0f && !l.d_orig) || (l.w_den != 0.0f && !l.d_den)))
        return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": NULL lanes with a weight that is not zero");
    if ((l.w_orig != 0.0f && (uintptr_t)l.d_orig % 4 != 0) || (l.w_den != 0.0f && (uintptr_t)l.d_den % 4 != 0))
        return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": the lanes are not aligned to their samples");
    return FVAD_OK;
}

// the piece from frame `done` on is the sink with src_offset advanced by done, orig_zeros lowered by min(orig_zeros, done) and
// orig_offset advanced by the rest of done -- the same pairing
void advance_mixed(MixSink& piece, uint64_t done)
{
    const uint64_t zeros_done = std::min(piece.orig_zeros, done);
    piece.src_offset += done;
    piece.orig_zeros -= zeros_done;
    piece.orig_offset += done - zeros_done;
}

auto make_mixed(const Mixed& l)
{
    return [l](const MixSink& s, EgressMixJob& j) -> uint64_t {
        const uint64_t frame_bytes = s.n_channels * sample_bytes_of(s.format);
        j.tile_frames = (uint32_t)(kIngestTileBytes / frame_bytes / 4 * 4); // >= 64: a frame is at most 256 bytes
        j.dst_off = s.byte_offset;
        j.n_frames = s.n_frames;
        // (the offsets of a source whose weight is zero are not checked and not used: they may wrap)
        j.den_off = s.first_lane * (uint64_t)l.den_stride + s.src_offset;
        j.orig_off = s.first_lane * (uint64_t)l.orig_stride + s.orig_offset;
        j.orig_zeros = s.orig_zeros;
        j.n_channels = (uint32_t)s.n_channels;
        return (s.n_frames + j.tile_frames - 1) / j.tile_frames;
    };
}

int launch_mixed(fvad_ctx* ctx, const Mixed& l, const Tables& t, const char* d_blob, void* d_out)
{
    return launch_tables(t, [&](int f, const Tables::Set& set) -> int {
        EgressMixArgs a{};
        a.orig = static_cast<const float*>(l.d_orig);
        a.den = static_cast<const float*>(l.d_den);
        a.orig_stride = l.orig_stride;
        a.den_stride = l.den_stride;
        a.out = static_cast<uint8_t*>(d_out);
        a.jobs = reinterpret_cast<const EgressMixJob*>(d_blob + set.o_jobs);
        a.unit_prefix = reinterpret_cast<const uint32_t*>(d_blob + set.o_prefix);
        a.n_jobs = set.n_jobs;
        a.n_units = set.n_units;
        a.w_orig = l.w_orig;
        a.w_den = l.w_den;
        a.file_format = f;
        time_begin(ctx, "egress_mix");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_egress_mix(a, ctx->stream));
        time_end(ctx);
        return FVAD_OK;
    });
}

} // namespace

extern "C" {

int fvad_egress_device(fvad_ctx* ctx, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                       const uint64_t* sinks, size_t n_sinks, void* d_out, uint64_t out_bytes)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks && (!d_lanes || !d_out)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_device: NULL argument");
    const Lanes l{d_lanes, src_format, lane_stride};
    const int bad = check_plain(ctx, "fvad_egress_device", sinks, n_sinks, out_bytes, l, n_lanes, n_samples);
    if (bad != FVAD_OK) return bad;
    if (n_sinks == 0) return FVAD_OK;
    return device_form<Sink, EgressJob>(ctx, "fvad_egress_device", "write in batches", "sink tables", sinks, n_sinks, {}, make_plain(l),
                                        [&](const Tables& t, const char* d_blob, const float*) { return launch_plain(ctx, l, t, d_blob, d_out); });
}

int fvad_egress(fvad_ctx* ctx, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                const uint64_t* sinks, size_t n_sinks, void* const* dst_host)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks && (!dst_host || !d_lanes)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress: NULL argument");
    if (n_sinks && !sinks) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress: NULL sinks");
    const Lanes l{d_lanes, src_format, lane_stride};
    const int bad = check_plain(ctx, "fvad_egress", placed_rows(sinks, n_sinks, FVAD_EGRESS_FIELDS, dst_host).data(), n_sinks, UINT64_MAX, l, n_lanes, n_samples);
    if (bad != FVAD_OK) return bad;
    if (!rows_have_bytes(sinks, n_sinks, FVAD_EGRESS_FIELDS, dst_host)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress: a sink with frames and no bytes");
    if (n_sinks == 0) return FVAD_OK;
    return host_form<Sink, EgressJob>(ctx, "fvad_egress", sinks, n_sinks, dst_host, &Sink::n_frames, kBatchSinks, {}, advance_plain, make_plain(l),
                                      [&](const Tables& t, const char* d_blob, const float*, void* d_out) { return launch_plain(ctx, l, t, d_blob, d_out); });
}

int fvad_egress_resample_device(fvad_ctx* ctx, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                const uint64_t* sinks, size_t n_sinks, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps,
                                void* d_out, uint64_t out_bytes)
{
    return resampled_device(ctx, "fvad_egress_resample_device", Resampled{d_lanes, lane_stride, Ratio{up, down}, taps, n_taps, false, 0}, src_format, n_lanes, n_samples, sinks, n_sinks, d_out, out_bytes);
}

int fvad_egress_resample(fvad_ctx* ctx, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                         const uint64_t* sinks, size_t n_sinks, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps,
                         void* const* dst_host)
{
    return resampled_host(ctx, "fvad_egress_resample", Resampled{d_lanes, lane_stride, Ratio{up, down}, taps, n_taps, false, 0}, src_format, n_lanes, n_samples, sinks, n_sinks, dst_host);
}

int fvad_egress_resample_strided_device(fvad_ctx* ctx, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                        const uint64_t* sinks, size_t n_sinks, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps,
                                        uint32_t src_step, void* d_out, uint64_t out_bytes)
{
    return resampled_device(ctx, "fvad_egress_resample_strided_device", Resampled{d_lanes, lane_stride, Ratio{up, down}, taps, n_taps, true, src_step}, src_format, n_lanes, n_samples, sinks, n_sinks, d_out, out_bytes);
}

int fvad_egress_resample_strided(fvad_ctx* ctx, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                 const uint64_t* sinks, size_t n_sinks, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps,
                                 uint32_t src_step, void* const* dst_host)
{
    return resampled_host(ctx, "fvad_egress_resample_strided", Resampled{d_lanes, lane_stride, Ratio{up, down}, taps, n_taps, true, src_step}, src_format, n_lanes, n_samples, sinks, n_sinks, dst_host);
}

int fvad_egress_mix_device(fvad_ctx* ctx, const void* d_orig, size_t orig_stride, size_t orig_samples, const void* d_den, size_t den_stride,
                           size_t den_samples, int src_format, size_t n_lanes, float w_orig, float w_den, const uint64_t* sinks, size_t n_sinks,
                           void* d_out, uint64_t out_bytes)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks && !d_out) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_mix_device: NULL argument");
    const Mixed l{d_orig, d_den, orig_stride, orig_samples, den_stride, den_samples, n_lanes, w_orig, w_den};
    const int bad = check_mixed(ctx, "fvad_egress_mix_device", sinks, n_sinks, out_bytes, src_format, l);
    if (bad != FVAD_OK) return bad;
    if (n_sinks == 0) return FVAD_OK;
    return device_form<MixSink, EgressMixJob>(ctx, "fvad_egress_mix_device", "write in batches", "sink tables", sinks, n_sinks, {}, make_mixed(l),
                                              [&](const Tables& t, const char* d_blob, const float*) { return launch_mixed(ctx, l, t, d_blob, d_out); });
}

int fvad_egress_mix(fvad_ctx* ctx, const void* d_orig, size_t orig_stride, size_t orig_samples, const void* d_den, size_t den_stride,
                    size_t den_samples, int src_format, size_t n_lanes, float w_orig, float w_den, const uint64_t* sinks, size_t n_sinks,
                    void* const* dst_host)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks && !dst_host) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_mix: NULL argument");
    if (n_sinks && !sinks) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_mix: NULL sinks");
    const Mixed l{d_orig, d_den, orig_stride, orig_samples, den_stride, den_samples, n_lanes, w_orig, w_den};
    const int bad = check_mixed(ctx, "fvad_egress_mix", placed_rows(sinks, n_sinks, FVAD_EGRESS_MIX_FIELDS, dst_host).data(), n_sinks, UINT64_MAX, src_format, l);
    if (bad != FVAD_OK) return bad;
    if (!rows_have_bytes(sinks, n_sinks, FVAD_EGRESS_MIX_FIELDS, dst_host)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_mix: a sink with frames and no bytes");
    if (n_sinks == 0) return FVAD_OK;
    return host_form<MixSink, EgressMixJob>(ctx, "fvad_egress_mix", sinks, n_sinks, dst_host, &MixSink::n_frames, kBatchSinks, {}, advance_mixed, make_mixed(l),
                                            [&](const Tables& t, const char* d_blob, const float*, void* d_out) { return launch_mixed(ctx, l, t, d_blob, d_out); });
}

} // extern "C"
