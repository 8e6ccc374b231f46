// engine_egress.cpp -- fvad_egress_device / fvad_egress: planar device lanes into the interleaved bytes of files' data chunks
// with kernels_egress.hip.  The argument rules are fvad_egress_check's (host_egress.cpp); here are the tables a launch searches
// and, for bytes in host memory, the two-slot page-locked ring that carries them from the device.
// The ring is fvad_ingest's own (Workspace::IngestRing, sized by the context option ingest_ring_bytes), SHARED, not a second
// one: both calls return only when their last batch is done, so the ring is idle whenever either starts, a slot of it is what
// this call needs as well -- one contiguous device image, its page-locked twin and room for a batch's tables behind them -- and
// a context that reads and writes a corpus keeps 2 x 32 MB of page-locked memory instead of 4 x.  ev[s] here means: slot s's
// bytes have arrived in its page-locked buffer.
#include <algorithm>
#include <cstring>
#include <vector>

#include "internal.h"

using namespace fvad;

namespace {

struct Sink { uint64_t byte_offset, n_frames, n_channels, format, first_lane, src_offset; };
Sink row(const uint64_t* sinks, size_t i)
{
    const uint64_t* r = sinks + i * FVAD_EGRESS_FIELDS;
    return {r[0], r[1], r[2], r[3], r[4], r[5]};
}
uint64_t sample_bytes(uint64_t format) { return format == FVAD_INGEST_PCM16 ? 2 : format == FVAD_INGEST_PCM24 ? 3 : 4; }
size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// The tables of one call or batch: per file format (a launch encodes one) the jobs and their unit prefix, laid out in ONE blob
// whose parts start on 16-byte boundaries, so that one copy carries them to the device (engine_ingest.cpp's layout).
struct Tables {
    struct Set { size_t o_jobs = 0, o_prefix = 0; uint32_t n_jobs = 0, n_units = 0; } set[3];
    std::vector<char> blob;
};

// as for the ingest: a launch is one workgroup of 256 lanes per unit and takes fewer than 2^24 units (about 270 GB of output)
constexpr uint64_t kMaxUnits = (1ull << 24) - 1;

// false: more than kMaxUnits units in one launch
bool build_tables(const std::vector<Sink>& sinks, size_t lane_stride, Tables& t)
{
    t.blob.clear();
    for (int f = 0; f < 3; ++f) {
        std::vector<EgressJob> jobs;
        std::vector<uint32_t> prefix;
        uint64_t units = 0;
        for (const Sink& s : sinks) {
            if ((int)s.format != f || s.n_frames == 0) continue; // (a sink without frames writes nothing)
            EgressJob j{};
            const uint64_t frame_bytes = s.n_channels * sample_bytes(s.format);
            j.tile_frames = (uint32_t)(kIngestTileBytes / frame_bytes / 4 * 4); // >= 64: a frame is at most 256 bytes
            j.dst_off = s.byte_offset;
            j.n_frames = s.n_frames;
            j.src_off = s.first_lane * (uint64_t)lane_stride + s.src_offset;
            const uint64_t nt = (s.n_frames + j.tile_frames - 1) / j.tile_frames;
            if (nt > kMaxUnits) return false;
            j.n_tiles = (uint32_t)nt;
            j.n_channels = (uint32_t)s.n_channels;
            prefix.push_back((uint32_t)units);
            jobs.push_back(j);
            units += nt;
            if (units > kMaxUnits) return false;
        }
        Tables::Set& set = t.set[f];
        set.n_jobs = (uint32_t)jobs.size();
        set.n_units = (uint32_t)units;
        if (jobs.empty()) continue;
        prefix.push_back((uint32_t)units);
        set.o_jobs = t.blob.size();
        set.o_prefix = set.o_jobs + up16(jobs.size() * sizeof(EgressJob));
        t.blob.resize(set.o_prefix + up16(prefix.size() * 4));
        memcpy(t.blob.data() + set.o_jobs, jobs.data(), jobs.size() * sizeof(EgressJob));
        memcpy(t.blob.data() + set.o_prefix, prefix.data(), prefix.size() * 4);
    }
    return true;
}

// the launches of one set of tables whose blob is at d_blob (queued on ctx->stream)
int launch_tables(fvad_ctx* ctx, const Tables& t, const char* d_blob, const void* d_lanes, int src_format, size_t lane_stride, void* d_out)
{
    for (int f = 0; f < 3; ++f) {
        const Tables::Set& set = t.set[f];
        if (!set.n_units) continue;
        EgressArgs a{};
        a.lanes = d_lanes;
        a.lane_stride = lane_stride;
        a.out = static_cast<uint8_t*>(d_out);
        a.jobs = reinterpret_cast<const EgressJob*>(d_blob + set.o_jobs);
        a.unit_prefix = reinterpret_cast<const uint32_t*>(d_blob + set.o_prefix);
        a.n_jobs = set.n_jobs;
        a.n_units = set.n_units;
        a.src_format = src_format;
        a.file_format = f;
        time_begin(ctx, "egress");
        FVAD_HIP(ctx, (hipError_t)fvad_launch_egress(a, ctx->stream));
        time_end(ctx);
    }
    return FVAD_OK;
}

int check_call(const fvad_ctx* ctx, const char* who, const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, int src_format,
               const void* d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples)
{
    const int rc = fvad_egress_check(sinks, n_sinks, out_bytes, src_format, n_lanes, lane_stride, n_samples);
    if (rc != FVAD_OK) return set_err(ctx, rc, std::string(who) + (rc == FVAD_ERR_OUT_OF_RANGE ? ": a sink's lanes, samples or bytes are out of range"
                                                                                                 : ": a bad argument or sink (fvad_egress_check)"));
    if ((uintptr_t)d_lanes % (src_format == FVAD_INGEST_PCM16 ? 2 : 4) != 0)
        return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, std::string(who) + ": the lanes are not aligned to their samples");
    return FVAD_OK;
}

// the pieces a batch of fvad_egress holds at most: the ring's table room is sized for as many IngestJobs in three sets
constexpr size_t kBatchSinks = 4096;
static_assert(sizeof(EgressJob) <= sizeof(IngestJob), "the ring's table room");

} // namespace

extern "C" {

int fvad_egress_device(fvad_ctx* ctx, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                       const uint64_t* sinks, size_t n_sinks, void* d_out, uint64_t out_bytes)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks && (!d_lanes || !d_out)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_device: NULL argument");
    const int bad = check_call(ctx, "fvad_egress_device", sinks, n_sinks, out_bytes, src_format, d_lanes, n_lanes, lane_stride, n_samples);
    if (bad != FVAD_OK) return bad;
    if (n_sinks == 0) return FVAD_OK;
    std::vector<Sink> all(n_sinks);
    for (size_t i = 0; i < n_sinks; ++i) all[i] = row(sinks, i);
    Tables t;
    if (!build_tables(all, lane_stride, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_device: more than 2^24 tiles in one call: write in batches");
    if (t.blob.empty()) return FVAD_OK; // nothing to write
    hipSetDevice(ctx->device);
    char* d = nullptr;
    if (hipMalloc((void**)&d, t.blob.size()) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "fvad_egress_device: hipMalloc of the sink tables failed"); }
    auto run = [&]() -> int {
        FVAD_HIP(ctx, hipMemcpyAsync(d, t.blob.data(), t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
        const int rc = launch_tables(ctx, t, d, d_lanes, src_format, lane_stride, d_out);
        if (rc != FVAD_OK) return rc;
        FVAD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FVAD_OK;
    };
    const int rc = run();
    if (rc != FVAD_OK) (void)hipStreamSynchronize(ctx->stream);
    hipFree(d);
    return rc;
}

// Batches of at most ring_bytes output bytes: the sinks' pieces are given places one after the other in a slot's device image
// (each on a 16-byte boundary), the batch's tables go up behind them, the kernels write the image, one DMA brings it to the
// slot's page-locked twin -- and while the device works on that, this thread moves the OTHER slot's batch from its page-locked
// buffer to where the caller wants it (memcpy: a mapped file's pages are written by the host alone).  A sink that does not fit
// what is left of a batch is cut at a multiple of 4 frames; a piece is a sink of its own, so the bytes are the same however
// the sinks are cut.  The bytes between two pieces of a slot are never copied out.
int fvad_egress(fvad_ctx* ctx, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                const uint64_t* sinks, size_t n_sinks, void* const* dst_host)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks && (!dst_host || !d_lanes)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress: NULL argument");
    if (n_sinks && !sinks) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress: NULL sinks");
    // the rules, with every sink's bytes at their absolute host address: two sinks of one file, or of overlapping buffers,
    // overlap there.  An address that wraps is saturated, which the range rule then refuses.
    std::vector<uint64_t> placed(sinks, sinks + n_sinks * FVAD_EGRESS_FIELDS);
    for (size_t i = 0; i < n_sinks; ++i) {
        uint64_t& at = placed[i * FVAD_EGRESS_FIELDS];
        const uint64_t base = (uint64_t)(uintptr_t)dst_host[i];
        at = at > UINT64_MAX - base ? UINT64_MAX : base + at;
    }
    const int bad = check_call(ctx, "fvad_egress", placed.data(), n_sinks, UINT64_MAX, src_format, d_lanes, n_lanes, lane_stride, n_samples);
    if (bad != FVAD_OK) return bad;
    for (size_t i = 0; i < n_sinks; ++i)
        if (!dst_host[i] && row(sinks, i).n_frames) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress: a sink with frames and no bytes");
    if (n_sinks == 0) return FVAD_OK;
    hipSetDevice(ctx->device);
    const size_t cap = (size_t)ctx->tune.ingest_ring_bytes;
    size_t table_room = 0;
    const int rc0 = ingest_ring_ensure(ctx, cap, &table_room);
    if (rc0 != FVAD_OK) return rc0;
    Workspace::IngestRing& ring = ctx->ws.ingest;
    const size_t o_tables = up16(cap);

    std::vector<Sink> batch;                              // the pieces of the batch being planned, byte_offset within the slot
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
        if (!build_tables(batch, lane_stride, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress: more than 2^24 tiles in one batch");
        if (t.blob.size() > table_room) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress: a batch's tables outgrew the ring"); // (kBatchSinks keeps them inside)
        // the slot is free: the batch it held was drained while the other slot's was in flight
        memcpy(ring.pin[slot] + o_tables, t.blob.data(), t.blob.size());
        FVAD_HIP(ctx, hipMemcpyAsync(ring.dev[slot] + o_tables, ring.pin[slot] + o_tables, t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
        const int rc = launch_tables(ctx, t, ring.dev[slot] + o_tables, d_lanes, src_format, lane_stride, ring.dev[slot]);
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
        for (size_t i = 0; i < n_sinks; ++i) {
            const Sink s = row(sinks, i);
            const uint64_t frame_bytes = s.n_channels * sample_bytes(s.format);
            uint64_t done = 0;
            while (done < s.n_frames) {
                size_t at = up16(used);
                uint64_t fit = at < cap ? (cap - at) / frame_bytes / 4 * 4 : 0; // frames that fit, cut at multiples of 4
                if ((fit == 0 && !batch.empty()) || batch.size() == kBatchSinks) {
                    const int rc = flush();
                    if (rc != FVAD_OK) return rc;
                    at = 0;
                    fit = cap / frame_bytes / 4 * 4; // >= 4: the ring holds at least 1 KB, a frame is at most 256 bytes
                }
                const uint64_t n = std::min<uint64_t>(s.n_frames - done, fit);
                Sink piece = s;
                piece.byte_offset = at;
                piece.n_frames = n;
                piece.src_offset = s.src_offset + done;
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
    return rc;
}

} // extern "C"
