// engine_egress_resample.cpp -- fvad_egress_resample_device / fvad_egress_resample: planar 48 kHz device lanes resampled into
// the interleaved bytes of files at another rate with kernels_egress_resample.hip.  The argument rules are
// fvad_egress_resample_check's (host_egress_resample.cpp) and the tile is egress_resample.h's; here are the tables a launch
// searches and, for bytes in host memory, engine_egress.cpp's use of the shared two-slot page-locked ring
// (Workspace::IngestRing, sized by the context option ingest_ring_bytes; both calls return only when their last batch is done,
// so the ring is idle whenever any of its users starts).  ev[s] here means: slot s's bytes have arrived in its page-locked
// buffer.  The tap table goes up once per call.
// fvad_egress_resample_strided_device / fvad_egress_resample_strided are the same two calls over a stream that lies src_step
// apart in its lanes (kernels_egress_strided.hip; the rules are host_egress_strided.cpp's): the internals here take a step, 0
// for the plain entries, which go on launching kernels_egress_resample.hip's kernel as they did.
#include <algorithm>
#include <cstring>
#include <vector>

#include "egress_strided.h"
#include "internal.h"

using namespace fvad;

namespace {

static_assert(kEgressResampleTileBytes == (uint64_t)kIngestTileBytes && kEgressResampleWindow == (uint64_t)kClipTile, "egress_resample.h restates the kernel's tile");

struct Row { uint64_t byte_offset, n_out, n_channels, format, first_lane, src_offset, frame_base, n_frames, stream_frames, out_from; };
Row row(const uint64_t* sinks, size_t i)
{
    const uint64_t* r = sinks + i * FVAD_EGRESS_RESAMPLE_FIELDS;
    return {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9]};
}
size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// The tables of one call or batch: per file format (a launch encodes one) the jobs and their unit prefix, laid out in ONE blob
// whose parts start on 16-byte boundaries, so that one copy carries them to the device (engine_egress.cpp's layout).
struct Tables {
    struct Set { size_t o_jobs = 0, o_prefix = 0; uint32_t n_jobs = 0, n_units = 0; } set[3];
    std::vector<char> blob;
};

// as for the egress: a launch is one workgroup of 256 lanes per unit and takes fewer than 2^24 units
constexpr uint64_t kMaxUnits = (1ull << 24) - 1;

// false: more than kMaxUnits units in one launch
bool build_tables(const std::vector<Row>& rows, size_t lane_stride, const Ratio& q, uint32_t n_taps, Tables& t)
{
    t.blob.clear();
    for (int f = 0; f < 3; ++f) {
        std::vector<EgressResampleJob> jobs;
        std::vector<uint32_t> prefix;
        uint64_t units = 0;
        for (const Row& s : rows) {
            if ((int)s.format != f || s.n_out == 0) continue; // (a row without outputs writes nothing)
            EgressResampleJob j{};
            j.tile_out = (uint32_t)egress_resample_tile(q, n_taps, s.n_channels, s.format); // >= 4: the check refused 0
            j.dst_off = s.byte_offset;
            j.out_from = s.out_from;
            j.n_out = s.n_out;
            j.src_off = s.first_lane * (uint64_t)lane_stride + s.src_offset;
            j.frame_base = s.frame_base;
            j.stream_frames = s.stream_frames;
            const uint64_t nt = (s.n_out + j.tile_out - 1) / j.tile_out;
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
        set.o_prefix = set.o_jobs + up16(jobs.size() * sizeof(EgressResampleJob));
        t.blob.resize(set.o_prefix + up16(prefix.size() * 4));
        memcpy(t.blob.data() + set.o_jobs, jobs.data(), jobs.size() * sizeof(EgressResampleJob));
        memcpy(t.blob.data() + set.o_prefix, prefix.data(), prefix.size() * 4);
    }
    return true;
}

// the launches of one set of tables whose blob is at d_blob (queued on ctx->stream)
// step 0: the plain kernel over contiguous lanes; otherwise the strided kernel
int launch_tables(fvad_ctx* ctx, const Tables& t, const char* d_blob, const void* d_lanes, size_t lane_stride, const float* d_table,
                  const Ratio& q, uint32_t n_taps, uint32_t step, void* d_out)
{
    for (int f = 0; f < 3; ++f) {
        const Tables::Set& set = t.set[f];
        if (!set.n_units) continue;
        EgressResampleArgs a{};
        a.lanes = static_cast<const float*>(d_lanes);
        a.lane_stride = lane_stride;
        a.out = static_cast<uint8_t*>(d_out);
        a.jobs = reinterpret_cast<const EgressResampleJob*>(d_blob + set.o_jobs);
        a.unit_prefix = reinterpret_cast<const uint32_t*>(d_blob + set.o_prefix);
        a.table = d_table;
        a.n_jobs = set.n_jobs;
        a.n_units = set.n_units;
        a.up = q.up;
        a.down = q.down;
        a.n_taps = n_taps;
        a.file_format = f;
        time_begin(ctx, step ? "egress_strided" : "egress_resample");
        FVAD_HIP(ctx, (hipError_t)(step ? fvad_launch_egress_strided(EgressStridedArgs{a, step}, ctx->stream) : fvad_launch_egress_resample(a, ctx->stream)));
        time_end(ctx);
    }
    return FVAD_OK;
}

int check_call(const fvad_ctx* ctx, const char* who, const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, uint32_t up, uint32_t down,
               const float* taps, uint32_t n_taps, bool strided, uint32_t step, int src_format, const void* d_lanes, size_t n_lanes, size_t lane_stride,
               size_t n_samples)
{
    const int rc = strided ? fvad_egress_resample_strided_check(sinks, n_sinks, out_bytes, up, down, taps, n_taps, step, src_format, n_lanes, lane_stride, n_samples)
                           : fvad_egress_resample_check(sinks, n_sinks, out_bytes, up, down, taps, n_taps, src_format, n_lanes, lane_stride, n_samples);
    if (rc != FVAD_OK) return set_err(ctx, rc, std::string(who) + (rc == FVAD_ERR_OUT_OF_RANGE ? ": a row's lanes, samples or bytes are out of range"
                                                                                                 : strided ? ": a bad argument, ratio, step, tap or row (fvad_egress_resample_strided_check)"
                                                                                                           : ": a bad argument, ratio, tap or row (fvad_egress_resample_check)"));
    if ((uintptr_t)d_lanes % 4 != 0) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, std::string(who) + ": the lanes are not aligned to their samples");
    return FVAD_OK;
}

// the pieces a batch of fvad_egress_resample holds at most: the ring's table room is sized for 4096 IngestJobs in three sets
constexpr size_t kBatchRows = 2048;
static_assert(kBatchRows * sizeof(EgressResampleJob) <= 4096 * sizeof(IngestJob), "the ring's table room");

// the device form of both entries (strided: `step` is the caller's, checked below; otherwise 0)
int device_call(fvad_ctx* ctx, const std::string& who, bool strided, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride,
                size_t n_samples, const uint64_t* sinks, size_t n_sinks, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps, uint32_t step,
                void* d_out, uint64_t out_bytes)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks && (!d_lanes || !d_out)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": NULL argument");
    const int bad = check_call(ctx, who.c_str(), sinks, n_sinks, out_bytes, up, down, taps, n_taps, strided, step, src_format, d_lanes, n_lanes, lane_stride, n_samples);
    if (bad != FVAD_OK) return bad;
    if (n_sinks == 0) return FVAD_OK;
    const Ratio q{up, down};
    std::vector<Row> all(n_sinks);
    for (size_t i = 0; i < n_sinks; ++i) all[i] = row(sinks, i);
    Tables t;
    if (!build_tables(all, lane_stride, q, n_taps, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": more than 2^24 tiles in one call: write in batches");
    if (t.blob.empty()) return FVAD_OK; // nothing to write
    const std::vector<float> table = resample_table(Taps{taps, n_taps}, q);
    const size_t o_blob = up16(table.size() * 4);
    hipSetDevice(ctx->device);
    char* d = nullptr; // the tap table, then the row tables
    if (hipMalloc((void**)&d, o_blob + t.blob.size()) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, who + ": hipMalloc of the tables failed"); }
    auto run = [&]() -> int {
        FVAD_HIP(ctx, hipMemcpyAsync(d, table.data(), table.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_blob, t.blob.data(), t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
        const int rc = launch_tables(ctx, t, d + o_blob, d_lanes, lane_stride, reinterpret_cast<const float*>(d), q, n_taps, step, d_out);
        if (rc != FVAD_OK) return rc;
        FVAD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FVAD_OK;
    };
    const int rc = run();
    if (rc != FVAD_OK) (void)hipStreamSynchronize(ctx->stream);
    hipFree(d);
    return rc;
}

// fvad_egress's batches of at most ring_bytes output bytes, cut in OUTPUT frames: a row that does not fit what is left of a
// batch is cut at a multiple of 4 output frames, and a piece is the row with out_from advanced and the SAME given frames -- they
// cover the row's window, so they cover the piece's, and the lanes are on the device already: nothing of the window is copied
// and the bytes cannot depend on the cut.  While the device fills one slot, this thread moves the other slot's batch from its
// page-locked buffer to where the caller wants it.
int host_call(fvad_ctx* ctx, const std::string& who, bool strided, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride,
              size_t n_samples, const uint64_t* sinks, size_t n_sinks, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps, uint32_t step,
              void* const* dst_host)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks && (!dst_host || !d_lanes)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": NULL argument");
    if (n_sinks && !sinks) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": NULL sinks");
    // the rules, with every row's bytes at their absolute host address (fvad_egress's way: an address that wraps is saturated,
    // which the range rule then refuses)
    std::vector<uint64_t> placed(sinks, sinks + n_sinks * FVAD_EGRESS_RESAMPLE_FIELDS);
    for (size_t i = 0; i < n_sinks; ++i) {
        uint64_t& at = placed[i * FVAD_EGRESS_RESAMPLE_FIELDS];
        const uint64_t base = (uint64_t)(uintptr_t)dst_host[i];
        at = at > UINT64_MAX - base ? UINT64_MAX : base + at;
    }
    const int bad = check_call(ctx, who.c_str(), placed.data(), n_sinks, UINT64_MAX, up, down, taps, n_taps, strided, step, src_format, d_lanes, n_lanes, lane_stride, n_samples);
    if (bad != FVAD_OK) return bad;
    for (size_t i = 0; i < n_sinks; ++i)
        if (!dst_host[i] && row(sinks, i).n_out) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": a row with outputs and no bytes");
    if (n_sinks == 0) return FVAD_OK;
    const Ratio q{up, down};
    hipSetDevice(ctx->device);
    const size_t cap = (size_t)ctx->tune.ingest_ring_bytes;
    size_t table_room = 0;
    const int rc0 = ingest_ring_ensure(ctx, cap, &table_room);
    if (rc0 != FVAD_OK) return rc0;
    Workspace::IngestRing& ring = ctx->ws.ingest;
    const size_t o_tables = up16(cap);
    const std::vector<float> table = resample_table(Taps{taps, n_taps}, q);
    float* d_table = nullptr;
    if (hipMalloc((void**)&d_table, table.size() * 4) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, who + ": hipMalloc of the tap table failed"); }

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
        if (!build_tables(batch, lane_stride, q, n_taps, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": more than 2^24 tiles in one batch");
        if (t.blob.size() > table_room) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": a batch's tables outgrew the ring"); // (kBatchRows keeps them inside)
        // the slot is free: the batch it held was drained while the other slot's was in flight
        memcpy(ring.pin[slot] + o_tables, t.blob.data(), t.blob.size());
        FVAD_HIP(ctx, hipMemcpyAsync(ring.dev[slot] + o_tables, ring.pin[slot] + o_tables, t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
        const int rc = launch_tables(ctx, t, ring.dev[slot] + o_tables, d_lanes, lane_stride, d_table, q, n_taps, step, ring.dev[slot]);
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
        FVAD_HIP(ctx, hipMemcpyAsync(d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        for (size_t i = 0; i < n_sinks; ++i) {
            const Row s = row(sinks, i);
            const uint64_t frame_bytes = s.n_channels * sample_bytes_of(s.format);
            uint64_t done = 0;
            while (done < s.n_out) {
                size_t at = up16(used);
                uint64_t fit = at < cap ? (cap - at) / frame_bytes / 4 * 4 : 0; // output frames that fit, cut at multiples of 4
                if ((fit == 0 && !batch.empty()) || batch.size() == kBatchRows) {
                    const int rc = flush();
                    if (rc != FVAD_OK) return rc;
                    at = 0;
                    fit = cap / frame_bytes / 4 * 4; // >= 4: the ring holds at least 1 KB, a frame is at most 256 bytes
                }
                const uint64_t n = std::min<uint64_t>(s.n_out - done, fit);
                Row piece = s;
                piece.byte_offset = at;
                piece.n_out = n;
                piece.out_from = s.out_from + done;
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
    hipFree(d_table);
    return rc;
}

} // namespace

extern "C" {

int fvad_egress_resample_device(fvad_ctx* ctx, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                const uint64_t* sinks, size_t n_sinks, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps,
                                void* d_out, uint64_t out_bytes)
{
    return device_call(ctx, "fvad_egress_resample_device", false, d_lanes, src_format, n_lanes, lane_stride, n_samples, sinks, n_sinks, up, down, taps, n_taps, 0, d_out, out_bytes);
}

int fvad_egress_resample(fvad_ctx* ctx, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                         const uint64_t* sinks, size_t n_sinks, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps,
                         void* const* dst_host)
{
    return host_call(ctx, "fvad_egress_resample", false, d_lanes, src_format, n_lanes, lane_stride, n_samples, sinks, n_sinks, up, down, taps, n_taps, 0, dst_host);
}

int fvad_egress_resample_strided_device(fvad_ctx* ctx, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                        const uint64_t* sinks, size_t n_sinks, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps,
                                        uint32_t src_step, void* d_out, uint64_t out_bytes)
{
    return device_call(ctx, "fvad_egress_resample_strided_device", true, d_lanes, src_format, n_lanes, lane_stride, n_samples, sinks, n_sinks, up, down, taps, n_taps, src_step, d_out, out_bytes);
}

int fvad_egress_resample_strided(fvad_ctx* ctx, const void* d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                                 const uint64_t* sinks, size_t n_sinks, uint32_t up, uint32_t down, const float* taps, uint32_t n_taps,
                                 uint32_t src_step, void* const* dst_host)
{
    return host_call(ctx, "fvad_egress_resample_strided", true, d_lanes, src_format, n_lanes, lane_stride, n_samples, sinks, n_sinks, up, down, taps, n_taps, src_step, dst_host);
}

} // extern "C"
