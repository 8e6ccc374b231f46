// engine_egress_mix.cpp -- fvad_egress_mix_device / fvad_egress_mix: two sets of planar f32 device lanes, weighted and summed,
// into the interleaved bytes of files' data chunks with kernels_egress_mix.hip.  engine_egress.cpp's two forms: the argument
// rules are fvad_egress_mix_check's (host_egress_mix.cpp); here are the tables a launch searches and, for bytes in host memory,
// the batches through the two-slot page-locked ring fvad_ingest and fvad_egress use (Workspace::IngestRing, shared: every one
// of these calls returns only when its last batch is done, so the ring is idle whenever one starts).
#include <algorithm>
#include <cstring>
#include <vector>

#include "egress_mix.h"
#include "internal.h"

using namespace fvad;

namespace {

struct Sink { uint64_t byte_offset, n_frames, n_channels, format, first_lane, src_offset, orig_offset, orig_zeros; };
Sink row(const uint64_t* sinks, size_t i)
{
    const uint64_t* r = sinks + i * FVAD_EGRESS_MIX_FIELDS;
    return {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
}
uint64_t sample_bytes(uint64_t format) { return format == FVAD_INGEST_PCM16 ? 2 : format == FVAD_INGEST_PCM24 ? 3 : 4; }
size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// the two lane sets and the weights of a call
struct Lanes {
    const void *d_orig, *d_den;
    size_t orig_stride, orig_samples, den_stride, den_samples, n_lanes;
    float w_orig, w_den;
};

// The tables of one call or batch: per file format (a launch encodes one) the jobs and their unit prefix, laid out in ONE blob
// whose parts start on 16-byte boundaries, so that one copy carries them to the device (engine_egress.cpp's layout).
struct Tables {
    struct Set { size_t o_jobs = 0, o_prefix = 0; uint32_t n_jobs = 0, n_units = 0; } set[3];
    std::vector<char> blob;
};

// as for the egress: a launch is one workgroup of 256 lanes per unit and takes fewer than 2^24 units
constexpr uint64_t kMaxUnits = (1ull << 24) - 1;

// false: more than kMaxUnits units in one launch
bool build_tables(const std::vector<Sink>& sinks, const Lanes& l, Tables& t)
{
    t.blob.clear();
    for (int f = 0; f < 3; ++f) {
        std::vector<EgressMixJob> jobs;
        std::vector<uint32_t> prefix;
        uint64_t units = 0;
        for (const Sink& s : sinks) {
            if ((int)s.format != f || s.n_frames == 0) continue; // (a sink without frames writes nothing)
            EgressMixJob j{};
            const uint64_t frame_bytes = s.n_channels * sample_bytes(s.format);
            j.tile_frames = (uint32_t)(kIngestTileBytes / frame_bytes / 4 * 4); // >= 64: a frame is at most 256 bytes
            j.dst_off = s.byte_offset;
            j.n_frames = s.n_frames;
            // (the offsets of a source whose weight is zero are not checked and not used: they may wrap)
            j.den_off = s.first_lane * (uint64_t)l.den_stride + s.src_offset;
            j.orig_off = s.first_lane * (uint64_t)l.orig_stride + s.orig_offset;
            j.orig_zeros = s.orig_zeros;
            j.n_channels = (uint32_t)s.n_channels;
            const uint64_t nt = (s.n_frames + j.tile_frames - 1) / j.tile_frames;
            if (nt > kMaxUnits) return false;
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
        set.o_prefix = set.o_jobs + up16(jobs.size() * sizeof(EgressMixJob));
        t.blob.resize(set.o_prefix + up16(prefix.size() * 4));
        memcpy(t.blob.data() + set.o_jobs, jobs.data(), jobs.size() * sizeof(EgressMixJob));
        memcpy(t.blob.data() + set.o_prefix, prefix.data(), prefix.size() * 4);
    }
    return true;
}

// the launches of one set of tables whose blob is at d_blob (queued on ctx->stream)
int launch_tables(fvad_ctx* ctx, const Tables& t, const char* d_blob, const Lanes& l, void* d_out)
{
    for (int f = 0; f < 3; ++f) {
        const Tables::Set& set = t.set[f];
        if (!set.n_units) continue;
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
    }
    return FVAD_OK;
}

// the check, then what it cannot see: the lanes of a source whose weight is not zero are there and aligned to their samples
int check_call(const fvad_ctx* ctx, const char* who, const uint64_t* sinks, size_t n_sinks, uint64_t out_bytes, int src_format, const Lanes& l)
{
    const int rc = fvad_egress_mix_check(sinks, n_sinks, out_bytes, src_format, l.w_orig, l.w_den, l.n_lanes, l.orig_stride, l.orig_samples,
                                         l.den_stride, l.den_samples);
    if (rc != FVAD_OK) return set_err(ctx, rc, std::string(who) + (rc == FVAD_ERR_OUT_OF_RANGE ? ": a sink's lanes, samples or bytes are out of range"
                                                                                                 : ": a bad argument or sink (fvad_egress_mix_check)"));
    if (n_sinks && ((l.w_orig != 0.0f && !l.d_orig) || (l.w_den != 0.0f && !l.d_den)))
        return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL lanes with a weight that is not zero");
    if ((l.w_orig != 0.0f && (uintptr_t)l.d_orig % 4 != 0) || (l.w_den != 0.0f && (uintptr_t)l.d_den % 4 != 0))
        return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, std::string(who) + ": the lanes are not aligned to their samples");
    return FVAD_OK;
}

// the pieces a batch of fvad_egress_mix holds at most: the ring's table room is sized for as many IngestJobs in three sets
constexpr size_t kBatchSinks = 4096;
static_assert(sizeof(EgressMixJob) <= sizeof(IngestJob), "the ring's table room");

} // namespace

extern "C" {

int fvad_egress_mix_device(fvad_ctx* ctx, const void* d_orig, size_t orig_stride, size_t orig_samples, const void* d_den, size_t den_stride,
                           size_t den_samples, int src_format, size_t n_lanes, float w_orig, float w_den, const uint64_t* sinks, size_t n_sinks,
                           void* d_out, uint64_t out_bytes)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks && !d_out) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_mix_device: NULL argument");
    const Lanes l{d_orig, d_den, orig_stride, orig_samples, den_stride, den_samples, n_lanes, w_orig, w_den};
    const int bad = check_call(ctx, "fvad_egress_mix_device", sinks, n_sinks, out_bytes, src_format, l);
    if (bad != FVAD_OK) return bad;
    if (n_sinks == 0) return FVAD_OK;
    std::vector<Sink> all(n_sinks);
    for (size_t i = 0; i < n_sinks; ++i) all[i] = row(sinks, i);
    Tables t;
    if (!build_tables(all, l, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_mix_device: more than 2^24 tiles in one call: write in batches");
    if (t.blob.empty()) return FVAD_OK; // nothing to write
    hipSetDevice(ctx->device);
    char* d = nullptr;
    if (hipMalloc((void**)&d, t.blob.size()) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, "fvad_egress_mix_device: hipMalloc of the sink tables failed"); }
    auto run = [&]() -> int {
        FVAD_HIP(ctx, hipMemcpyAsync(d, t.blob.data(), t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
        const int rc = launch_tables(ctx, t, d, l, d_out);
        if (rc != FVAD_OK) return rc;
        FVAD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FVAD_OK;
    };
    const int rc = run();
    if (rc != FVAD_OK) (void)hipStreamSynchronize(ctx->stream);
    hipFree(d);
    return rc;
}

// fvad_egress's batches (engine_egress.cpp): the sinks' pieces one after the other in a slot's device image, each on a 16-byte
// boundary, the batch's tables behind them; one DMA per batch, and while the device fills one slot this thread moves the other
// slot's bytes to where the caller wants them.  A sink that does not fit what is left of a batch is cut at a multiple of 4
// frames; the piece from frame `done` on is the sink with src_offset advanced by done, orig_zeros lowered by min(orig_zeros,
// done) and orig_offset advanced by the rest of done -- the same pairing, so the bytes are the same however the sinks are cut.
int fvad_egress_mix(fvad_ctx* ctx, const void* d_orig, size_t orig_stride, size_t orig_samples, const void* d_den, size_t den_stride,
                    size_t den_samples, int src_format, size_t n_lanes, float w_orig, float w_den, const uint64_t* sinks, size_t n_sinks,
                    void* const* dst_host)
{
    if (!ctx) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_sinks && !dst_host) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_mix: NULL argument");
    if (n_sinks && !sinks) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_mix: NULL sinks");
    // the rules, with every sink's bytes at their absolute host address (an address that wraps is saturated: the range rule refuses it)
    std::vector<uint64_t> placed(sinks, sinks + n_sinks * FVAD_EGRESS_MIX_FIELDS);
    for (size_t i = 0; i < n_sinks; ++i) {
        uint64_t& at = placed[i * FVAD_EGRESS_MIX_FIELDS];
        const uint64_t base = (uint64_t)(uintptr_t)dst_host[i];
        at = at > UINT64_MAX - base ? UINT64_MAX : base + at;
    }
    const Lanes l{d_orig, d_den, orig_stride, orig_samples, den_stride, den_samples, n_lanes, w_orig, w_den};
    const int bad = check_call(ctx, "fvad_egress_mix", placed.data(), n_sinks, UINT64_MAX, src_format, l);
    if (bad != FVAD_OK) return bad;
    for (size_t i = 0; i < n_sinks; ++i)
        if (!dst_host[i] && row(sinks, i).n_frames) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_mix: a sink with frames and no bytes");
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
        if (!build_tables(batch, l, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_mix: more than 2^24 tiles in one batch");
        if (t.blob.size() > table_room) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, "fvad_egress_mix: a batch's tables outgrew the ring"); // (kBatchSinks keeps them inside)
        // the slot is free: the batch it held was drained while the other slot's was in flight
        memcpy(ring.pin[slot] + o_tables, t.blob.data(), t.blob.size());
        FVAD_HIP(ctx, hipMemcpyAsync(ring.dev[slot] + o_tables, ring.pin[slot] + o_tables, t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
        const int rc = launch_tables(ctx, t, ring.dev[slot] + o_tables, l, ring.dev[slot]);
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
                const uint64_t zeros_done = std::min(s.orig_zeros, done);
                Sink piece = s;
                piece.byte_offset = at;
                piece.n_frames = n;
                piece.src_offset = s.src_offset + done;
                piece.orig_zeros = s.orig_zeros - zeros_done;
                piece.orig_offset = s.orig_offset + (done - zeros_done);
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
