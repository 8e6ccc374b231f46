// kernels_vad.hip -- the VAD state machines of a parameter sweep on the GPU: one lane per (stream, config) machine.
//
// host_vad.cpp's VadMachine::run (VADMachine.zig:138-239) with the same bits: f64 rolling averages summed in index order
// (RollingAverage.zig:45-56) and the long-term chain in the host's order, around the step both share (vad_machine.h: the lazily
// exact long-term bound, the four-state machine, the segment statistics and the margin audit).  The library is built with
// -ffp-contract=off.  What only depends on the stream -- the volume ratio of each frame -- comes from the host.
//
// Storage per machine.  Pushed samples are f32, so every ring holds f32 and the f64 term fl(data[i] * scalar) is recomputed
// inside the chain with the bits the host's cached product has (data[i] = (double)sample there).  The long-term ring also
// needs "slot still holds initial_long_term_avg": slot i holds a pushed value iff i < lt_filled (pushes fill it from slot 0).
// The long-term rings (8437 slots at the defaults) are in global memory, four slots of a machine side by side and those groups
// slot-major over the machines, so that a wavefront's load of four slots is one 1 KB run and the exact chain keeps 64 slots in
// flight; the short-term and channel-ratio rings (9 and 23 at the defaults) are in LDS when
// the workgroup's rings fit, else in global memory (one template, instantiated for either address space: the LDS form must
// not go through flat pointers, whose loads take a global load's latency).
//
// Lane mapping (one wavefront per workgroup, 64 machines): by stream, the lanes of a wavefront are configs of one stream (or of a
// few), so the per-frame ratio load is one address and every lane runs as many frames; by config, they are streams of one config,
// so every lane has the same ring lengths.  The work is latency-bound scalar f64 per lane; a wavefront runs the union of its
// lanes' exact long-term chains.
// Every loop is bounded by the machine's frame count or a ring length; no workgroup waits on another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "kernels.h"
#include "vad_avgs.h"
#include "vad_machine.h"

namespace {

using fvad::VadMachineCfg;

template <class P> // float* (global) or an LDS float pointer: the address space is known, so LDS slots are ds_read / ds_write
struct Ring { // a rolling average without initial value (RollingAverage.zig:11-56) over f32 slots base[i * stride]
    P base;
    long stride;
    uint32_t len, w, wc;
    double scalar, pref;

    // RollingAverage.push: before the ring is full the chain over the written slots with 1 / written_count; once full
    // host_vad.cpp's prefix form (the chain resumed from the sum below the write index: the same additions in the same order)
    __device__ double push(float x)
    {
        base[(long)w * stride] = x;
        if (wc == len) {
            double acc = (w == 0) ? 0.0 : pref;
            acc += (double)x * scalar;
            const double new_pref = acc;
#pragma unroll 8
            for (uint32_t i = w + 1; i < len; ++i) acc += (double)base[(long)i * stride] * scalar;
            w = (w + 1 == len) ? 0 : w + 1;
            pref = (w == 0) ? 0.0 : new_pref;
            return acc;
        }
        w = (w + 1 == len) ? 0 : w + 1;
        wc += 1;
        const double sc = 1.0 / (double)wc;
        double acc = 0.0;
#pragma unroll 8
        for (uint32_t i = 0; i < wc; ++i) acc += (double)base[(long)i * stride] * sc;
        if (wc == len) pref = 0.0; // steady from here on (the write index is back at 0)
        return acc;
    }
};

template <class P>
struct Machine : fvad::VadMachineState { // the step (decide, finish_step) and the long-term bound are vad_machine.h's
    VadMachineCfg cf; // in registers: read through a pointer, every field would be loaded again after each ring store (may alias)
    // long-term ring (host_vad.cpp: long_term_push, long_term_exact).  Slot i of this machine at lt[(i / 4) * lt_stride + i % 4]:
    // four consecutive slots are one 16-byte load of the lane.
    float* lt;
    long lt_stride;
    float lt_next = 0; // slot lt_w, loaded one push ahead (the next lazy push overwrites it and needs its old value at once)
    uint32_t lt_w = 0, lt_wc = 0, lt_filled = 0;
    bool lt_steady = false;
    Ring<P> st, cr;

    __device__ float& slot(uint32_t i) const { return lt[(long)(i >> 2) * lt_stride + (i & 3)]; }
    __device__ double lt_q(uint32_t i, float x) const { return i < lt_filled ? (double)x * cf.lt_scalar : cf.lt_q_init; }

    // The reference's chain over the whole ring.  The chain's adds depend on each other, its loads do not: blocks of kLtBlock
    // slots are loaded (16 bytes per lane and instruction) one block ahead of the adds, so that 2 kLtBlock slots are in flight
    // (the ring is allocated in whole blocks plus one: the loads past long_len stay inside it, their terms are not added)
    static constexpr int kLtBlock = 64;
    __device__ void load_block(uint32_t i0, float4 (&x)[kLtBlock / 4]) const
    {
#pragma unroll
        for (int g = 0; g < kLtBlock / 4; ++g) x[g] = *reinterpret_cast<const float4*>(lt + (long)((i0 >> 2) + g) * lt_stride);
    }
    __device__ __forceinline__ void lt_exact() // (inlined at each call: a call would put the machine on the stack)
    {
        double acc = 0.0, abs_sum = 0.0;
        const uint32_t n = cf.long_len;
        float4 cur[kLtBlock / 4], nxt[kLtBlock / 4];
        load_block(0, cur);
        for (uint32_t i0 = 0; i0 < n; i0 += kLtBlock) {
            load_block(i0 + kLtBlock, nxt); // (unconditional: a branch here would make the adds below wait for these loads too)
#pragma unroll
            for (int j = 0; j < kLtBlock; ++j) {
                const float4 v = cur[j / 4];
                const float x = (j & 3) == 0 ? v.x : (j & 3) == 1 ? v.y : (j & 3) == 2 ? v.z : v.w;
                const uint32_t i = i0 + (uint32_t)j;
                const double q = lt_q(i, x);
                acc = i < n ? acc + q : acc; // (a skipped term: the chain as if it were not there)
                abs_sum = i < n ? abs_sum + fabs(q) : abs_sum;
            }
#pragma unroll
            for (int g = 0; g < kLtBlock / 4; ++g) cur[g] = nxt[g];
        }
        anchor(acc, abs_sum);
    }

    __device__ void lt_push(float mv)
    {
        const uint32_t len = cf.long_len;
        if (!lt_steady) { // ring not full yet: RollingAverage.push as the reference runs it
            slot(lt_w) = mv;
            lt_w = (lt_w + 1 == len) ? 0 : lt_w + 1;
            lt_wc += 1;
            lt_filled = lt_wc;
            const double sc = 1.0 / (double)lt_wc;
            double acc = 0.0;
#pragma unroll 8
            for (uint32_t i = 0; i < lt_wc; ++i) acc += (double)slot(i) * sc;
            lt_last = acc;
            has_last = true;
            if (lt_wc == len) { lt_steady = true; lt_next = slot(0); lt_exact(); }
            return;
        }
        if (!lt_anchored) lt_exact();
        const uint32_t w = lt_w;
        const double qn = (double)mv * cf.lt_scalar, qo = lt_q(w, lt_next);
        slot(w) = mv;
        if (lt_filled < len) lt_filled += 1; // (only with an initial value: slot w == lt_filled is the one written now)
        lt_w = (w + 1 == len) ? 0 : w + 1;
        lt_next = slot(lt_w); // (w + 1 == len == 1: the slot just written, read back after the store)
        if (lazy_update(qn, qo)) lt_exact();
    }

    // lt_push for the cooperative form (vad_machines_coop_kernel): the same steps, but where lt_push runs lt_exact the wavefront
    // runs the chain together.  The caller has run it before this call if the ring was steady and not anchored; true: the
    // chain is due after this push (the ring became full, or lazy_update asked for a new anchor)
    __device__ bool lt_push_flag(float mv)
    {
        const uint32_t len = cf.long_len;
        if (!lt_steady) {
            slot(lt_w) = mv;
            lt_w = (lt_w + 1 == len) ? 0 : lt_w + 1;
            lt_wc += 1;
            lt_filled = lt_wc;
            const double sc = 1.0 / (double)lt_wc;
            double acc = 0.0;
#pragma unroll 8
            for (uint32_t i = 0; i < lt_wc; ++i) acc += (double)slot(i) * sc;
            lt_last = acc;
            has_last = true;
            if (lt_wc == len) { lt_steady = true; lt_next = slot(0); return true; }
            return false;
        }
        const uint32_t w = lt_w;
        const double qn = (double)mv * cf.lt_scalar, qo = lt_q(w, lt_next);
        slot(w) = mv;
        if (lt_filled < len) lt_filled += 1;
        lt_w = (w + 1 == len) ? 0 : w + 1;
        lt_next = slot(lt_w);
        return lazy_update(qn, qo);
    }
};

// the step's state field by field (a copy of the whole struct takes it through the stack or LDS)
__device__ __forceinline__ void copy_state(fvad::VadMachineState& d, const fvad::VadMachineState& s)
{
    d.state = s.state;
    d.speech_start = s.speech_start;
    d.speech_end = s.speech_end;
    d.ratio_sum = s.ratio_sum;
    d.ratio_count = s.ratio_count;
    d.met_cum = s.met_cum;
    d.audit.min_rel_threshold_margin = s.audit.min_rel_threshold_margin;
    d.audit.min_abs_ratio_margin = s.audit.min_abs_ratio_margin;
    d.audit.n_frames = s.audit.n_frames;
    d.lt_last = s.lt_last;
    d.has_last = s.has_last;
    d.lt_approx = s.lt_approx;
    d.lt_err = s.lt_err;
    d.lt_abs = s.lt_abs;
    d.lt_abs_anchor = s.lt_abs_anchor;
    d.lt_stale = s.lt_stale;
    d.lt_anchored = s.lt_anchored;
    d.lt_updates = s.lt_updates;
    d.exact_evals = s.exact_evals;
    d.lazy_pushes = s.lazy_pushes;
}

} // namespace

typedef __attribute__((address_space(3))) float lds_float;

// RINGS_LDS: the short-term and channel-ratio rings in LDS ([st_max + cr_max][64]), else in global memory.
// RESUME: the machine lives on between launches (a.state, a.rings, a.lt_rings: fvad_vad_batch_run_device_part): it is loaded
// before the frame loop and stored after it, so that the loop itself is the one-shot form's
// SIZED: the machines run on frames of several sizes (a.sized): each lane takes its config's frame size, frame count and ratio
// row, and by stream a stream's lanes take their configs in a.lane_config's order; the frame loop is the other forms'
template <bool RINGS_LDS, bool RESUME, bool SIZED = false>
__global__ __launch_bounds__(64) void vad_machines_kernel(VadMachinesArgs a)
{
    extern __shared__ float vad_rings[];
    using P = typename std::conditional<RINGS_LDS, lds_float*, float*>::type;
    const int lane = threadIdx.x;
    const long m = (long)blockIdx.x * 64 + lane; // this lane's place: its rings
    if (m >= a.n_machines) return;
    // which machine the lane runs: by stream, lane m is machine m (the configs of a stream side by side); by config, the streams of
    // a config side by side (every lane of a wavefront has that config's ring lengths)
    long s;
    int c;
    if (a.by_config) { c = (int)(m / a.n_streams); s = m - (long)c * a.n_streams; }
    else {
        s = m / a.n_configs;
        c = (int)(m - s * a.n_configs);
        if constexpr (SIZED) { if (a.lane_config) c = a.lane_config[c]; }
    }
    const long id = s * a.n_configs + c; // machine index of the outputs
    const VadMachineCfg* cfg = a.cfgs + c;

    Machine<P> mc;
    mc.cf = *cfg;
    mc.lt = a.lt_rings + 4 * m;
    mc.lt_stride = 4 * a.n_machines;
    P rb;
    long rs;
    if constexpr (RINGS_LDS) { rb = (lds_float*)vad_rings + lane; rs = 64; }
    else { rb = a.rings + m; rs = a.n_machines; }
    mc.st = Ring<P>{rb, rs, cfg->short_len, 0, 0, cfg->st_scalar, 0.0};
    mc.cr = Ring<P>{rb + (long)a.st_max * rs, rs, cfg->ratio_len, 0, 0, cfg->cr_scalar, 0.0};
    // the machine's frame clock: its frame size and the part's first frame in its frames; its (size, stream) row of n_frames
    // and the frame ratios
    uint64_t F = a.fft_size, first_frame = a.first_frame;
    long row = s;
    if constexpr (SIZED) {
        const uint32_t g = a.size_of[c];
        F = a.sizes[g];
        first_frame = a.first_sample / F;
        row = (long)g * a.n_streams + s;
    }
    uint32_t n_segs = 0, seg_base = 0; // (seg_base: the machine's first segment in the buffer)
    long k0 = 0;                       // the part's first frame this launch runs
    if (RESUME && !a.fresh) {          // the machine where the previous launch left it
        const fvad::VadLaneState& ls = a.state[id];
        copy_state(mc, ls.m);
        mc.st.w = ls.st_w; mc.st.wc = ls.st_wc; mc.st.pref = ls.st_pref;
        mc.cr.w = ls.cr_w; mc.cr.wc = ls.cr_wc; mc.cr.pref = ls.cr_pref;
        mc.lt_w = ls.lt_w; mc.lt_wc = ls.lt_wc; mc.lt_filled = ls.lt_filled; mc.lt_steady = ls.lt_steady != 0;
        mc.lt_next = mc.slot(mc.lt_w);
        n_segs = ls.n_segs;
        seg_base = a.rebase ? n_segs : ls.seg_base;
        k0 = ls.next_frame > first_frame ? (long)(ls.next_frame - first_frame) : 0;
        if constexpr (RINGS_LDS) { // the rings' home between launches is a.rings, laid out as the global form has them
            for (uint32_t i = 0; i < cfg->short_len; ++i) rb[(long)i * 64] = a.rings[(long)i * a.n_machines + m];
            for (uint32_t i = 0; i < cfg->ratio_len; ++i)
                rb[(long)(a.st_max + i) * 64] = a.rings[(long)(a.st_max + i) * a.n_machines + m];
        }
    } else if (cfg->has_init) { // RollingAverage.init with an initial value (RollingAverage.zig:20-26): full, steady, its average evaluated
        double acc = 0.0;
        for (uint32_t i = 0; i < cfg->long_len; ++i) acc += cfg->lt_q_init;
        mc.lt_last = acc;
        mc.has_last = true;
        mc.lt_steady = true;
        mc.lt_wc = cfg->long_len;
        mc.lt_next = mc.slot(0);
    }

    const long nf = a.n_frames[row];
    const int C = a.n_channels;
    const float* band = a.band + ((long)cfg->band * a.n_lanes + s * C) * a.band_stride;
    const float* ratio = a.ratio + row * a.ratio_stride;
    fvad_speech_segment* seg = a.segs + id * (long)a.seg_cap;
    // the next frame's band values (up to kPre channels) and ratio are loaded while this frame runs; the minimum is taken when the
    // frame is run, so that the loads are waited for a frame later (more channels: loaded and reduced at once)
    constexpr int kPre = 4;
    float nv[kPre], nr = 0.0f;
    auto fetch = [&](long k) {
#pragma unroll
        for (int ch = 0; ch < kPre; ++ch) nv[ch] = ch < C ? band[(long)ch * a.band_stride + k] : 999.0f;
        nr = ratio[k];
    };
    auto min_vol = [&](long k) { // VADMachine.zig:153-158, channels in order
        float mn = 999;
#pragma unroll
        for (int ch = 0; ch < kPre; ++ch) if (ch < C && nv[ch] < mn) mn = nv[ch];
        for (int ch = kPre; ch < C; ++ch) {
            const float v = band[(long)ch * a.band_stride + k];
            if (v < mn) mn = v;
        }
        return mn;
    };
    long k_end = nf;
    if (nf > k0) fetch(k0);
    for (long k = k0; k < nf; ++k) {
        if (RESUME && n_segs - seg_base >= a.seg_cap) { k_end = k; *a.paused = 1; break; } // no room for a segment of this frame
        const float mv = min_vol(k), rt = nr;
        if (k + 1 < nf) fetch(k + 1);
        // every frame overlaps a chunk, so its metadata always has a ratio (BufferedFFT.zig:137-140): has_ratio is true, and a
        // NaN ratio (from NaN audio) goes into the ring as it is, as on the host
        const double st = mc.st.push(mv);
        const double cr = mc.cr.push(rt);
        const bool met = mc.decide(mc.cf, st, cr, [&] { mc.lt_exact(); });
        if (!met) mc.lt_push(mv);
        const uint64_t frame = RESUME ? first_frame + (uint64_t)k : (uint64_t)k;
        const uint64_t sample = SIZED ? a.first_sample + (uint64_t)k * F : frame * F;
        mc.finish_step(mc.cf, sample, met, true, rt, [&](const fvad_speech_segment& sg) {
            if (n_segs - seg_base < a.seg_cap) seg[n_segs - seg_base] = sg;
            ++n_segs; // counted past the capacity: the caller sees the overflow and runs again with room for all
        });
    }
    if (RESUME) {
        fvad::VadLaneState& ls = a.state[id];
        copy_state(ls.m, mc);
        ls.st_w = mc.st.w; ls.st_wc = mc.st.wc; ls.st_pref = mc.st.pref;
        ls.cr_w = mc.cr.w; ls.cr_wc = mc.cr.wc; ls.cr_pref = mc.cr.pref;
        ls.lt_w = mc.lt_w; ls.lt_wc = mc.lt_wc; ls.lt_filled = mc.lt_filled; ls.lt_steady = mc.lt_steady ? 1u : 0u;
        ls.n_segs = n_segs;
        ls.seg_base = seg_base;
        ls.next_frame = first_frame + (uint64_t)k_end;
        if constexpr (RINGS_LDS) {
            for (uint32_t i = 0; i < cfg->short_len; ++i) a.rings[(long)i * a.n_machines + m] = rb[(long)i * 64];
            for (uint32_t i = 0; i < cfg->ratio_len; ++i)
                a.rings[(long)(a.st_max + i) * a.n_machines + m] = rb[(long)(a.st_max + i) * 64];
        }
    }
    a.seg_count[id] = n_segs;
    a.audits[id] = mc.audit;
    a.stats[2 * id] = mc.exact_evals;
    a.stats[2 * id + 1] = mc.lazy_pushes;
}

// ------------------------------------------------------------------ the cooperative form (context option vad_chain "coop")
// The same machines with the same bits, but an exact long-term chain is run by the whole wavefront: in the lane form one lane's
// chain takes the other 63 lanes through its loop, each dragging its own ring along, and the chain waits for one memory round
// trip per 64 slots.  Here a lane that would call lt_exact raises a flag; the wavefront ballots the flags and, owner by owner
// in lane order, all 64 lanes load the owner's ring (lane j the float4 rows j, j + 64, ...), each lane turns its slots into
// the chain's f64 terms and puts them into an LDS tile in slot order, and the two add chains (the sum and the sum of absolute
// values) run over the tile in that order: the reference's additions, one after the other.  A tile is kCoopTile slots (four
// loads of 64 rows); the next tile's loads are in flight and the LDS tiles alternate while the current one is added.
//
// A frame has two places for the chain: before the frame's push into the long-term ring (decide's exact(), or a steady ring
// that was never anchored) and after it (the ring became full, or lazy_update asked for a new anchor); a machine takes at most
// one of them in a frame.  Control flow around both is wavefront-uniform: lanes without a machine, lanes whose stream has ended
// and lanes that paused for segment room stay in the frame loop as helpers.  RESUME is a run-time flag here (a.resume): the
// one-shot launch is the resume form with fresh machines and no state to load or store.
constexpr int kCoopTile = 1024;                                            // slots of an LDS tile: 256 float4 rows, 4 per lane
constexpr size_t kCoopLdsBytes = 2 * (size_t)kCoopTile * sizeof(double);   // two tiles of f64 terms, ahead of the short rings
typedef __attribute__((address_space(3))) double lds_double;

namespace {

__device__ __forceinline__ uint32_t lane_u32(uint32_t x, int o) { return (uint32_t)__builtin_amdgcn_readlane((int)x, o); }
__device__ __forceinline__ double lane_f64(double x, int o)
{
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    const uint64_t r = (uint64_t)lane_u32((uint32_t)u, o) | (uint64_t)lane_u32((uint32_t)(u >> 32), o) << 32;
    return __longlong_as_double((long long)r);
}

// The chain of Machine::lt_exact over the ring of the machine at place m_o (long_len n, lt_filled filled), by all 64 lanes:
// every lane returns the owner's acc and abs_sum.  `tiles` is the wavefront's 2 * kCoopTile doubles of LDS.
__device__ __forceinline__ void coop_chain(const float* lt_rings, long n_machines, long m_o, uint32_t n, uint32_t filled, double scalar,
                                           double q_init, lds_double* tiles, int lane, double* acc_out, double* abs_out)
{
    const float* base = lt_rings + 4 * m_o;
    const long stride = 4 * n_machines;
    const uint32_t rows = n ? (n + 3) / 4 : 1; // (a ring has at least one slot)
    constexpr int kU = kCoopTile / 256; // float4 rows of a tile per lane
    // (a row past the ring's last: that last row again, its terms are not added.  Nothing is read outside the ring, and no
    // branch stands between the loads and the adds, which would make the adds wait for the next tile's loads too)
    auto load_tile = [&](uint32_t t, float4 (&x)[kU]) {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const uint32_t r = t * (kCoopTile / 4) + (uint32_t)u * 64 + (uint32_t)lane;
            x[u] = *reinterpret_cast<const float4*>(base + (long)(r < rows ? r : rows - 1) * stride);
        }
    };
    double acc = 0.0, abs_sum = 0.0;
    float4 cur[kU], nxt[kU];
    load_tile(0, cur);
    const uint32_t n_tiles = (rows + kCoopTile / 4 - 1) / (kCoopTile / 4);
    for (uint32_t t = 0; t < n_tiles; ++t) {
        load_tile(t + 1, nxt); // (in flight while this tile is added)
        lds_double* q = tiles + (t & 1) * kCoopTile;
        // this lane's 4 kU slots as the chain's terms, at their places in slot order
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const uint32_t lr = (uint32_t)u * 64 + (uint32_t)lane; // row within the tile
            const uint32_t i = t * kCoopTile + 4 * lr;
            const float xs[4] = {cur[u].x, cur[u].y, cur[u].z, cur[u].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) q[4 * lr + e] = i + e < filled ? (double)xs[e] * scalar : q_init;
        }
        __syncthreads(); // (one wavefront: the tile's writes before its reads)
        const uint32_t cnt = n - t * kCoopTile < (uint32_t)kCoopTile ? n - t * kCoopTile : (uint32_t)kCoopTile;
        // the adds in slot order, 32 terms read at a time (every lane reads the same address: a broadcast)
        const uint32_t full = cnt & ~31u;
        for (uint32_t i = 0; i < full; i += 32) {
            double c[32];
#pragma unroll
            for (int j = 0; j < 32; ++j) c[j] = q[i + j];
#pragma unroll
            for (int j = 0; j < 32; ++j) { acc += c[j]; abs_sum += fabs(c[j]); }
        }
        for (uint32_t i = full; i < cnt; ++i) { const double d = q[i]; acc += d; abs_sum += fabs(d); }
#pragma unroll
        for (int u = 0; u < kU; ++u) cur[u] = nxt[u];
    }
    __syncthreads(); // (the next chain's first tile is written after this chain's last reads)
    *acc_out = acc;
    *abs_out = abs_sum;
}

} // namespace

// TABLE (context option vad_avgs "table", a.table): the frame's short-term and channel-ratio averages are loaded from the tables
// kernels_vadavgs.hip filled before the launch, and its min_volume from the row that kernel's input was, instead of pushing the
// two short rings: two f64 loads per frame in place of two chains over LDS.  The form has no short rings (RINGS_LDS is false).
// A launch that stores state writes into the rings' home and the cursors what the ring form's pushes of the same frames would
// have left (vad_avgs.h), so every later launch -- of either form, after a retain or not -- goes on from the same bits.
//
// EMIT (context option vad_trigger "shared", a.emit): the trigger alone.  The lane runs fetch, the pushes or table reads, decide,
// both chain sections and lt_push_flag as ever and, in place of finish_step, shifts threshold_met into a 64-bit word that it
// stores after its 64th frame (the last, partial word with its upper bits zero): VadMachinesArgs.bits, which the finishing kernel
// (kernels_vadfinish.hip) walks once per config of the key.  It closes no segment, so it never pauses for room.
template <bool RINGS_LDS, bool SIZED, bool TABLE = false, bool EMIT = false>
__global__ __launch_bounds__(64) void vad_machines_coop_kernel(VadMachinesArgs a)
{
    extern __shared__ double vad_coop_lds[]; // [2][kCoopTile] chain terms, then the short rings [st_max + cr_max][64] (RINGS_LDS)
    using P = typename std::conditional<RINGS_LDS, lds_float*, float*>::type;
    lds_double* tiles = (lds_double*)vad_coop_lds;
    const int lane = threadIdx.x;
    const long m_raw = (long)blockIdx.x * 64 + lane;
    const bool valid = m_raw < a.n_machines;
    const long m = valid ? m_raw : a.n_machines - 1; // (a lane without a machine: addresses of the last one, nothing run or stored)
    const bool RESUME = a.resume != 0;
    long s;
    int c;
    if (a.by_config) { c = (int)(m / a.n_streams); s = m - (long)c * a.n_streams; }
    else {
        s = m / a.n_configs;
        c = (int)(m - s * a.n_configs);
        if constexpr (SIZED) { if (a.lane_config) c = a.lane_config[c]; }
    }
    const long id = s * a.n_configs + c;
    const VadMachineCfg* cfg = a.cfgs + c;

    Machine<P> mc;
    mc.cf = *cfg;
    mc.lt = a.lt_rings + 4 * m;
    mc.lt_stride = 4 * a.n_machines;
    P rb;
    long rs;
    if constexpr (RINGS_LDS) { rb = (lds_float*)(vad_coop_lds + 2 * kCoopTile) + lane; rs = 64; }
    else { rb = a.rings + m; rs = a.n_machines; }
    mc.st = Ring<P>{rb, rs, cfg->short_len, 0, 0, cfg->st_scalar, 0.0};
    mc.cr = Ring<P>{rb + (long)a.st_max * rs, rs, cfg->ratio_len, 0, 0, cfg->cr_scalar, 0.0};
    uint64_t F = a.fft_size, first_frame = a.first_frame;
    long row = s;
    if constexpr (SIZED) {
        const uint32_t g = a.size_of[c];
        F = a.sizes[g];
        first_frame = a.first_sample / F;
        row = (long)g * a.n_streams + s;
    }
    uint32_t n_segs = 0, seg_base = 0;
    long k0 = 0;
    if (valid && RESUME && !a.fresh) {
        const fvad::VadLaneState& ls = a.state[id];
        copy_state(mc, ls.m);
        mc.st.w = ls.st_w; mc.st.wc = ls.st_wc; mc.st.pref = ls.st_pref;
        mc.cr.w = ls.cr_w; mc.cr.wc = ls.cr_wc; mc.cr.pref = ls.cr_pref;
        mc.lt_w = ls.lt_w; mc.lt_wc = ls.lt_wc; mc.lt_filled = ls.lt_filled; mc.lt_steady = ls.lt_steady != 0;
        mc.lt_next = mc.slot(mc.lt_w);
        n_segs = ls.n_segs;
        seg_base = a.rebase ? n_segs : ls.seg_base;
        k0 = ls.next_frame > first_frame ? (long)(ls.next_frame - first_frame) : 0;
        if constexpr (RINGS_LDS) {
            for (uint32_t i = 0; i < cfg->short_len; ++i) rb[(long)i * 64] = a.rings[(long)i * a.n_machines + m];
            for (uint32_t i = 0; i < cfg->ratio_len; ++i)
                rb[(long)(a.st_max + i) * 64] = a.rings[(long)(a.st_max + i) * a.n_machines + m];
        }
    } else if (valid && cfg->has_init) {
        double acc = 0.0;
        for (uint32_t i = 0; i < cfg->long_len; ++i) acc += cfg->lt_q_init;
        mc.lt_last = acc;
        mc.has_last = true;
        mc.lt_steady = true;
        mc.lt_wc = cfg->long_len;
        mc.lt_next = mc.slot(0);
    }

    const long nf = valid ? a.n_frames[row] : 0;
    const int C = a.n_channels;
    const float* band = a.band + ((long)cfg->band * a.n_lanes + s * C) * a.band_stride;
    const float* ratio = a.ratio + row * a.ratio_stride;
    fvad_speech_segment* seg = a.segs + id * (long)a.seg_cap;
    constexpr int kPre = 4;
    float nv[kPre], nr = 0.0f;
    // the table form's rows: min_volume of (band, stream), the two averages of (key, stream), their next frame's values
    const float* mv_row = nullptr;
    const double *st_row = nullptr, *cr_row = nullptr;
    long st_nk = 0, cr_nk = 0;
    float nmv = 0.0f;
    double nst = 0.0, ncr = 0.0;
    if constexpr (TABLE) {
        const VadAvgKey& ks = a.st_keys[a.st_key[c]];
        const VadAvgKey& kc = a.cr_keys[a.cr_key[c]];
        mv_row = a.minvol + ((long)cfg->band * a.n_streams + s) * a.minvol_stride;
        st_row = a.st_tab + ks.base + s * a.tab_frames[ks.size] * (long)ks.nk;
        cr_row = a.cr_tab + kc.base + s * a.tab_frames[kc.size] * (long)kc.nk;
        st_nk = ks.nk;
        cr_nk = kc.nk;
    }
    auto fetch = [&](long k) {
        if constexpr (TABLE) {
            nmv = mv_row[k];
            nr = ratio[k];
            nst = st_row[k * st_nk];
            ncr = cr_row[k * cr_nk];
            return;
        }
#pragma unroll
        for (int ch = 0; ch < kPre; ++ch) nv[ch] = ch < C ? band[(long)ch * a.band_stride + k] : 999.0f;
        nr = ratio[k];
    };
    auto min_vol = [&](long k) {
        float mn = 999;
#pragma unroll
        for (int ch = 0; ch < kPre; ++ch) if (ch < C && nv[ch] < mn) mn = nv[ch];
        for (int ch = kPre; ch < C; ++ch) {
            const float v = band[(long)ch * a.band_stride + k];
            if (v < mn) mn = v;
        }
        return mn;
    };
    // the flagged lanes' chains, owner by owner in lane order; each owner anchors on its own
    auto run_chains = [&](bool flag) {
        unsigned long long owners = __ballot(flag);
        if (owners == 0) return;
        // the lanes' ring stores of this and earlier frames before the other lanes' loads of those slots
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        while (owners) {
            const int o = __builtin_ctzll(owners);
            owners &= owners - 1;
            double acc, abs_sum;
            coop_chain(a.lt_rings, a.n_machines, (long)blockIdx.x * 64 + o, lane_u32(mc.cf.long_len, o), lane_u32(mc.lt_filled, o),
                       lane_f64(mc.cf.lt_scalar, o), lane_f64(mc.cf.lt_q_init, o), tiles, lane, &acc, &abs_sum);
            if (lane == o) mc.anchor(acc, abs_sum);
        }
    };
    long k_end = nf, k = k0;
    bool running = k < nf; // this lane still has frames to run (else it only helps)
    if (running) fetch(k);
    // EMIT: the word being filled and where this machine's words of the stream go (word w at bits_row[w * bits_nk])
    unsigned long long word = 0, *bits_row = nullptr;
    long bits_nk = 0;
    if constexpr (EMIT) {
        const VadTrigKey tk = a.trig_keys[c];
        bits_row = a.bits + tk.base + s * (long)tk.words * (long)tk.nk;
        bits_nk = (long)tk.nk;
    }
    while (__ballot(running) != 0) { // (at least one running lane moves a frame on in every pass: bounded by the frame counts)
        if (!EMIT && running && RESUME && n_segs - seg_base >= a.seg_cap) { k_end = k; *a.paused = 1; running = false; }
        float mv = 0.0f, rt = 0.0f;
        double st = 0.0, cr = 0.0;
        bool met = false, before = false, redo = false;
        if (running) {
            if constexpr (TABLE) {
                mv = nmv;
                rt = nr;
                st = nst;
                cr = ncr;
                if (k + 1 < nf) fetch(k + 1);
            } else {
                mv = min_vol(k);
                rt = nr;
                if (k + 1 < nf) fetch(k + 1);
                st = mc.st.push(mv);
                cr = mc.cr.push(rt);
            }
            // decide up to its exact(): if it asks for the chain, what it did to the audit with the stale average is undone
            // and it runs again after the chain (then with a current average: the path below its exact())
            const fvad_vad_audit au = mc.audit;
            met = mc.decide(mc.cf, st, cr, [&] { redo = true; });
            if (redo) mc.audit = au;
            before = redo || (!met && mc.lt_steady && !mc.lt_anchored);
        }
        run_chains(before);
        bool after = false;
        if (running) {
            if (redo) met = mc.decide(mc.cf, st, cr, [] {});
            if (!met) after = mc.lt_push_flag(mv);
        }
        run_chains(after);
        if (running) {
            if constexpr (EMIT) {
                word |= (unsigned long long)met << (k & 63);
                if ((k & 63) == 63) { bits_row[(k >> 6) * bits_nk] = word; word = 0; }
            } else {
                const uint64_t frame = first_frame + (uint64_t)k; // (one-shot: first_frame is 0)
                const uint64_t sample = SIZED ? a.first_sample + (uint64_t)k * F : frame * F;
                mc.finish_step(mc.cf, sample, met, true, rt, [&](const fvad_speech_segment& sg) {
                    if (n_segs - seg_base < a.seg_cap) seg[n_segs - seg_base] = sg;
                    ++n_segs;
                });
            }
            ++k;
            running = k < nf;
        }
    }
    if (!valid) return;
    if constexpr (EMIT) {
        if (nf > k0 && (nf & 63)) bits_row[(nf >> 6) * bits_nk] = word; // (the part's last word: the bits past nf are zero)
    }
    if constexpr (TABLE) {
        if (RESUME) { // the short rings as the ring form's pushes of frames [0, k_end) of the part would have left them
            const uint64_t done = first_frame + (uint64_t)k_end; // pushes since the stream's start
            auto settle = [&](Ring<P>& r, const float* row, long home_row) {
                float* home = a.rings + home_row * a.n_machines + m;
                const long len = (long)r.len;
                for (long j = k_end > len ? k_end - len : 0; j < k_end; ++j)
                    home[(long)((first_frame + (uint64_t)j) % r.len) * a.n_machines] = row[j];
                r.w = fvad::ring_w_after(done, r.len);
                r.wc = fvad::ring_wc_after(done, r.len);
                double acc = 0.0;
                if (r.wc == r.len)
                    for (uint32_t i = 0; i < r.w; ++i) acc += (double)home[(long)i * a.n_machines] * r.scalar;
                r.pref = acc;
            };
            settle(mc.st, mv_row, 0);
            settle(mc.cr, ratio, a.st_max);
        }
    }
    if (RESUME) {
        fvad::VadLaneState& ls = a.state[id];
        copy_state(ls.m, mc);
        ls.st_w = mc.st.w; ls.st_wc = mc.st.wc; ls.st_pref = mc.st.pref;
        ls.cr_w = mc.cr.w; ls.cr_wc = mc.cr.wc; ls.cr_pref = mc.cr.pref;
        ls.lt_w = mc.lt_w; ls.lt_wc = mc.lt_wc; ls.lt_filled = mc.lt_filled; ls.lt_steady = mc.lt_steady ? 1u : 0u;
        ls.n_segs = n_segs;
        ls.seg_base = seg_base;
        ls.next_frame = first_frame + (uint64_t)k_end;
        if constexpr (RINGS_LDS) {
            for (uint32_t i = 0; i < cfg->short_len; ++i) a.rings[(long)i * a.n_machines + m] = rb[(long)i * 64];
            for (uint32_t i = 0; i < cfg->ratio_len; ++i)
                a.rings[(long)(a.st_max + i) * a.n_machines + m] = rb[(long)(a.st_max + i) * 64];
        }
    }
    a.seg_count[id] = n_segs;
    a.audits[id] = mc.audit;
    a.stats[2 * id] = mc.exact_evals;
    a.stats[2 * id + 1] = mc.lazy_pushes;
}

int fvad_launch_vad_machines(const VadMachinesArgs& a, hipStream_t stream)
{
    if (a.n_machines <= 0) return (int)hipSuccess;
    if (a.coop && a.emit) { // the shared-trigger form's first stage: the same launches, the machines emit bits
        const bool lds_rings = !a.table && a.rings_in_lds;
        const size_t lds = kCoopLdsBytes + (lds_rings ? (size_t)(a.st_max + a.cr_max) * 64 * sizeof(float) : 0);
        const dim3 grid((unsigned)((a.n_machines + 63) / 64));
        if (a.table) {
            if (a.sized) hipLaunchKernelGGL((vad_machines_coop_kernel<false, true, true, true>), grid, dim3(64), lds, stream, a);
            else hipLaunchKernelGGL((vad_machines_coop_kernel<false, false, true, true>), grid, dim3(64), lds, stream, a);
        } else if (a.sized) {
            if (lds_rings) hipLaunchKernelGGL((vad_machines_coop_kernel<true, true, false, true>), grid, dim3(64), lds, stream, a);
            else hipLaunchKernelGGL((vad_machines_coop_kernel<false, true, false, true>), grid, dim3(64), lds, stream, a);
        } else if (lds_rings) hipLaunchKernelGGL((vad_machines_coop_kernel<true, false, false, true>), grid, dim3(64), lds, stream, a);
        else hipLaunchKernelGGL((vad_machines_coop_kernel<false, false, false, true>), grid, dim3(64), lds, stream, a);
        return (int)hipGetLastError();
    }
    if (a.emit) return (int)hipErrorInvalidValue; // (only the cooperative form emits)
    if (a.coop && a.table) { // the table form: the two chain tiles, no short rings
        const dim3 grid((unsigned)((a.n_machines + 63) / 64));
        if (a.sized) hipLaunchKernelGGL((vad_machines_coop_kernel<false, true, true>), grid, dim3(64), kCoopLdsBytes, stream, a);
        else hipLaunchKernelGGL((vad_machines_coop_kernel<false, false, true>), grid, dim3(64), kCoopLdsBytes, stream, a);
        return (int)hipGetLastError();
    }
    if (a.coop) { // the cooperative form: two chain tiles ahead of the short rings (at most 16 + 48 KB)
        const size_t lds = kCoopLdsBytes + (a.rings_in_lds ? (size_t)(a.st_max + a.cr_max) * 64 * sizeof(float) : 0);
        const dim3 grid((unsigned)((a.n_machines + 63) / 64));
        if (a.sized) {
            if (a.rings_in_lds) hipLaunchKernelGGL((vad_machines_coop_kernel<true, true>), grid, dim3(64), lds, stream, a);
            else hipLaunchKernelGGL((vad_machines_coop_kernel<false, true>), grid, dim3(64), lds, stream, a);
        } else if (a.rings_in_lds) hipLaunchKernelGGL((vad_machines_coop_kernel<true, false>), grid, dim3(64), lds, stream, a);
        else hipLaunchKernelGGL((vad_machines_coop_kernel<false, false>), grid, dim3(64), lds, stream, a);
        return (int)hipGetLastError();
    }
    const size_t lds = a.rings_in_lds ? (size_t)(a.st_max + a.cr_max) * 64 * sizeof(float) : 0;
    const dim3 grid((unsigned)((a.n_machines + 63) / 64));
    if (a.sized) {
        if (a.resume) {
            if (a.rings_in_lds) hipLaunchKernelGGL((vad_machines_kernel<true, true, true>), grid, dim3(64), lds, stream, a);
            else hipLaunchKernelGGL((vad_machines_kernel<false, true, true>), grid, dim3(64), 0, stream, a);
        } else if (a.rings_in_lds) hipLaunchKernelGGL((vad_machines_kernel<true, false, true>), grid, dim3(64), lds, stream, a);
        else hipLaunchKernelGGL((vad_machines_kernel<false, false, true>), grid, dim3(64), 0, stream, a);
    } else if (a.resume) {
        if (a.rings_in_lds) hipLaunchKernelGGL((vad_machines_kernel<true, true>), grid, dim3(64), lds, stream, a);
        else hipLaunchKernelGGL((vad_machines_kernel<false, true>), grid, dim3(64), 0, stream, a);
    } else if (a.rings_in_lds) hipLaunchKernelGGL((vad_machines_kernel<true, false>), grid, dim3(64), lds, stream, a);
    else hipLaunchKernelGGL((vad_machines_kernel<false, false>), grid, dim3(64), 0, stream, a);
    return (int)hipGetLastError();
}
