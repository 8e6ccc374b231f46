"""The cooperative form of the device VAD machines (context option vad_chain "coop": a wavefront runs an exact long-term chain
together, kernels_vad.hip) against the lane form, bit for bit -- segments, audits, lazy statistics and scores of every machine --
and against the CPU oracle's machines directly, on the smallest shapes at which the cooperative section can go wrong
(vad_chain_cases.py).  Every case checks from lazy_stats that its machines really ran exact chains on a full ring."""
import numpy as np
import pytest

import vad_chain_cases as K
import vad_oracle_cases as V

pytestmark = pytest.mark.gpu

STAT = V.STAT_CFGS[1]


def labels(seconds):
    return [[(1.0, 2.5), (4.0, 7.0), (float(int(s) - 6), float(int(s) - 2))] for s in seconds]


def upload(ctx, arr):
    d = ctx.device_alloc(arr.nbytes)
    ctx.to_device(d, arr)
    return d


def blocks(sw, I, sizes=None):
    """the band blocks as sw.bands() orders them: [n_bands][streams][stride] (every config reads the default speech band)"""
    bands, _ = sw.bands()
    if sizes is None:
        assert len(bands) == 1
        return np.ascontiguousarray(I["band"][None])
    stride = max(I[F]["band"].shape[1] for F in sw.sizes)
    out = np.zeros((len(bands), I[sw.sizes[0]]["band"].shape[0], stride), np.float32)
    for j, (F, _, _) in enumerate(bands):
        out[j, :, :I[F]["band"].shape[1]] = I[F]["band"]
    return out


def new_sweep(fv, I, cfgs, sizes, seconds):
    S = len(seconds)
    sw = fv.VadSweep(S, cfgs, fft_size=I["F"]) if sizes is None else fv.VadSweepSized(S, cfgs, sizes)
    sw.set_references(labels(seconds), STAT)
    return sw


def one_shot(fv, ctx, chain, I, cfgs, seconds, sizes=None):
    """one fvad_vad_batch_run_device(_sized) with vad_chain = chain -> the sweep (scored on the device)"""
    ctx.set_option("vad_chain", chain)
    try:
        sw = new_sweep(fv, I, cfgs, sizes, seconds)
        J = I if sizes is None else I[sw.sizes[0]]
        band = blocks(sw, I, sizes)
        d = upload(ctx, band)
        try:
            if sizes is None:
                sw.run_device(ctx, d, band.shape[2], I["n_frames"], I["rms"], I["n_chunks"])
            else:
                sw.run_device_sized(ctx, d, band.shape[2], [I[F]["n_frames"] for F in sw.sizes], J["rms"], J["n_chunks"])
        finally:
            ctx.device_free(d)
        assert sw.chain_form() == (2 if chain == "coop" else 1)
        return sw
    finally:
        ctx.set_option("vad_chain", None)


def snapshot(sw, S, NC, scored=True):
    """everything a run leaves, as raw bits: per machine segments, audit and lazy statistics; per config the scores"""
    segs = [sw.segments(c) for c in range(NC)]
    out = {"segs": [[V.seg_bits(segs[c][s]) for c in range(NC)] for s in range(S)],
           "audit": [[V.audit_bits(sw.audit(s, c)) for c in range(NC)] for s in range(S)],
           "lazy": [[tuple(int(x) for x in sw.lazy_stats(s, c)) for c in range(NC)] for s in range(S)]}
    if scored:
        out["scores"] = [sw.config_stats(c).view(np.uint32).tolist() for c in range(NC)]
    return out


def assert_same(got, want, what):
    for k in want:
        assert got[k] == want[k], (what, k)


def assert_oracle(snap, want, what):
    for s, row in enumerate(want):
        for c, (segs, audit) in enumerate(row):
            assert snap["segs"][s][c] == V.seg_bits(segs), (what, s, c)
            assert snap["audit"][s][c] == V.audit_bits(audit), (what, s, c)


def both(fv, ctx, I, cfgs, seconds, what, sizes=None, want=None):
    """lane and coop one-shot runs: equal bits, coop equal to the oracle; -> coop's snapshot"""
    S, NC = len(seconds), len(cfgs)
    snaps = {}
    for chain in ("lane", "coop"):
        sw = one_shot(fv, ctx, chain, I, cfgs, seconds, sizes)
        snaps[chain] = snapshot(sw, S, NC)
        sw.close()
    assert_same(snaps["coop"], snaps["lane"], what)
    assert_oracle(snaps["coop"], K.oracle(I, cfgs, sizes) if want is None else want, what)
    return snaps["coop"]


def steady_chains(snap, s, c):
    """(exact evaluations, lazy pushes) of a machine.  The machines run the exact chain on a full ring only (before that the
    reference's growing average is summed push by push), so one exact evaluation is one pass through the cooperative section
    in steady state; the case streams were checked against that on the CPU before the bounds below were written"""
    return snap["lazy"][s][c]


@pytest.mark.parametrize("F", [512, 1024])
def test_ring_lengths_around_every_boundary(fv, pkg, gpu_ctx, F):
    """rings of 1 .. 5, 63 .. 65, 255 .. 257 and TILE - 1 .. TILE + 1 slots, exactly on and one f32 ulp below, with and without an
    initial average, on 60 s (the longest ring fills after 11 / 22 s)"""
    seconds = [60.0]
    I = K.inputs(pkg, seconds, F, seed=F)
    cfgs = K.ring_configs(F)
    lens = sorted({V.ring_len(K.RATE, F, c["long_term_speech_avg_sec"]) for c in cfgs})
    assert set(K.RINGS) <= set(lens) and K.TILE - 2 in lens
    snap = both(fv, gpu_ctx, I, cfgs, seconds, ("rings", F))
    for c in range(len(cfgs)):
        ex, lazy = steady_chains(snap, 0, c)
        assert ex >= 1 and lazy >= 1, (F, cfgs[c], ex, lazy)


def test_initial_average_on_a_stream_shorter_than_the_window(fv, pkg, gpu_ctx):
    """a 300 s window (14062 slots) on 40 s: with an initial average the ring is full from the first frame and lt_filled stays
    below long_len inside every chain; without one the ring never fills (no chain: the form must still agree)"""
    seconds = [40.0]
    I = K.inputs(pkg, seconds, seed=3)
    cfgs = [{"long_term_speech_avg_sec": 300.0, "initial_long_term_avg": 0.01, "speech_threshold_factor": 4.0, **K.FAST},
            {"long_term_speech_avg_sec": 300.0, "has_initial_long_term_avg": 0, "speech_threshold_factor": 4.0, **K.FAST},
            {"initial_long_term_avg": 0.01, "speech_threshold_factor": 4.0, **K.FAST}]
    snap = both(fv, gpu_ctx, I, cfgs, seconds, "initial")
    assert steady_chains(snap, 0, 0)[0] >= 1 and steady_chains(snap, 0, 0)[1] >= 1
    assert steady_chains(snap, 0, 2)[0] >= 1
    assert steady_chains(snap, 0, 1) == (0, 0)


@pytest.mark.parametrize("n", [1, 21, 63, 64, 65, 130])
def test_partial_wavefronts(fv, pkg, gpu_ctx, n):
    seconds = [30.0]
    I = K.inputs(pkg, seconds, seed=n)
    cfgs = K.factor_configs(n, n)
    snap = both(fv, gpu_ctx, I, cfgs, seconds, ("machines", n))
    assert all(steady_chains(snap, 0, c)[0] >= 1 for c in range(0, n, 3))


@pytest.mark.parametrize("kind", ["identical", "factor"])
def test_several_owners_in_one_frame(fv, pkg, gpu_ctx, kind):
    """64 identical configs on one stream: every lane asks for the chain in the same frames (64 owners at once); 64 configs that
    differ in the factor only: the owners of a frame are scattered over the wavefront"""
    seconds = [30.0]
    I = K.inputs(pkg, seconds, seed=64)
    cfgs = [dict(K.factor_configs(1, 0)[0]) for _ in range(64)] if kind == "identical" else K.factor_configs(64, 7)
    want = None
    if kind == "identical":   # (one oracle machine serves all 64)
        want = [[K.oracle(I, cfgs[:1])[0][0]] * 64]
    snap = both(fv, gpu_ctx, I, cfgs, seconds, ("owners", kind), want=want)
    ex = [steady_chains(snap, 0, c)[0] for c in range(64)]
    if kind == "identical":
        assert len(set(ex)) == 1 and ex[0] >= 1   # the same frames in every lane: at least two owners per cooperative section
    else:   # every third config sits on the near-threshold frames: 22 machines that run the chain in the same frames
        assert min(ex[0::3]) >= 1 and len(set(ex[0::3])) == 1 and len(set(ex)) > 1


@pytest.mark.parametrize("lane_map", ["stream", "config"])
def test_ring_lengths_mixed_in_a_wavefront_and_the_config_lane_map(fv, pkg, gpu_ctx, lane_map):
    """by stream the lanes of a wavefront have windows of 2, 6, 15 and 20 s side by side; by config a config's three streams"""
    seconds = [40.0, 40.0, 40.0]
    I = K.inputs(pkg, seconds, seed=11)
    cfgs = K.window_configs(24)
    gpu_ctx.set_option("vad_lane_map", lane_map)
    try:
        snap = both(fv, gpu_ctx, I, cfgs, seconds, ("lane map", lane_map))
    finally:
        gpu_ctx.set_option("vad_lane_map", None)
    assert all(steady_chains(snap, s, c)[0] >= 1 for s in range(3) for c in range(24))


def test_streams_of_different_length_share_a_wavefront(fv, pkg, gpu_ctx):
    """3 streams x 20 configs in one wavefront, 20, 45 and 70 s: the lanes of the ended streams go on helping the others' chains.
    The last config's 50 s window without an initial average cannot be full before second 50, so its chains on the longest
    stream all run after the two other streams' lanes have ended"""
    seconds = [20.0, 45.0, 70.0]
    I = K.inputs(pkg, seconds, seed=5)
    cfgs = K.window_configs(19) + [{"long_term_speech_avg_sec": 50.0, "has_initial_long_term_avg": 0, "speech_threshold_factor": 4.0, **K.FAST}]
    snap = both(fv, gpu_ctx, I, cfgs, seconds, "lengths")
    assert steady_chains(snap, 2, 19)[0] >= 1 and steady_chains(snap, 0, 19) == steady_chains(snap, 1, 19) == (0, 0)
    assert all(steady_chains(snap, 2, c)[0] >= 1 for c in range(19))


def run_parts(fv, ctx, I, cfgs, seconds, cuts, chains, use_async=(), retain_at=None, keep=None):
    """the stream in parts ending at chunks `cuts`, part i with vad_chain = chains[i] (part i in use_async: the async call);
    retain_at: the part before which the configs `keep` are retained -> the sweep"""
    S = len(seconds)
    F = I["F"]
    sw = fv.VadSweep(S, cfgs, fft_size=F)
    sw.set_references(labels(seconds), STAT)
    c0 = 0
    forms = []
    try:
        for i, c1 in enumerate(cuts):
            if retain_at == i:
                sw.retain(ctx, keep)
            ctx.set_option("vad_chain", chains[i])
            f0 = c0 * K.CHUNK // F
            nf = [max(0, min(n, c1 * K.CHUNK // F) - f0) for n in I["n_frames"]]
            nc = [max(0, min(n, c1) - c0) for n in I["n_chunks"]]
            pb = np.ascontiguousarray(I["band"][None, :, f0:f0 + max(max(nf), 1)])
            prms = np.ascontiguousarray(I["rms"][:, c0:c1])
            d = upload(ctx, pb)
            d_rms = None
            try:
                if i in use_async:
                    d_rms = upload(ctx, prms)
                    sw.run_device_part_async(ctx, d, pb.shape[2], nf, d_rms, prms.shape[1], nc, c0 * K.CHUNK)
                    sw.part_wait(ctx)
                else:
                    sw.run_device_part(ctx, d, pb.shape[2], nf, prms, nc, f0)
            finally:
                ctx.device_free(d)
                if d_rms is not None:
                    ctx.device_free(d_rms)
            forms.append(sw.chain_form())
            c0 = c1
    finally:
        ctx.set_option("vad_chain", None)
    assert forms == [2 if ch == "coop" else 1 for ch in chains]
    sw.score(4)
    return sw


def test_parts_switch_forms_pause_for_room_and_run_async(fv, pkg, gpu_ctx):
    """three parts lane -> coop -> lane, two segments of room per machine (machines pause at different frames while others run on,
    the room grows and the part is launched again), the coop part also through the async call; against one lane-form launch"""
    ctx = gpu_ctx
    seconds = [48.0, 40.0]
    I = K.inputs(pkg, seconds, seed=21)
    cfgs = [dict(c, has_initial_long_term_avg=1) for c in K.window_configs(12)]
    cfgs += [dict(c, has_initial_long_term_avg=1, initial_long_term_avg=0.02, speech_threshold_factor=f)
             for c, f in zip(K.factor_configs(6, 2), [3.0, 3.5, 4.0, 4.5, 5.0, 6.0])]
    S, NC = 2, len(cfgs)
    ref = one_shot(fv, ctx, "lane", I, cfgs, seconds)
    want = snapshot(ref, S, NC)
    ref.close()
    assert min(len(want["segs"][s][c]) for s in range(S) for c in range(NC)) >= 5
    assert len({len(want["segs"][s][0]) for s in range(S)}) > 1   # the two streams' machines (one wavefront) fill their room apart
    assert all(want["lazy"][s][c][0] >= 1 for s in range(S) for c in range(NC))
    assert_oracle(want, K.oracle(I, cfgs), "parts reference")
    ctx.set_option("vad_seg_cap", "2")
    try:
        for chains, use_async in ((("lane", "coop", "lane"), ()), (("coop", "coop", "coop"), ()), (("lane", "coop", "coop"), (1, 2))):
            sw = run_parts(fv, ctx, I, cfgs, seconds, [32, 64, 96], chains, use_async)
            assert_same(snapshot(sw, S, NC), want, ("parts", chains, use_async))
            sw.close()
    finally:
        ctx.set_option("vad_seg_cap", None)


def test_retain_between_two_cooperative_parts(fv, pkg, gpu_ctx):
    ctx = gpu_ctx
    seconds = [48.0, 48.0]
    I = K.inputs(pkg, seconds, seed=31)
    cfgs = K.window_configs(16)
    keep = [1, 2, 3, 7, 10, 15]
    kept = [cfgs[c] for c in keep]
    sw = run_parts(fv, ctx, I, cfgs, seconds, [32, 96], ("coop", "coop"), retain_at=1, keep=keep)
    got = snapshot(sw, 2, len(keep))
    sw.close()
    fresh = run_parts(fv, ctx, I, kept, seconds, [32, 96], ("coop", "coop"))
    assert_same(got, snapshot(fresh, 2, len(keep)), "retain against a fresh batch")
    fresh.close()
    assert_oracle(got, K.oracle(I, kept), "retain")
    assert all(got["lazy"][s][c][0] >= 1 for s in range(2) for c in range(len(keep)))


def test_sized_batch(fv, pkg, gpu_ctx):
    """machines at 512 and 2048 points in one launch (the sized form of the kernel)"""
    seconds = [40.0, 32.0]
    I = {F: K.inputs(pkg, seconds, F, seed=F) for F in (512, 2048)}
    for F in I:   # (one chunk RMS for both sizes: the streams are the same audio)
        I[F]["rms"] = I[512]["rms"]
        I[F]["ratio"] = [pkg.simulator.frame_ratios(np.ascontiguousarray(I[512]["rms"][s:s + 1, :nc].T), I[F]["n_frames"][s], fft_size=F,
                                                    chunk=K.CHUNK) for s, nc in enumerate(I[F]["n_chunks"])]
    cfgs = K.window_configs(16)
    sizes = [512 if c % 3 else 2048 for c in range(16)]
    snap = both(fv, gpu_ctx, I, cfgs, seconds, "sized", sizes=sizes)
    assert all(steady_chains(snap, s, c)[0] >= 1 for s in range(2) for c in range(16))


def test_global_ring_form(fv, pkg, gpu_ctx):
    """a 3 s short window at 512 points (282 slots): the short rings of a workgroup no longer fit in LDS and live in global memory"""
    seconds = [40.0]
    I = K.inputs(pkg, seconds, 512, seed=9)
    cfgs = [dict(c, short_term_speech_avg_sec=3.0 if i % 2 else 0.2) for i, c in enumerate(K.window_configs(8))]
    snap = both(fv, gpu_ctx, I, cfgs, seconds, "global rings")
    assert all(steady_chains(snap, 0, c)[0] >= 1 for c in range(8))


def test_ten_minute_stream_with_the_default_and_the_300_s_window(fv, pkg, gpu_ctx):
    """vad_oracle_cases' ten-minute drift stream at 1024 points: the default 8437-slot ring and a 300 s window (14062 slots)"""
    seconds = [600.0]
    I = K.inputs(pkg, seconds, seed=0, stress=True)
    cfgs = [{}, {"long_term_speech_avg_sec": 300.0, "speech_threshold_factor": 10.0},
            {"has_initial_long_term_avg": 0, "long_term_speech_avg_sec": 60.0, "speech_threshold_factor": 10.0}]
    assert V.ring_len(K.RATE, 1024, 180.0) == 8437
    snap = both(fv, gpu_ctx, I, cfgs, seconds, "stress")
    assert all(steady_chains(snap, 0, c)[0] >= 1 and steady_chains(snap, 0, c)[1] >= 4096 for c in range(3))   # (4096 lazy pushes: a re-anchor)


def test_option_rules(fv, pkg, gpu_ctx):
    ctx = gpu_ctx
    with pytest.raises(fv.FvadError) as e:
        ctx.set_option("vad_chain", "bogus")
    assert e.value.status == fv.FVAD_ERR_INVALID_ARGUMENT
    seconds = [20.0]
    I = K.inputs(pkg, seconds, seed=1)
    cfgs = K.factor_configs(3, 1)
    for restore in (None, ""):
        ctx.set_option("vad_chain", "coop")
        ctx.set_option("vad_chain", restore)
        sw = new_sweep(fv, I, cfgs, None, seconds)
        assert sw.chain_form() == 0
        d = upload(ctx, np.ascontiguousarray(I["band"][None]))
        try:
            sw.run_device(ctx, d, I["band"].shape[1], I["n_frames"], I["rms"], I["n_chunks"])
        finally:
            ctx.device_free(d)
        assert sw.chain_form() == 1
        sw.close()
