"""The averages' tables of the device VAD machines (context option vad_avgs "table") on the GPU: the table kernels alone
(VadSweep.averages_device) against the oracle's rolling average as uint64 bits, and the table form of the machines against the
ring form (both with vad_chain "coop") and against the oracle's machines, bit for bit -- segments, audits, lazy statistics and
scores -- in one launch, in parts that switch forms, pause for segment room, retain configs and run async, under a budget too
small for the tables, and through run_grid.  Every case asserts from avgs_form() which form really ran."""
import numpy as np
import pytest

import test_vad_chain_gpu as T
from test_vad_score_gpu import write_plan
import vad_avgs_cases as A
import vad_chain_cases as K
import vad_oracle_cases as V

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the table alone
def table_reference(I, sw):
    """{(band, len): [per stream]}, {(size index, len): [per stream]} from orc_ra_push over the whole streams"""
    st_keys, cr_keys, _, _ = sw.avg_keys()
    nch, S = I["nch"], len(I["n_frames"])
    mv = [A.min_volume(I["band"][s * nch:(s + 1) * nch, :I["n_frames"][s]]) for s in range(S)]
    st = {(b, n): [A.oracle_avgs(mv[s], n) for s in range(S)] for b, n in st_keys}
    cr = {(g, n): [A.oracle_avgs(I["ratio"][s], n) for s in range(S)] for g, n in cr_keys}
    return st, cr


def check_table(got, want_st, want_cr, n_frames, first=0, what=None):
    for keys, tab, want in ((got["st_keys"], got["st"], want_st), (got["cr_keys"], got["cr"], want_cr)):
        for j, key in enumerate(keys):
            for s, nf in enumerate(n_frames):
                w = want[key][s][first:first + nf]
                assert (A.bits(tab[j, s, :nf]) == A.bits(w)).all(), (what, key, s, int(np.argmax(A.bits(tab[j, s, :nf]) != A.bits(w))))


def one_size(fv, ctx, seconds, F, nch, cfgs, seed, ties=False):
    I = A.inputs(seconds, F, nch, seed, ties)
    sw = fv.VadSweep(len(seconds), cfgs, n_channels=nch, fft_size=F)
    band = np.ascontiguousarray(I["band"][None])
    d = A.upload(ctx, band)
    try:
        got = sw.averages_device(ctx, d, band.shape[2], I["n_frames"], I["rms"], I["n_chunks"])
        want_st, want_cr = table_reference(I, sw)
        check_table(got, want_st, want_cr, I["n_frames"], what=(F, nch))
        assert sw.avgs_form() == 0   # (the tap changes nothing in the batch)
        return got
    finally:
        ctx.device_free(d)
        sw.close()


@pytest.mark.parametrize("F,nch", [(512, 2), (1024, 1), (1024, 5), (2048, 2), (960, 2)])
def test_table_ring_lengths_sizes_and_channels(fv, gpu_ctx, F, nch):
    """every ring length of TABLE_LENS exactly on and one f32 ulp below, on two streams of different length (40 and 23 s)"""
    cfgs = A.len_configs(F, A.TABLE_LENS, below=True)
    got = one_size(fv, gpu_ctx, [40.0, 23.0], F, nch, cfgs, seed=F + nch)
    lens = {n for _, n in got["st_keys"]}
    assert set(A.TABLE_LENS) <= lens and {n - 1 for n in A.TABLE_LENS if n > 2} <= lens


def test_table_equal_channels_keep_the_first(fv, gpu_ctx):
    one_size(fv, gpu_ctx, [30.0], 1024, 2, A.len_configs(1024, [3, 9, 23]), seed=4, ties=True)


@pytest.mark.parametrize("chunks", [5, 6, 11])
def test_table_frame_tile_and_rings_longer_than_the_stream(fv, gpu_ctx, chunks):
    """at 960 points a chunk is 25 frames: 125, 150 and 275 frames lie below one tile, inside it and one frame tile further; no
    frame count is a multiple of the tile, so with the stream cut below the tail workgroup is partial.  Rings of 282 and 400
    slots never fill on the short streams"""
    F = 960
    for cut in (A.TILE - 1, A.TILE, A.TILE + 1, None):
        I = A.inputs([chunks * 0.5], F, 1, seed=chunks)
        if cut is not None:
            if I["n_frames"][0] < cut:
                continue
            I["n_frames"] = [cut]
            I["ratio"] = [I["ratio"][0][:cut]]
        cfgs = A.len_configs(F, [9, 64, 282, 400])
        sw = fv.VadSweep(1, cfgs, fft_size=F)
        band = np.ascontiguousarray(I["band"][None])
        d = A.upload(gpu_ctx, band)
        try:
            got = sw.averages_device(gpu_ctx, d, band.shape[2], I["n_frames"], I["rms"], I["n_chunks"])
            want_st, want_cr = table_reference(I, sw)
            check_table(got, want_st, want_cr, I["n_frames"], what=(chunks, cut))
        finally:
            gpu_ctx.device_free(d)
            sw.close()


def test_table_part_shorter_than_the_ring_reads_the_homes(fv, gpu_ctx):
    """a first part of 32 chunks run by the ring form, then the tap on a second part of 2 chunks (93 frames at 1024 points): rings
    of 256, 257 and 282 slots hold mostly frames of the first part, which the tap reads from the rings' homes"""
    ctx = gpu_ctx
    I = A.inputs([40.0, 40.0], 1024, 2, seed=8)
    cfgs = A.len_configs(1024, [9, 93, 94, 256, 257, 282])
    sw = fv.VadSweep(2, cfgs, n_channels=2)
    try:
        want_st, want_cr = table_reference(I, sw)
        with pytest.raises(fv.FvadError) as e:   # no part state to read the history from
            part_tap(fv, ctx, sw, I, 32, 34)
        assert e.value.status == fv.FVAD_ERR_INVALID_ARGUMENT
        for lane_map in ("stream", "config"):
            ctx.set_option("vad_lane_map", lane_map)
            try:
                run_part(ctx, sw, I, 0, 32, "ring")
                assert sw.avgs_form() == 1
                got = part_tap(fv, ctx, sw, I, 32, 34)
            finally:
                ctx.set_option("vad_lane_map", None)
            nf = [2 * K.CHUNK // 1024] * 2
            check_table(got, want_st, want_cr, nf, first=32 * K.CHUNK // 1024, what=lane_map)
    finally:
        sw.close()


def part_counts(I, c0, c1):
    F = I["F"]
    f0 = c0 * K.CHUNK // F
    nf = [max(0, min(n, c1 * K.CHUNK // F) - f0) for n in I["n_frames"]]
    nc = [max(0, min(n, c1) - c0) for n in I["n_chunks"]]
    return f0, nf, nc


def part_tap(fv, ctx, sw, I, c0, c1):
    f0, nf, nc = part_counts(I, c0, c1)
    pb = np.ascontiguousarray(I["band"][None, :, f0:f0 + max(max(nf), 1)])
    d = A.upload(ctx, pb)
    try:
        return sw.averages_device(ctx, d, pb.shape[2], nf, np.ascontiguousarray(I["rms"][:, c0:c1]), nc, first_sample=c0 * K.CHUNK)
    finally:
        ctx.device_free(d)


def run_part(ctx, sw, I, c0, c1, avgs, use_async=False, blocks=None):
    """chunks [c0, c1) of every stream as one device part with vad_chain coop and vad_avgs = avgs"""
    f0, nf, nc = part_counts(I, c0, c1)
    src = I["band"][None] if blocks is None else blocks
    pb = np.ascontiguousarray(src[:, :, f0:f0 + max(max(nf), 1)])
    prms = np.ascontiguousarray(I["rms"][:, c0:c1])
    ctx.set_option("vad_chain", "coop")
    ctx.set_option("vad_avgs", avgs)
    d = A.upload(ctx, pb)
    d_rms = None
    try:
        if use_async:
            d_rms = A.upload(ctx, prms)
            sw.run_device_part_async(ctx, d, pb.shape[2], nf, d_rms, prms.shape[1], nc, c0 * K.CHUNK)
            assert sw.avgs_form() == (2 if avgs == "table" else 1)   # (counted when queued)
            sw.part_wait(ctx)
        else:
            sw.run_device_part(ctx, d, pb.shape[2], nf, prms, nc, f0)
    finally:
        ctx.device_free(d)
        if d_rms is not None:
            ctx.device_free(d_rms)
        ctx.set_option("vad_chain", None)
        ctx.set_option("vad_avgs", None)


# ------------------------------------------------------------------ the machines: table against ring against the oracle
def one_shot(fv, ctx, avgs, I, cfgs, seconds, sizes=None, blocks=None, want_form=None):
    ctx.set_option("vad_avgs", avgs)
    try:
        if blocks is None:
            sw = T.one_shot(fv, ctx, "coop", I, cfgs, seconds, sizes)
        else:
            ctx.set_option("vad_chain", "coop")
            sw = T.new_sweep(fv, I, cfgs, None, seconds)
            d = A.upload(ctx, blocks)
            try:
                sw.run_device(ctx, d, blocks.shape[2], I["n_frames"], I["rms"], I["n_chunks"])
            finally:
                ctx.device_free(d)
                ctx.set_option("vad_chain", None)
    finally:
        ctx.set_option("vad_avgs", None)
    assert sw.avgs_form() == (want_form or (2 if avgs == "table" else 1)), avgs
    assert (sw.avgs_bytes() > 0) == (sw.avgs_form() == 2)
    return sw


def both(fv, ctx, I, cfgs, seconds, what, sizes=None, blocks=None, want=None):
    """ring and table one-shot runs (coop): equal bits, and equal to the oracle -> the table run's snapshot"""
    S, NC = len(seconds), len(cfgs)
    snaps = {}
    for avgs in ("ring", "table"):
        sw = one_shot(fv, ctx, avgs, I, cfgs, seconds, sizes, blocks)
        snaps[avgs] = T.snapshot(sw, S, NC)
        sw.close()
    T.assert_same(snaps["table"], snaps["ring"], what)
    T.assert_oracle(snaps["table"], K.oracle(I, cfgs, sizes) if want is None else want, what)
    return snaps["table"]


def two_band_blocks(fv, I, cfgs, seed):
    """band blocks [2][S][frames] for configs on two speech bands (block 1 another script()), and the oracle's machines on them"""
    probe = fv.VadSweep(1, cfgs, fft_size=I["F"])
    bands, band_of = probe.bands()
    probe.close()
    assert len(bands) == 2
    S = len(I["n_frames"])
    blocks = np.zeros((2, S, I["band"].shape[1]), np.float32)
    blocks[0] = I["band"]
    for s, nf in enumerate(I["n_frames"]):
        blocks[1, s, :nf] = K.script(nf, I["F"], seed + 50 + s) * np.float32(0.75)
    jobs = [(cfg, K.RATE, 1, I["F"], blocks[band_of[c], s:s + 1, :I["n_frames"][s]], I["ratio"][s]) for s in range(S) for c, cfg in enumerate(cfgs)]
    res = iter(V.oracle_machines(jobs))
    return blocks, [[next(res) for _ in cfgs] for _ in range(S)]


@pytest.mark.parametrize("lane_map", ["stream", "config"])
def test_grid_with_shared_keys(fv, pkg, gpu_ctx, lane_map):
    """128 configs (8 short keys, 2 ratio keys) on two streams of 30 and 22 s: two wavefronts per stream by stream"""
    seconds = [30.0, 22.0]
    I = K.inputs(pkg, seconds, seed=41)
    cfgs = A.shared_grid()
    blocks, want = two_band_blocks(fv, I, cfgs, 41)
    gpu_ctx.set_option("vad_lane_map", lane_map)
    try:
        snap = both(fv, gpu_ctx, I, cfgs, seconds, ("shared", lane_map), blocks=blocks, want=want)
    finally:
        gpu_ctx.set_option("vad_lane_map", None)
    assert sum(len(snap["segs"][0][c]) for c in range(128)) > 128


@pytest.mark.parametrize("n", [5, 70])
def test_every_config_its_own_key(fv, pkg, gpu_ctx, n):
    """fewer than 64 machines per stream, and more; the 0.0 s short window (one slot) among them"""
    seconds = [30.0]
    I = K.inputs(pkg, seconds, seed=n)
    cfgs = A.unique_grid(n - 1) + [{"short_term_speech_avg_sec": 0.0, "speech_threshold_factor": 4.0, "long_term_speech_avg_sec": 5.0,
                                    "has_initial_long_term_avg": 0, **A.FAST}]
    snap = both(fv, gpu_ctx, I, cfgs, seconds, ("unique", n))
    assert len(snap["segs"][0][n - 1]) >= 1 and snap["lazy"][0][n - 1][0] >= 1


def test_sized_batch(fv, pkg, gpu_ctx):
    seconds = [40.0, 32.0]
    I = {F: K.inputs(pkg, seconds, F, seed=F) for F in (512, 2048)}
    for F in I:
        I[F]["rms"] = I[512]["rms"]
        I[F]["ratio"] = [pkg.simulator.frame_ratios(np.ascontiguousarray(I[512]["rms"][s:s + 1, :nc].T), I[F]["n_frames"][s], fft_size=F,
                                                    chunk=K.CHUNK) for s, nc in enumerate(I[F]["n_chunks"])]
    cfgs = [dict(c, short_term_speech_avg_sec=[0.2, 0.5, 3.0][i % 3]) for i, c in enumerate(K.window_configs(16))]
    sizes = [512 if c % 3 else 2048 for c in range(16)]
    snap = both(fv, gpu_ctx, I, cfgs, seconds, "sized", sizes=sizes)
    assert all(snap["lazy"][s][c][0] >= 1 for s in range(2) for c in range(16))


# ------------------------------------------------------------------ parts
PARTS_F = 960   # 25 frames per chunk: a part may start at any chunk (at 1024 points only at every 16th)


def parts_cfgs():
    """short windows of 0.6, 1 and 2 s and ratio windows of 0.6 and 1.5 s: at PARTS_F 30 .. 100 slots, every ring longer than a
    part of one chunk"""
    cfgs = [dict(c, has_initial_long_term_avg=1, short_term_speech_avg_sec=[0.6, 1.0, 2.0][i % 3], channel_vol_ratio_avg_sec=0.6)
            for i, c in enumerate(K.window_configs(12))]
    cfgs += [dict(c, has_initial_long_term_avg=1, initial_long_term_avg=0.02, speech_threshold_factor=f, channel_vol_ratio_avg_sec=1.5,
                  short_term_speech_avg_sec=0.6) for c, f in zip(K.factor_configs(6, 2), [3.0, 3.5, 4.0, 4.5, 5.0, 6.0])]
    return cfgs


def run_parts(fv, ctx, I, cfgs, seconds, cuts, forms, use_async=(), retain_at=None, keep=None):
    sw = fv.VadSweep(len(seconds), cfgs, fft_size=I["F"])
    sw.set_references(T.labels(seconds), T.STAT)
    c0 = 0
    for i, c1 in enumerate(cuts):
        if retain_at == i:
            sw.retain(ctx, keep)
        run_part(ctx, sw, I, c0, c1, forms[i], use_async=i in use_async)
        assert sw.avgs_form() == (2 if forms[i] == "table" else 1) and sw.chain_form() == 2, (i, forms[i])
        c0 = c1
    sw.score(4)
    return sw


def test_parts_switch_forms_pause_for_room_and_run_async(fv, pkg, gpu_ctx):
    """3 and 7 parts ring -> table -> ring -> table ..., parts of one chunk (25 frames at 960 points: shorter than every ring), two
    segments of room per machine (machines pause and are relaunched inside a table part, which reads the
    tables again), table parts through the async call; against one ring-form launch and the oracle"""
    ctx = gpu_ctx
    seconds = [48.0, 40.0]
    I = K.inputs(pkg, seconds, PARTS_F, seed=21)
    cfgs = parts_cfgs()
    S, NC = 2, len(cfgs)
    ref = one_shot(fv, ctx, "ring", I, cfgs, seconds)
    want = T.snapshot(ref, S, NC)
    ref.close()
    T.assert_oracle(want, K.oracle(I, cfgs), "parts reference")
    # many machines close more segments than the room of two holds (they pause), others close none or one (they run on beside them)
    counts = [len(want["segs"][s][c]) for s in range(S) for c in range(NC)]
    assert sum(n >= 3 for n in counts) >= 12 and sum(n < 2 for n in counts) >= 2
    ctx.set_option("vad_seg_cap", "2")
    try:
        alt = ("ring", "table") * 4
        for cuts, forms, use_async in (([32, 64, 96], ("table", "ring", "table"), ()), ([32, 64, 96], ("table",) * 3, (1, 2)),
                                       ([7, 8, 31, 50, 51, 80, 96], alt[:7], ()), ([7, 8, 31, 50, 51, 80, 96], alt[1:8], (2, 4))):
            sw = run_parts(fv, ctx, I, cfgs, seconds, cuts, forms, use_async)
            T.assert_same(T.snapshot(sw, S, NC), want, ("parts", cuts, forms, use_async))
            assert sw.device_bytes() > 0
            sw.close()
    finally:
        ctx.set_option("vad_seg_cap", None)


def test_retain_between_table_parts(fv, pkg, gpu_ctx):
    """retain between table parts drops the only configs of a short key and of a ratio key (the representative machines of the
    kept keys move to new places); the later table parts read their history from the gathered homes.  Equal to a fresh batch of
    the survivors, and to the oracle"""
    ctx = gpu_ctx
    seconds = [48.0, 48.0]
    I = K.inputs(pkg, seconds, PARTS_F, seed=31)
    cfgs = [dict(c, short_term_speech_avg_sec=[0.2, 0.5, 1.0, 2.0][i % 4], channel_vol_ratio_avg_sec=1.5 if i == 0 else 0.5)
            for i, c in enumerate(K.window_configs(16))]
    keep = [1, 2, 4, 5, 6, 10, 13]   # no config of the 2.0 s window, nor config 0 with the only 1.5 s ratio window
    kept = [cfgs[c] for c in keep]
    sw = run_parts(fv, ctx, I, cfgs, seconds, [20, 21, 60, 96], ("table",) * 4, retain_at=2, keep=keep)
    got = T.snapshot(sw, 2, len(keep))
    assert len(sw.avg_keys()[0]) == 3 and len(sw.avg_keys()[1]) == 1
    sw.close()
    fresh = run_parts(fv, ctx, I, kept, seconds, [20, 21, 60, 96], ("table", "ring", "table", "table"))
    T.assert_same(got, T.snapshot(fresh, 2, len(keep)), "retain against a fresh batch")
    fresh.close()
    T.assert_oracle(got, K.oracle(I, kept), "retain")


def test_retain_drops_a_band(fv, pkg, gpu_ctx):
    ctx = gpu_ctx
    seconds = [30.0]
    I = K.inputs(pkg, seconds, seed=33)
    cfgs = [c for c in A.shared_grid() if c["speech_threshold_factor"] in (4.0, 5.0)][:16]
    blocks, want = two_band_blocks(fv, I, cfgs, 33)
    probe = fv.VadSweep(1, cfgs)
    band_of = probe.bands()[1]
    probe.close()
    keep = [c for c in range(16) if band_of[c] == 1]
    sw = fv.VadSweep(1, cfgs)
    try:
        run_part(ctx, sw, I, 0, 32, "table", blocks=blocks)
        sw.retain(ctx, keep)
        assert len(sw.bands()[0]) == 1
        run_part(ctx, sw, I, 32, 60, "table", blocks=blocks[1:])
        assert sw.avgs_form() == 2
        for j, c in enumerate(keep):
            assert V.seg_bits(sw.segments(j)[0]) == V.seg_bits(want[0][c][0]), c
            assert V.audit_bits(sw.audit(0, j)) == V.audit_bits(want[0][c][1]), c
    finally:
        sw.close()


def test_budget_too_small_runs_the_rings(fv, pkg, gpu_ctx):
    ctx = gpu_ctx
    seconds = [30.0]
    I = K.inputs(pkg, seconds, seed=6)
    cfgs = A.unique_grid(8)
    full = one_shot(fv, ctx, "table", I, cfgs, seconds)
    need = full.avgs_bytes()
    want = T.snapshot(full, 1, 8)
    full.close()
    assert need == I["n_frames"][0] * (16 * 8 + 4)   # 8 + 8 keys of f64, one min_volume row
    for budget, form in ((need - 1, 1), (need, 2)):
        ctx.set_option("vad_avgs_max_bytes", str(budget))
        try:
            sw = one_shot(fv, ctx, "table", I, cfgs, seconds, want_form=form)
            T.assert_same(T.snapshot(sw, 1, 8), want, ("budget", budget))
            sw.close()
            # the same rule in a part
            sw = fv.VadSweep(1, cfgs)
            run_part(ctx, sw, I, 0, 60, "table")
            assert sw.avgs_form() == form
            sw.close()
        finally:
            ctx.set_option("vad_avgs_max_bytes", None)


def test_option_rules(fv, pkg, gpu_ctx):
    ctx = gpu_ctx
    for name, bad in (("vad_avgs", "lds"), ("vad_avgs_max_bytes", "-1"), ("vad_avgs_max_bytes", "1k")):
        with pytest.raises(fv.FvadError) as e:
            ctx.set_option(name, bad)
        assert e.value.status == fv.FVAD_ERR_INVALID_ARGUMENT
    seconds = [20.0]
    I = K.inputs(pkg, seconds, seed=1)
    cfgs = K.factor_configs(3, 1)
    # "table" with the lane form of the kernel: the rings run (the harness refuses the pair; the library falls back)
    ctx.set_option("vad_avgs", "table")
    try:
        sw = T.one_shot(fv, ctx, "lane", I, cfgs, seconds)
        assert sw.avgs_form() == 1 and sw.avgs_bytes() == 0
        sw.close()
    finally:
        ctx.set_option("vad_avgs", None)
    sw = one_shot(fv, ctx, "ring", I, cfgs, seconds)   # (restored: the default)
    sw.close()


def test_run_grid_sliced_halving_overlap(fv, pkg, gpu_ctx, tmp_path):
    """two short stereo streams, 32 configs, sliced with halving and overlap on a reproducible context: the statistics of the
    table run equal the ring run's as uint32"""
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, ((2, "f32", 32.0), (2, "pcm16", 24.5)))
    grid = {"base": {"long_term_speech_avg_sec": 4.0, "min_vad_duration_sec": 0.1},
            "axes": {"short_term_speech_avg_sec": [0.1, 0.2, 0.4, 0.8], "speech_threshold_factor": [2.0, 3.0, 4.0, 6.0],
                     "channel_vol_ratio_avg_sec": [0.3, 0.5]}}
    gpu_ctx.set_option("reproducible", "1")
    try:
        res = {}
        for avgs in ("ring", "table"):
            res[avgs] = sim.run_grid(plan, grid, ctx=gpu_ctx, out=None, vad_on="device", score_on="device", slice_chunks=16,
                                     halving_eta=2, halving_rungs=1, overlap=True, vad_chain="coop", vad_avgs=avgs)
    finally:
        gpu_ctx.set_option("reproducible", None)
    assert gpu_ctx.option_set("vad_avgs") is None and gpu_ctx.option_set("vad_chain") is None
    assert res["ring"]["times"]["avgs_form"] == 1 and res["ring"]["times"]["avgs_bytes"] == 0
    assert res["table"]["times"]["avgs_form"] == 2 and res["table"]["times"]["avgs_bytes"] > 0
    assert res["table"]["slices"] == res["ring"]["slices"] > 1
    assert res["table"]["survivors"] == res["ring"]["survivors"] and len(res["table"]["configs"]) == 32
    a, b = np.asarray(res["table"]["stats"], np.float32), np.asarray(res["ring"]["stats"], np.float32)
    assert a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()
