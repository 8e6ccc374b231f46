"""Shared triggers on the device (context option vad_trigger "shared"): the bits the emitting form of the cooperative kernel
stores against the oracle's threshold_met, and the shared form -- emitting machines, then kernels_vadfinish.hip -- against the
per-config machines and the oracle's machines, bit for bit: segments, counts, audits, lazy statistics and device scores; in one
shot, in parts (blocking and async, with segment room that overflows), across a retain, and through run_grid."""
import json

import numpy as np
import pytest

import vad_avgs_cases as A
import vad_chain_cases as K
import vad_oracle_cases as V
import vad_trigger_cases as T
from test_vad_chain_gpu import STAT, assert_oracle, assert_same, blocks, labels, new_sweep, snapshot, upload
from test_vad_score_gpu import write_plan

pytestmark = pytest.mark.gpu

SECONDS = [40.0, 23.0]   # 1875 and 1078 frames at 1024 points: 30 and 17 words, both last words partial


class options:
    """context options for a block, unset afterwards"""

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            self.ctx.set_option(k, None)


def shared(ctx, **kw):
    return options(ctx, vad_chain="coop", vad_trigger="shared", **kw)


def one_shot(fv, ctx, I, cfgs, seconds, sizes=None):
    """one fvad_vad_batch_run_device(_sized) over vad_chain_cases.inputs (mono) or vad_avgs_cases.inputs (I["nch"] channels)"""
    if sizes is None and I.get("nch", 1) > 1:
        sw = fv.VadSweep(len(seconds), cfgs, n_channels=I["nch"], fft_size=I["F"])
        sw.set_references(labels(seconds), STAT)
    else:
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
    return sw


def oracle_bits(I, cfgs, rep, sizes=None):
    """[key][stream] -> the oracle trace's threshold_met of the key's first config, packed"""
    out = []
    for c in rep:
        J = I if sizes is None else I[sizes[c]]
        nch = J.get("nch", 1)
        row = []
        for s, nf in enumerate(J["n_frames"]):
            _, tr = T.oracle_trace(cfgs[c], K.RATE, nch, J["F"], J["band"][s * nch:(s + 1) * nch, :nf], J["ratio"][s])
            row.append(T.pack(tr["threshold_met"] != 0))
        out.append(row)
    return out


def check_bits(fv, ctx, I, cfgs, seconds, sizes=None):
    """one shared run: the tap's words equal the oracle's for every (key, stream), words past a stream's end are zero"""
    with shared(ctx):
        sw = one_shot(fv, ctx, I, cfgs, seconds, sizes)
    try:
        key_of, rep = sw.trigger_keys()
        assert sw.trigger_form() == 2 and len(rep) < len(cfgs)
        want = oracle_bits(I, cfgs, rep, sizes)
        n_words = max(len(w) for row in want for w in row)
        got = sw.trigger_bits(ctx, n_words)
        rich = [False] * len(seconds)
        for k, row in enumerate(want):
            for s, w in enumerate(row):
                assert got[k, s, :len(w)].tolist() == w.tolist(), (k, s)
                assert not got[k, s, len(w):].any()
                rich[s] = rich[s] or (w.any() and (w == 0).any() and (w != np.uint64(0xFFFFFFFFFFFFFFFF)).any())
        assert all(rich)   # every stream has, for some key, set bits, clear bits and an all-zero word
        assert sw.trigger_bytes() > 0
        # a one-shot run holds nothing but the bits afterwards, and they count
        # (a key's rows are as long as the longest stream of its size: [stream][word][keys of that size])
        assert sw.device_bytes() == sw.trigger_bytes() == 8 * len(seconds) * sum(max(len(w) for w in row) for row in want)
        return snapshot(sw, len(seconds), len(cfgs))
    finally:
        sw.close()


GRID8 = T.grid(T.trigger_configs(8))   # 8 keys x 16 finishing combinations: 128 configs, two wavefronts per stream


@pytest.mark.parametrize("avgs", ["ring", "table"])
@pytest.mark.parametrize("lane_map", ["stream", "config"])
def test_bits_at_1024_points(fv, pkg, gpu_ctx, avgs, lane_map):
    I = K.inputs(pkg, SECONDS, seed=41)
    with options(gpu_ctx, vad_avgs=avgs, vad_lane_map=lane_map):
        check_bits(fv, gpu_ctx, I, GRID8[:32], SECONDS)


@pytest.mark.parametrize("avgs", ["ring", "table"])
@pytest.mark.parametrize("nch,seed", [(2, 50), (5, 51)])
def test_bits_and_results_with_channels(fv, gpu_ctx, nch, seed, avgs):
    """vad_avgs_cases.inputs: the smallest channel changes every seven frames (fetch: the minimum over the channels) and the ratio
    rows come from the channels' RMS; the bits and then every machine's segments and audit against the oracle's at nch channels"""
    I = A.inputs(SECONDS, 1024, nch, seed)
    cfgs = GRID8[:32]
    with options(gpu_ctx, vad_avgs=avgs):
        snap = check_bits(fv, gpu_ctx, I, cfgs, SECONDS)
    jobs = [(cfg, K.RATE, nch, 1024, I["band"][s * nch:(s + 1) * nch, :nf], I["ratio"][s]) for s, nf in enumerate(I["n_frames"]) for cfg in cfgs]
    res = iter(V.oracle_machines(jobs))
    want = [[next(res) for _ in cfgs] for _ in SECONDS]
    assert_oracle(snap, want, ("channels", nch, avgs))
    assert max(len(segs) for row in want for segs, _ in row) >= 2


def test_bits_at_960_points(fv, pkg, gpu_ctx):
    I = K.inputs(pkg, SECONDS, F=960, seed=42)
    check_bits(fv, gpu_ctx, I, GRID8[:24], SECONDS)


@pytest.mark.parametrize("avgs", ["ring", "table"])
def test_bits_of_a_sized_batch(fv, pkg, gpu_ctx, avgs):
    I = {F: K.inputs(pkg, SECONDS, F=F, seed=43) for F in (512, 2048)}
    cfgs = GRID8[:24]
    sizes = [512 if (c // 2) % 2 else 2048 for c in range(len(cfgs))]
    with options(gpu_ctx, vad_avgs=avgs):
        check_bits(fv, gpu_ctx, I, cfgs, SECONDS, sizes)


@pytest.fixture(scope="module")
def case128(pkg):
    I = K.inputs(pkg, SECONDS, seed=44)
    return I, K.oracle(I, GRID8)


@pytest.mark.parametrize("avgs", ["ring", "table"])
def test_shared_equals_per_config_equals_the_oracle(fv, gpu_ctx, case128, avgs):
    I, want = case128
    S, NC = len(SECONDS), len(GRID8)
    with options(gpu_ctx, vad_chain="coop", vad_avgs=avgs):
        ref = one_shot(fv, gpu_ctx, I, GRID8, SECONDS)
        assert ref.trigger_form() == 1 and ref.trigger_bytes() == 0
        a = snapshot(ref, S, NC)
        ref.close()
    with shared(gpu_ctx, vad_avgs=avgs):
        sw = one_shot(fv, gpu_ctx, I, GRID8, SECONDS)
        assert sw.trigger_form() == 2 and len(sw.trigger_keys()[1]) == 8 and sw.trigger_launches() == (1, 1)
        assert sw.avgs_form() == (2 if avgs == "table" else 1)
        b = snapshot(sw, S, NC)
        sw.close()
    assert_same(b, a, ("shared", avgs))
    assert_oracle(b, want, ("shared", avgs))
    assert max(len(b["segs"][s][c]) for s in range(S) for c in range(NC)) >= 2
    assert len({tuple(map(tuple, b["segs"][0][c])) for c in range(0, NC, 8)}) > 1   # the finishing fields matter


@pytest.mark.parametrize("n", [1, 8])
def test_unique_grids_and_a_single_config(fv, pkg, gpu_ctx, n):
    I = K.inputs(pkg, SECONDS, seed=45)
    cfgs = [dict(t, **K.FAST) for t in T.trigger_configs(n)]
    with shared(gpu_ctx):
        sw = one_shot(fv, gpu_ctx, I, cfgs, SECONDS)
        assert sw.trigger_form() == 2 and len(sw.trigger_keys()[1]) == n
        snap = snapshot(sw, len(SECONDS), n)
        sw.close()
    assert_oracle(snap, K.oracle(I, cfgs), ("unique", n))


def run_parts(fv, ctx, I, cfgs, seconds, cuts, use_async=(), keep_segments=1, retain_at=None, keep=None, flip_at=None):
    """the streams in parts ending at chunks `cuts` (part i in use_async: the async call) -> the sweep"""
    sw = fv.VadSweep(len(seconds), cfgs, fft_size=I["F"])
    sw.set_references(labels(seconds), V.STAT_CFGS[1])
    sw.keep_segments(keep_segments)
    F, c0 = I["F"], 0
    for i, c1 in enumerate(cuts):
        if retain_at == i:
            sw.retain(ctx, keep)
        if flip_at == i:   # the option changed mid-run: the run keeps its form
            ctx.set_option("vad_trigger", "config" if ctx.option_set("vad_trigger") == "shared" else "shared")
        f0 = c0 * K.CHUNK // F
        nf = [max(0, min(n, c1 * K.CHUNK // F) - f0) for n in I["n_frames"]]
        nc = [max(0, min(n, c1) - c0) for n in I["n_chunks"]]
        pb = np.ascontiguousarray(I["band"][None, :, f0:f0 + max(max(nf), 1)])
        prms = np.ascontiguousarray(I["rms"][:, c0:c1])
        d, d_rms = upload(ctx, pb), None
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
        c0 = c1
    return sw


CUTS = [16, 32, 80]   # 16-chunk cuts: parts start at frames 0, 375, 750 -- not on words; the 23 s stream ends inside the last


@pytest.mark.parametrize("use_async", [(), (0, 1, 2)], ids=["blocking", "async"])
@pytest.mark.parametrize("keep", [0, 1])
def test_parts_with_room_that_overflows(fv, gpu_ctx, case128, use_async, keep):
    I, want = case128
    S, NC = len(SECONDS), len(GRID8)
    with shared(gpu_ctx, vad_seg_cap="2"):
        sw = run_parts(fv, gpu_ctx, I, GRID8, SECONDS, CUTS, use_async, keep_segments=keep)
        machines, finish = sw.trigger_launches()
        assert sw.trigger_form() == 2 and machines == len(CUTS) and finish > len(CUTS)   # only the finishing kernel ran again
        assert sw.trigger_bytes() > 0 and sw.device_bytes() > sw.trigger_bytes()
        if keep:
            sw.score(4)
            assert_oracle(snapshot(sw, S, NC), want, ("parts", use_async))
        else:
            sw.score_device(gpu_ctx)
            got = [sw.config_stats(c).view(np.uint32).tolist() for c in range(NC)]
            for s in range(S):
                for c in range(NC):
                    assert V.audit_bits(sw.audit(s, c)) == V.audit_bits(want[s][c][1])
        sw.close()
    if not keep:
        with options(gpu_ctx, vad_chain="coop"):
            ref = one_shot(fv, gpu_ctx, I, GRID8, SECONDS)
            assert got == [ref.config_stats(c).view(np.uint32).tolist() for c in range(NC)]
            ref.close()


def test_one_shot_with_room_that_overflows_launches_the_machines_once(fv, gpu_ctx, case128):
    I, want = case128
    with shared(gpu_ctx, vad_seg_cap="1"):
        sw = one_shot(fv, gpu_ctx, I, GRID8, SECONDS)
        machines, finish = sw.trigger_launches()
        assert machines == 1 and finish > 1
        assert_oracle(snapshot(sw, len(SECONDS), len(GRID8)), want, "one shot, room 1")
        sw.close()


@pytest.mark.parametrize("what", ["whole keys", "parts of keys", "representative", "long window"])
def test_retain_between_parts(fv, pkg, gpu_ctx, what):
    I = K.inputs(pkg, SECONDS, seed=46)
    trig = T.trigger_configs(4) + [{"long_term_speech_avg_sec": 300.0, "initial_long_term_avg": 0.01, "speech_threshold_factor": 4.0}]
    cfgs = T.grid(trig, T.FINISH[:4])   # 5 keys x 4; key 4 alone has the 300 s window (14062 slots)
    keep = {"whole keys": [c for c in range(20) if c % 5 in (1, 3)], "parts of keys": [0, 1, 7, 8, 13, 19],
            "representative": [2, 3, 5, 6, 10, 11, 12], "long window": [c for c in range(20) if c % 5 != 4]}[what]
    kept = [cfgs[c] for c in keep]
    S = len(SECONDS)
    with shared(gpu_ctx):
        sw = run_parts(fv, gpu_ctx, I, cfgs, SECONDS, CUTS, retain_at=1, keep=keep)
        fresh = fv.VadSweep(S, kept)
        assert sw.trigger_form() == 2 and sw.trigger_keys() == fresh.trigger_keys()
        fresh.close()
        sw.score(4)
        got = snapshot(sw, S, len(kept))
        sw.close()
        a = run_parts(fv, gpu_ctx, I, kept, SECONDS, CUTS)   # a fresh shared batch of the survivors
        a.score(4)
        assert_same(snapshot(a, S, len(kept)), got, (what, "fresh shared"))
        a.close()
    with options(gpu_ctx, vad_chain="coop"):
        b = run_parts(fv, gpu_ctx, I, kept, SECONDS, CUTS)   # and a per-config one
        assert b.trigger_form() == 1
        b.score(4)
        assert_same(snapshot(b, S, len(kept)), got, (what, "per config"))
        b.close()
    assert_oracle(got, K.oracle(I, kept), what)


def test_rule_and_form(fv, pkg, gpu_ctx):
    ctx = gpu_ctx
    I = K.inputs(pkg, SECONDS, seed=47)
    cfgs = GRID8[:32]
    S, NC = len(SECONDS), len(cfgs)
    with shared(ctx):
        ref = one_shot(fv, ctx, I, cfgs, SECONDS)
        want = snapshot(ref, S, NC)
        need = ref.trigger_bytes()
        ref.close()
    assert need == 2 * 30 * 8 * 8   # 2 streams x 30 words (rows as long as the longest stream) x 8 keys x 8 bytes
    with options(ctx, vad_trigger="shared"):   # without coop: the per-config lane form
        sw = one_shot(fv, ctx, I, cfgs, SECONDS)
        assert sw.trigger_form() == 1 and sw.chain_form() == 1
        assert_same(snapshot(sw, S, NC), want, "no coop")
        sw.close()
    with shared(ctx, vad_trigger_max_bytes=str(need - 1)):   # the bits do not fit: per-config machines
        sw = one_shot(fv, ctx, I, cfgs, SECONDS)
        assert sw.trigger_form() == 1 and sw.trigger_bytes() == 0
        assert_same(snapshot(sw, S, NC), want, "budget")
        sw.close()
    with shared(ctx, vad_trigger_max_bytes=str(need)):
        sw = one_shot(fv, ctx, I, cfgs, SECONDS)
        assert sw.trigger_form() == 2
        sw.close()
    for first, form in (("shared", 2), ("config", 1)):   # the option changed mid-run: the run keeps its form
        with options(ctx, vad_chain="coop", vad_trigger=first):
            sw = run_parts(fv, ctx, I, cfgs, SECONDS, CUTS, flip_at=1)
            assert sw.trigger_form() == form
            sw.score(4)
            got = snapshot(sw, S, NC)
            assert_same(got, {k: want[k] for k in ("segs", "audit", "lazy")}, ("flip", first))
            sw.close()
    for name, bad in (("vad_trigger", "keys"), ("vad_trigger_max_bytes", "-1")):
        with pytest.raises(fv.FvadError):
            ctx.set_option(name, bad)


def test_run_grid(fv, pkg, gpu_ctx, tmp_path, monkeypatch):
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, ((2, "f32", 32.0), (1, "pcm16", 24.5)))
    grid = {"base": {"long_term_speech_avg_sec": 4.0},
            "axes": {"speech_threshold_factor": [2.0, 3.0, 4.0, 6.0], "min_consecutive_sec_to_open": [0.0, 0.1],
                     "max_speech_gap_sec": [0.1, 0.5], "min_vad_duration_sec": [0.0, 0.3]}}
    with pytest.raises(ValueError):
        sim.run_grid(plan, grid, ctx=gpu_ctx, out=None, vad_trigger="shared")
    with pytest.raises(ValueError):
        sim.run_grid(plan, grid, ctx=gpu_ctx, out=None, vad_chain="coop", vad_trigger="key")
    modes = {"unsliced": {}, "sliced": {"slice_chunks": 16}, "halving": {"slice_chunks": 16, "halving_eta": 2, "halving_rungs": 1},
             "overlap": {"slice_chunks": 16, "overlap": True},
             # two contexts that run_grid makes and closes itself (the synthetic weights of gpu_ctx, reproducible from the environment,
             # which a context reads when it is made): one instance each
             "devices": {"slice_chunks": 16, "ctx": None, "devices": [0, 0], "synth_seed": 7}}
    monkeypatch.setenv("FVAD_REPRODUCIBLE", "1")
    gpu_ctx.set_option("reproducible", "1")
    try:
        first = None
        for name, kw in modes.items():
            kw = dict({"ctx": gpu_ctx}, **kw)
            res = {t: sim.run_grid(plan, grid, out=None, vad_on="device", score_on="device", vad_chain="coop",
                                   vad_trigger=t, json_path=str(tmp_path / f"{t}.json"), **kw) for t in ("config", "shared")}
            assert res["config"]["times"]["trigger_form"] == 1 and res["shared"]["times"]["trigger_form"] == 2, name
            assert res["shared"]["times"]["trigger_keys"] == 4 and res["shared"]["times"]["trigger_bytes"] > 0, name
            a, b = np.asarray(res["shared"]["stats"], np.float32), np.asarray(res["config"]["stats"], np.float32)
            assert a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all(), name
            if name != "halving":   # (halving scores its losers on part of the streams) reproducible contexts: every mode's statistics
                first = a if first is None else first
                assert (a.view(np.uint32) == first.view(np.uint32)).all(), name
            if name == "devices":
                assert [t["instances"] for t in res["shared"]["share_times"]] == [[0], [1]]
                assert all(t["times"]["trigger_form"] == 2 and t["times"]["trigger_keys"] == 4 for t in res["shared"]["share_times"])
            doc = json.load(open(tmp_path / "shared.json"))
            assert doc["trigger_keys"] == 4 and doc["trigger_form"] == 2
    finally:
        gpu_ctx.set_option("reproducible", None)
    assert gpu_ctx.option_set("vad_trigger") is None
