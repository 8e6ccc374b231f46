"""simulator.run_grid over several contexts on one MI355X: share lists of caller-owned contexts (reproducible = 1) against
the single context, bit for bit -- stats, rows, JSON and the printed table -- unsliced with device and with host machines,
sliced, on a sized grid and with successive halving; uneven shares (a share of one channel count, a share whose instances
end before the first rung, an empty share); a share that fails mid-run; the default mode; owned contexts from devices."""
import io
import json
import math
import re
import threading

import numpy as np
import pytest

from test_vad_retain_gpu import GRID
from test_vad_score_gpu import rows_bits, write_plan

pytestmark = pytest.mark.gpu

# mono and stereo, PCM16 and f32, different lengths (test_vad_retain_gpu's STREAMS, the third one shortened: 12 chunks, so
# that with three contexts its share ends before the first rung at chunk 32)
STREAMS = [(1, "pcm16", 47.3), (2, "f32", 61.1), (1, "f32", 6.2), (2, "pcm16", 20.2)]
SIZED = dict(GRID, fft_size=[512, 2048])


@pytest.fixture
def contexts(fv, gpu_ctx):
    """gpu_ctx and four more contexts on device 0 (synthetic weights, seed 7), all reproducible; returns a function of how
    many to use"""
    extra = []
    try:
        for _ in range(4):
            c = fv.Context(0)
            extra.append(c)
            c.load_synth(7)
        for c in [gpu_ctx] + extra:
            c.set_option("reproducible", "1")
        yield lambda n: [gpu_ctx] + extra[:n - 1]
    finally:
        gpu_ctx.set_option("reproducible", None)
        for c in extra:
            c.close()


def timing_free(text):
    """the printed table without its timings: every "<number> s" of the bracketed lines, and the shares' wall times"""
    out = []
    for line in text.splitlines():
        if line.startswith("["):
            line = re.sub(r"; shares' wall times [^\]]*", "", line)
            line = re.sub(r"\d+\.\d+ s", "T s", line)
        out.append(line)
    return out


def json_doc(path):
    doc = json.loads(open(path).read())
    for g in doc.get("rung_times", []):
        g.pop("seconds")
    return doc


def run(sim, plan, grid, ctx, tmp_path, name, **kw):
    buf = io.StringIO()
    r = sim.run_grid(plan, grid, ctx=ctx, out=buf, json_path=str(tmp_path / f"{name}.json"), top=100, **kw)
    return r, buf.getvalue(), json_doc(tmp_path / f"{name}.json")


def assert_same(one, many, halving=False):
    (r1, t1, j1), (rn, tn, jn) = one, many
    assert np.array_equal(rn["stats"].view(np.uint32), r1["stats"].view(np.uint32))
    assert rows_bits(rn["rows"]) == rows_bits(r1["rows"])
    assert [{k: v for k, v in r.items() if k not in ("P", "TP", "FP", "FN", "TPR", "PPV", "FNR", "FDR", "F", "FM")}
            for r in rn["rows"]] == [{k: v for k, v in r.items() if k not in ("P", "TP", "FP", "FN", "TPR", "PPV", "FNR", "FDR",
                                                                            "F", "FM")} for r in r1["rows"]]
    assert json.dumps(jn, sort_keys=True) == json.dumps(j1, sort_keys=True)
    assert timing_free(tn) == timing_free(t1)
    if halving:
        for k in ("survivors", "rung", "evaluated_seconds"):
            assert rn[k] == r1[k], k
        assert [(g["rung"], g["end_chunk"], g["configs_in"], g["configs_kept"]) for g in rn["rung_times"]] == \
               [(g["rung"], g["end_chunk"], g["configs_in"], g["configs_kept"]) for g in r1["rung_times"]]


CASES = {
    "unsliced device": (GRID, dict(vad_on="device", score_on="device")),
    "unsliced host": (GRID, dict(vad_on="host", score_on="host")),
    "sliced": (GRID, dict(vad_on="device", score_on="device", slice_chunks=16)),
    "sized": (SIZED, dict(vad_on="device", score_on="device", slice_chunks=32)),
    "halving": (GRID, dict(vad_on="device", score_on="device", slice_chunks=16, halving_eta=2, halving_rungs=2)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_two_contexts_equal_one(pkg, contexts, tmp_path, case):
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, STREAMS)
    grid, kw = CASES[case]
    ctxs = contexts(2)
    one = run(sim, plan, grid, ctxs[0], tmp_path, "one", **kw)
    two = run(sim, plan, grid, ctxs, tmp_path, "two", **kw)
    assert_same(one, two, halving="halving_eta" in kw)
    r = two[0]
    assert [t["instances"] for t in r["share_times"]] == [[0, 2], [1, 3]]
    assert [t["device"] for t in r["share_times"]] == [0, 0]
    assert "shares' wall times" in two[1] and "shares' wall times" not in one[1]
    if "slice_chunks" in kw:
        assert r["device_bytes"] == max(r["device_bytes_per_share"]) > 0
    else:
        assert r["device_bytes"] is None and r["device_bytes_per_share"] == [None, None]
    assert set(r["times"]) == set(one[0]["times"])


@pytest.mark.parametrize("n_ctx", [3, 5])
def test_uneven_shares_equal_one(pkg, contexts, tmp_path, n_ctx):
    """three contexts: shares [0, 3] (mono and stereo), [1] (stereo only), [2] (12 chunks: ended before the first rung at
    chunk 32); five: one share per instance and an empty one"""
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, STREAMS)
    ctxs = contexts(n_ctx)
    grid, kw = CASES["halving"]
    assert sim.halving_schedule(122, 16, 2, 2)[0] == 32
    one = run(sim, plan, grid, ctxs[0], tmp_path, "one", **kw)
    many = run(sim, plan, grid, ctxs, tmp_path, "many", **kw)
    assert_same(one, many, halving=True)
    shares = [t["instances"] for t in many[0]["share_times"]]
    assert shares == ([[0, 3], [1], [2]] if n_ctx == 3 else [[0], [1], [2], [3], []])
    if n_ctx == 5:
        assert many[0]["device_bytes_per_share"][4] is None and many[0]["share_times"][4]["wall"] == 0.0
        # unsliced, too
        grid, kw = CASES["unsliced device"]
        assert_same(run(sim, plan, grid, ctxs[0], tmp_path, "one_u", **kw), run(sim, plan, grid, ctxs, tmp_path, "many_u", **kw))


def test_a_failing_share(fv, pkg, contexts, tmp_path, monkeypatch):
    """a Python exception in one share's third device part (before the library is called): run_grid raises it, leaves no
    thread behind, and gpu_ctx -- the failing share's context -- runs the next grid"""
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, STREAMS)
    ctxs = contexts(2)
    victim = ctxs[0]
    real = fv.VadSweep.run_device_part_sized
    n = {"victim": 0}

    def part(self, ctx, *a, **k):
        if ctx is victim:
            n["victim"] += 1
            if n["victim"] == 3:
                raise RuntimeError("injected failure in a share")
        return real(self, ctx, *a, **k)

    grid, kw = CASES["halving"]
    before = set(threading.enumerate())
    monkeypatch.setattr(fv.VadSweep, "run_device_part_sized", part)
    with pytest.raises(RuntimeError, match="injected failure"):
        sim.run_grid(plan, grid, ctx=ctxs, out=None, **kw)
    monkeypatch.undo()
    assert set(threading.enumerate()) == before
    assert n["victim"] == 3
    after = sim.run_grid(plan, grid, ctx=victim, out=None, **kw)
    assert len(after["survivors"]) == math.ceil(math.ceil(len(after["configs"]) / 2) / 2)


def test_default_mode_completes(fv, pkg, gpu_ctx, tmp_path):
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, STREAMS)
    other = fv.Context(0)
    try:
        other.load_synth(7)
        r = sim.run_grid(plan, GRID, ctx=[gpu_ctx, other], out=None, vad_on="device", score_on="device", slice_chunks=16,
                         halving_eta=2, halving_rungs=2)
    finally:
        other.close()
    NC = len(r["configs"])
    assert len(r["survivors"]) == math.ceil(math.ceil(NC / 2) / 2)
    assert [c for c in range(NC) if r["rung"][c] is None] == r["survivors"]


def test_owned_contexts_from_devices(pkg, tmp_path):
    """devices=[0, 0]: two contexts made (synthetic weights) and closed by run_grid"""
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, STREAMS)
    r = sim.run_grid(plan, GRID, devices=[0, 0], synth_seed=7, out=None, vad_on="device", score_on="device", slice_chunks=16)
    assert len(r["rows"]) == 16 and r["stats"].shape == (16, 4, 11)
    assert [(t["device"], t["instances"]) for t in r["share_times"]] == [(0, [0, 2]), (0, [1, 3])]
    assert r["slices"] > 0 and all(t["wall"] > 0 for t in r["share_times"])
