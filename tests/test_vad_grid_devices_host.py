"""simulator.run_grid over several contexts, without a GPU: the ctx / devices argument rules (before any context is made),
instance_shares against run_plan's deal, the CLI's --devices for --sweep-grid, and the share workers' coordination --
plan-order stats, per-share results, successive halving's rungs across shares, and a failing share -- with the per-share
flow (_grid_share) replaced by a stand-in that writes known statistics."""
import io
import json
import threading
import time

import numpy as np
import pytest

from test_harness import write_wav

GRID = {"axes": {"speech_threshold_factor": [2.0, 3.0, 5.0, 8.0], "min_vad_duration_sec": [0.3, 0.7]}}
STREAMS = [(1, "pcm16", 30.0), (2, "f32", 40.3), (1, "f32", 6.2), (2, "pcm16", 21.1), (1, "pcm16", 33.0)]
N_CHUNKS = [int(round(sec * 48000)) // 24000 for _, _, sec in STREAMS]   # 60, 80, 12, 42, 66


@pytest.fixture(scope="module")
def sim(pkg):
    return pkg.simulator


def write_plan(pkg, d, streams=STREAMS):
    insts = []
    for i, (nch, fmt, sec) in enumerate(streams):
        pcm, labels = pkg.synth.make_stream(sec, seed=900 + i, n_channels=nch)
        write_wav(str(d / f"s{i}.wav"), pcm, fmt=fmt)
        (d / f"s{i}.txt").write_text(pkg.synth.labels_to_audacity(labels))
        insts.append({"name": f"stream{i}", "audio_path": f"s{i}.wav", "ref_path": f"s{i}.txt"})
    (d / "plan.json").write_text(json.dumps({"instances": insts}))
    return str(d / "plan.json")


def fake_ctx(fv, device=0):
    """a Context object that holds no library context (nothing is run on it here)"""
    c = fv.Context.__new__(fv.Context)
    c.h = fv.vp()
    c.device = device
    return c


@pytest.fixture
def no_context(fv, monkeypatch):
    def fail(self, *a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(fv.Context, "__init__", fail)


@pytest.mark.parametrize("kw,words", [
    (dict(devices=[0], ctx="CTX"), "not both"),
    (dict(devices=[]), "non-empty"),
    (dict(devices=()), "non-empty"),
    (dict(devices=0), "non-empty"),
    (dict(devices=[0, -1]), "device index"),
    (dict(devices=[0, 1.0]), "device index"),
    (dict(devices=["0"]), "device index"),
    (dict(devices=[True]), "device index"),
    (dict(ctx=[]), "not empty"),
    (dict(ctx=[object()]), "not a Context"),
    (dict(ctx=("CTX", None)), "not a Context"),
    (dict(ctx=["CTX", 0]), "not a Context"),
    (dict(ctx=["CTX", "CTX"]), "twice"),
])
def test_argument_errors_before_any_context(fv, sim, pkg, tmp_path, no_context, kw, words):
    plan = write_plan(pkg, tmp_path)
    c = fake_ctx(fv)
    kw = {k: ([c if x == "CTX" else x for x in v] if isinstance(v, list) else
              tuple(c if x == "CTX" else x for x in v) if isinstance(v, tuple) else c if v == "CTX" else v)
          for k, v in kw.items()}
    with pytest.raises(ValueError, match=words):
        sim.run_grid(plan, GRID, out=None, **kw)


def test_instance_shares_deal_like_run_plan(fv, sim, pkg, tmp_path, monkeypatch):
    for n in range(0, 12):
        for d in range(1, 10):
            shares = sim.instance_shares(n, d)
            assert len(shares) == d
            assert sorted(i for s in shares for i in s) == list(range(n))
            assert all(i % d == k for k, s in enumerate(shares) for i in s) and all(s == sorted(s) for s in shares)
    # run_plan's own deal, seen through the instances each of its contexts gets
    plan = write_plan(pkg, tmp_path)
    lengths = [int(round(sec * 48000)) for _, _, sec in STREAMS]
    got = {}
    lock = threading.Lock()

    def run_instances(ctx, plan_, audio):
        with lock:
            got[ctx.device] = [lengths.index(a.shape[1]) for a in audio]
        return [([], None) for _ in audio]

    monkeypatch.setattr(sim, "_make_ctx", lambda plan_, device, seed: fake_ctx(fv, device))
    monkeypatch.setattr(sim, "_run_instances", run_instances)
    sim.run_plan(plan, out=None, devices=[0, 1, 2])
    assert [got[d] for d in range(3)] == sim.instance_shares(len(STREAMS), 3) == [[0, 3], [1, 4], [2]]


def test_cli_devices_reach_run_grid(sim, pkg, tmp_path, monkeypatch):
    plan = write_plan(pkg, tmp_path)
    grid = tmp_path / "grid.json"
    grid.write_text(json.dumps(GRID))
    calls = []
    monkeypatch.setattr(sim, "run_grid", lambda *a, **k: calls.append(("grid", a, k)))
    monkeypatch.setattr(sim, "run_sweep", lambda *a, **k: calls.append(("sweep", a, k)))
    sim.main(["-i", plan, "--sweep-grid", str(grid), "--devices", "0,1"])
    sim.main(["-i", plan, "--sweep-grid", str(grid)])
    sim.main(["-i", plan, "--sweep", "--devices", "0,1"])
    assert [c[0] for c in calls] == ["grid", "grid", "sweep"]
    assert calls[0][2]["devices"] == [0, 1]
    assert calls[1][2]["devices"] is None          # no --devices: the single-context path
    assert "devices" not in calls[2][2]             # --sweep stays on device 0


# ------------------------------------------------------------------ the share workers, with a stand-in per-share flow

def known_stats(NC, n_inst):
    """stats[config][instance]: distinct F-scores per config, P = 100 s everywhere"""
    s = np.zeros((NC, n_inst, 11), np.float32)
    for c in range(NC):
        for i in range(n_inst):
            tp = np.float32(20 + (37 * c + 11 * i) % 71)
            s[c, i, :4] = (100, tp, 100 - tp, 100 - tp)
            s[c, i, 10] = 0.7
    return s


def stand_in(sim, calls, fail_share=None, halting=None):
    """a _grid_share that records its arguments and writes known_stats into its instances' columns; with rungs it takes part
    in every rung as the real one does.  fail_share: the share (by its first instance) that raises at its first rung or, with
    halting set, at once while the others wait for the stop"""
    def share(ctx, job, audio, refs, ids, stats, times, rungs, stop):
        configs, slice_chunks, n_threads = job.configs, job.slice_chunks, job.n_threads
        calls.append({"device": ctx.device, "ids": list(ids), "n_threads": n_threads, "thread": threading.current_thread(),
                      "n_audio": len(audio)})
        want = known_stats(len(configs), stats.shape[1])
        if halting is not None:
            if ids[0] == fail_share:
                time.sleep(0.05)
                raise RuntimeError("share failed")
            for _ in range(500):   # stopped at its next "slice"
                sim._check_stop(stop)
                time.sleep(0.01)
            raise AssertionError("the other share was not stopped")
        if rungs is None:
            stats[:, ids] = want[:, ids]
            times["machines"] += 1.0
            return 1, None if slice_chunks is None else 1000 + int(ids[0])
        for s0 in range(0, rungs.K, slice_chunks):
            s1 = min(s0 + slice_chunks, rungs.K)
            rungs.count(ids, s0, s1)
            if s1 in rungs.ends:
                if ids[0] == fail_share:
                    raise RuntimeError("share failed")
                for c, o in enumerate(rungs.alive):
                    stats[o, ids] = want[o, ids] + np.float32(len(rungs.log))
                rungs.wait(rungs.choose)
                rungs.wait(rungs.logged)
        for o in rungs.alive:
            stats[o, ids] = want[o, ids]
        rungs.wait(rungs.ended)
        return 2, 500 + int(ids[0])
    return share


@pytest.fixture
def shares_stubbed(sim, fv, monkeypatch):
    calls = []

    def install(**kw):
        monkeypatch.setattr(sim, "_grid_share", stand_in(sim, calls, **kw))
        return calls
    monkeypatch.setattr(sim, "_make_ctx", lambda plan_, device, seed: fake_ctx(fv, device))
    return install


def test_shares_fill_plan_order(fv, sim, pkg, tmp_path, shares_stubbed):
    plan = write_plan(pkg, tmp_path)
    calls = shares_stubbed()
    one = sim.run_grid(plan, GRID, out=None, ctx=fake_ctx(fv), vad_on="host")
    assert len(calls) == 1 and calls[0]["thread"] is threading.main_thread() and calls[0]["n_threads"] == 16
    assert "share_times" not in one and "device_bytes_per_share" not in one
    calls.clear()
    before = set(threading.enumerate())
    three = sim.run_grid(plan, GRID, out=None, devices=[0, 1, 0], vad_on="host", n_threads=16, json_path=str(tmp_path / "g.json"))
    assert set(threading.enumerate()) == before
    assert sorted((c["device"], c["ids"]) for c in calls) == [(0, [0, 3]), (0, [2]), (1, [1, 4])]
    assert all(c["n_threads"] == 5 and c["thread"] is not threading.main_thread() for c in calls)
    assert np.array_equal(three["stats"].view(np.uint32), one["stats"].view(np.uint32))
    assert [r["F"] for r in three["rows"]] == [r["F"] for r in one["rows"]]
    assert [(t["device"], t["instances"]) for t in three["share_times"]] == [(0, [0, 3]), (1, [1, 4]), (0, [2])]
    assert three["times"]["machines"] == 3.0 and three["slices"] == 3
    assert three["device_bytes"] is None and three["device_bytes_per_share"] == [None] * 3
    # five shares over five instances, then seven: the empty shares make no context and do no work
    calls.clear()
    seven = sim.run_grid(plan, GRID, out=None, devices=list(range(7)), vad_on="device", slice_chunks=16)
    assert sorted(c["device"] for c in calls) == [0, 1, 2, 3, 4]
    assert seven["device_bytes_per_share"] == [1000, 1001, 1002, 1003, 1004, None, None]
    assert seven["device_bytes"] == 1004
    assert seven["share_times"][5] == {"device": 5, "instances": [], "wall": 0.0, "times": {}}
    assert np.array_equal(seven["stats"].view(np.uint32), one["stats"].view(np.uint32))


def test_halving_rungs_across_shares(fv, sim, pkg, tmp_path, shares_stubbed):
    plan = write_plan(pkg, tmp_path)
    calls = shares_stubbed()
    kw = dict(vad_on="device", score_on="device", slice_chunks=16, halving_eta=2, halving_rungs=2)
    buf = io.StringIO()
    one = sim.run_grid(plan, GRID, ctx=fake_ctx(fv), out=buf, **kw)
    out_one = buf.getvalue()
    # rungs at chunks 32 and 48 of 80; instance 2 (12 chunks) ends before the first, alone in share 2 of [0, 1, 2]
    assert [g["end_chunk"] for g in one["rung_times"]] == [32, 48, 80]
    assert [(g["configs_in"], g["configs_kept"]) for g in one["rung_times"]] == [(8, 4), (4, 2), (2, 2)]
    for devs in ([0, 0], [0, 1, 2], list(range(6))):
        calls.clear()
        buf = io.StringIO()
        many = sim.run_grid(plan, GRID, devices=devs, out=buf, **kw)
        out_many = buf.getvalue()
        for k in ("survivors", "rung", "evaluated_seconds"):
            assert many[k] == one[k], (devs, k)
        assert [(g["rung"], g["end_chunk"], g["configs_in"], g["configs_kept"]) for g in many["rung_times"]] == \
               [(g["rung"], g["end_chunk"], g["configs_in"], g["configs_kept"]) for g in one["rung_times"]]
        assert np.array_equal(many["stats"].view(np.uint32), one["stats"].view(np.uint32))
        assert many["slices"] == 2 * len(calls)
        # the table is the same; the summary line adds the shares' wall times
        assert [x for x in out_many.splitlines() if not x.startswith("[")] == \
               [x for x in out_one.splitlines() if not x.startswith("[")]
        assert "shares' wall times" in out_many and "shares' wall times" not in out_one
    assert one["evaluated_seconds"][one["survivors"][0]] == sum(N_CHUNKS) * 0.5


@pytest.mark.parametrize("halting", [False, True])
def test_a_failing_share_stops_the_others(fv, sim, pkg, tmp_path, shares_stubbed, halting):
    """the share of instance 1 raises: at its first rung while the others wait at the barrier, or at once while another one
    runs slices; run_grid raises its exception and leaves no thread behind"""
    plan = write_plan(pkg, tmp_path)
    calls = shares_stubbed(fail_share=1, halting=True if halting else None)
    before = set(threading.enumerate())
    with pytest.raises(RuntimeError, match="share failed"):
        sim.run_grid(plan, GRID, out=None, devices=[0, 0, 0], vad_on="device", score_on="device", slice_chunks=16,
                      halving_eta=2, halving_rungs=2)
    assert set(threading.enumerate()) == before
    assert len(calls) == 3
