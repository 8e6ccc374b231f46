"""Scoring on the GPU (kernels_eval.hip): the device statistics of every (stream, config) machine against the host scorer
fvad_vad_batch_score bit for bit -- both lane mappings, the overflow relaunch, a two-hour stream, keep_segments 0 -- and
simulator.run_grid against itself (device / host scoring) and against run_sweep."""
import json

import numpy as np
import pytest

from test_harness import write_wav
from test_vad_score_host import make_labels, stat_cfgs_of
from test_vad_sweep_gpu import sweep_configs
from test_vad_sweep_host import CHUNK, FS, synth_inputs

pytestmark = pytest.mark.gpu


def device_run(fv, ctx, cfgs, n_chunks, nch, seed, keep=True):
    """one device sweep over ragged streams with references set: (VadSweep, refs, stat configs)"""
    S = len(n_chunks)
    sw = fv.VadSweep(S, cfgs, n_channels=nch)
    bins, _ = sw.bands()
    band, rms = synth_inputs(S, nch, max(n_chunks), bins, seed)
    rng = np.random.default_rng(seed)
    refs = [make_labels(rng, k * CHUNK / FS, max(2, int(k * CHUNK / FS / 6)), "empty" if s == 2 else "mixed")
            for s, k in enumerate(n_chunks)]
    scs = stat_cfgs_of(cfgs, seed)
    sw.set_references(refs, scs)
    sw.keep_segments(keep)
    d_band = ctx.device_alloc(band.nbytes)
    try:
        ctx.to_device(d_band, band)
        sw.run_device(ctx, d_band, band.shape[2], [k * CHUNK // 1024 for k in n_chunks], rms, n_chunks)
    finally:
        ctx.device_free(d_band)
    return sw, refs, scs


def all_stats(sw, n_configs):
    return np.stack([sw.config_stats(c) for c in range(n_configs)])


def host_scores(sw, n_configs):
    """the host scorer over the segments the device run brought back"""
    sw.score(16)
    return all_stats(sw, n_configs)


def assert_bits(a, b):
    assert a.shape == b.shape
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert bad.size == 0, (bad[:5], a[tuple(bad[0][:2])], b[tuple(bad[0][:2])])


N_CHUNKS = [200, 40, 120, 8, 160, 64, 1, 96]   # ragged, stream 2 without labels


def test_device_scores_equal_host_scorer(fv, gpu_ctx):
    ctx = gpu_ctx
    cfgs = sweep_configs(64, seed=3)
    sw, refs, scs = device_run(fv, ctx, cfgs, N_CHUNKS, 2, seed=21)
    dev = all_stats(sw, len(cfgs))
    assert sum(len(x) for c in range(len(cfgs)) for x in sw.segments(c)) > 500
    assert_bits(dev, host_scores(sw, len(cfgs)))
    # the other lane mapping of the machines: the same machines, the same scores
    ctx.set_option("vad_lane_map", "config")
    try:
        sw2, _, _ = device_run(fv, ctx, cfgs, N_CHUNKS, 2, seed=21)
        assert_bits(all_stats(sw2, len(cfgs)), dev)
        assert_bits(host_scores(sw2, len(cfgs)), dev)
    finally:
        ctx.set_option("vad_lane_map", None)
    # the overflow path: the scores are of the second launch's segments
    ctx.set_option("vad_seg_cap", "2")
    try:
        sw3, _, _ = device_run(fv, ctx, cfgs, N_CHUNKS, 2, seed=21)
        assert_bits(all_stats(sw3, len(cfgs)), dev)
        assert_bits(host_scores(sw3, len(cfgs)), dev)
    finally:
        ctx.set_option("vad_seg_cap", None)


def test_keep_segments_off(fv, gpu_ctx):
    cfgs = sweep_configs(64, seed=3)
    ref_sw, _, _ = device_run(fv, gpu_ctx, cfgs, N_CHUNKS, 2, seed=21)
    sw, _, _ = device_run(fv, gpu_ctx, cfgs, N_CHUNKS, 2, seed=21, keep=False)
    assert_bits(all_stats(sw, len(cfgs)), all_stats(ref_sw, len(cfgs)))
    for s in range(len(N_CHUNKS)):   # audits and lazy statistics still come back
        for c in (0, 1, 63):
            assert sw.audit(s, c) == ref_sw.audit(s, c) and sw.lazy_stats(s, c) == ref_sw.lazy_stats(s, c)
    lib = fv.lib()
    offs = (fv.sz * (len(N_CHUNKS) + 1))()
    assert lib.fvad_vad_batch_config_segments(sw.h, 0, None, 0, offs) == fv.FVAD_ERR_INVALID_ARGUMENT
    assert lib.fvad_vad_batch_segments(sw.h, None, 0, offs) == fv.FVAD_ERR_INVALID_ARGUMENT
    assert lib.fvad_vad_batch_total_segments(sw.h) == 2 ** 64 - 1
    assert lib.fvad_vad_batch_score(sw.h, 4) == fv.FVAD_ERR_INVALID_ARGUMENT   # no segments to score on the host
    with pytest.raises(fv.FvadError):
        sw.segments(0)


def test_two_hour_stream_device_scores(fv, gpu_ctx):
    cfgs = sweep_configs(16, seed=8)
    sw, _, _ = device_run(fv, gpu_ctx, cfgs, [14400], 2, seed=33)
    assert max(x[1] for c in range(len(cfgs)) for x in sw.segments(c)[0]) > 1 << 24
    assert_bits(all_stats(sw, len(cfgs)), host_scores(sw, len(cfgs)))


def write_plan(pkg, tmp_path, streams):
    synth = pkg.synth
    insts = []
    for i, (nch, fmt, sec) in enumerate(streams):
        pcm, labels = synth.make_stream(sec, seed=500 + i, n_channels=nch)
        write_wav(str(tmp_path / f"s{i}.wav"), pcm, fmt=fmt)
        (tmp_path / f"s{i}.txt").write_text(synth.labels_to_audacity(labels))
        insts.append({"name": f"stream{i}", "audio_path": f"s{i}.wav", "ref_path": f"s{i}.txt"})
    plan = {"instances": insts, "config": {"vad_config": {"vad_machine_config": {"speech_threshold_factor": 7}}}}
    (tmp_path / "plan.json").write_text(json.dumps(plan))
    return str(tmp_path / "plan.json")


def rows_bits(rows):
    return [tuple(np.float32(r[k]).view(np.uint32) for k in ("P", "TP", "FP", "FN", "TPR", "PPV", "FNR", "FDR", "F", "FM"))
            for r in rows]


def test_run_grid_device_host_and_run_sweep(pkg, gpu_ctx, tmp_path):
    ctx = gpu_ctx
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, ((1, "f32", 70.0), (2, "pcm16", 45.0), (1, "pcm16", 30.5)))
    grid = {"base": {"max_speech_gap_sec": 2.0},
            "axes": {"speech_threshold_factor": [5, 7, 10], "speech_min_freq": [300, 500], "initial_long_term_avg": [None, 0.005]}}
    ctx.set_option("reproducible", "1")
    try:
        dev = sim.run_grid(plan, grid, ctx=ctx, out=None, vad_on="device", score_on="device", json_path=str(tmp_path / "g.json"))
        host = sim.run_grid(plan, grid, ctx=ctx, out=None, vad_on="device", score_on="host")
        hh = sim.run_grid(plan, grid, ctx=ctx, out=None, vad_on="host", score_on="host")
        sweep = sim.run_sweep(plan, ctx=ctx, configs=dev["configs"], out=None)
        # a grid that holds the plan's own config (speech_threshold_factor 7) and run_sweep's default: the plan's configs
        assert not ctx.timing                     # run_grid left the kernel timing as it found it: off
        # a caller with kernel timing on keeps it on, and its records (run_grid's kernels among them) are not drained
        ctx.enable_timing(True)
        try:
            own = sim.run_grid(plan, {"axes": {"speech_threshold_factor": [5, 7]}}, ctx=ctx, out=None, vad_on="device",
                               score_on="device")
            assert ctx.timing
            kt = ctx.kernel_times()
            assert "vad_machines" in kt and "vad_score" in kt
        finally:
            ctx.enable_timing(False)
        plan_sweep = sim.run_sweep(plan, ctx=ctx, out=None)
    finally:
        ctx.set_option("reproducible", None)
    assert len(dev["rows"]) == 12
    assert rows_bits(dev["rows"]) == rows_bits(host["rows"]) == rows_bits(hh["rows"])
    assert np.array_equal(dev["stats"].view(np.uint32), hh["stats"].view(np.uint32))
    # the grid's configs through run_sweep (per-segment scoring): the same rows and per-instance stats
    assert rows_bits(dev["rows"]) == rows_bits(sweep["rows"])
    for c in range(12):
        for i in range(3):
            assert np.array_equal(dev["stats"][c, i].view(np.uint32), fv_stats_bits(pkg, sweep["stats"][c][i]))
    assert sum(len(x) for per in sweep["segments"] for x in per) > 0
    assert len(plan_sweep["rows"]) == 1 and rows_bits(own["rows"][1:]) == rows_bits(plan_sweep["rows"])
    saved = json.load(open(tmp_path / "g.json"))
    assert len(saved["rows"]) == 12 and saved["configs"] == dev["configs"]


def fv_stats_bits(pkg, s):
    return pkg.binding.single_stats_to_array(s).view(np.uint32)


def test_run_grid_thousands_of_configs(pkg, gpu_ctx, tmp_path, capsys):
    ctx = gpu_ctx
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, ((1, "f32", 40.0), (2, "pcm16", 25.0)))
    grid = {"axes": {"speech_threshold_factor": [3, 4, 5, 6, 7, 8, 10, 12], "short_term_speech_avg_sec": [0.1, 0.2, 0.3, 0.5],
                     "max_speech_gap_sec": [0.5, 1.0, 2.0, 3.0], "min_vad_duration_sec": [0.3, 0.7],
                     "speech_min_freq": [300, 500, 800, 1000]}}
    ctx.set_option("reproducible", "1")
    try:
        dev = sim.run_grid(plan, grid, ctx=ctx, out=None, json_path=str(tmp_path / "g.json"))   # auto: device machines and scoring
        host = sim.run_grid(plan, grid, ctx=ctx, out=None, vad_on="device", score_on="host")
    finally:
        ctx.set_option("reproducible", None)
    assert len(dev["rows"]) == 1024
    assert rows_bits(dev["rows"]) == rows_bits(host["rows"])
    with capsys.disabled():
        print(f"\n1024-config grid: device {dev['times']}, host scoring {host['times']}")
