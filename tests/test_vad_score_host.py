"""Scoring a VAD batch on the host (fvad_vad_batch_set_references / _score / _config_stats): every machine's statistics bit for
bit fvad_stats_from_segments of its converted segments and its stream's labels, on label sets built to hit the walk's edges; the
argument checks; simulator.expand_grid / run_grid's grid validation.  No GPU needed."""
import ctypes as C
import json

import numpy as np
import pytest

from test_vad_sweep_host import CHUNK, CONFIGS, FS, synth_inputs

STAT = {"extrude_start": 5.0, "extrude_end": 10.0, "fill_gaps": 5.0}


def score_configs(n, seed):
    """n configs around CONFIGS; the last one never opens (a machine with no segments)"""
    rng = np.random.default_rng(seed)
    out = [dict(c) for c in CONFIGS]
    while len(out) < n - 1:
        c = dict(CONFIGS[int(rng.integers(len(CONFIGS)))])
        c["speech_threshold_factor"] = float(rng.uniform(1.5, 6.0))
        c["min_vad_duration_sec"] = float(rng.uniform(0.0, 1.0))
        c["max_speech_gap_sec"] = float(rng.uniform(0.0, 3.0))
        out.append(c)
    out = out[:n - 1]
    out.append({"speech_threshold_factor": 1e9})
    return out


def stat_cfgs_of(configs, seed):
    """run_sweep's StatConfig for most configs, other extrusion / gap settings for a few"""
    rng = np.random.default_rng(seed)
    out = []
    for i, c in enumerate(configs):
        sc = {"ignore_shorter_than_sec": float(np.float32(c.get("min_vad_duration_sec", 0.7))), **STAT}
        if i % 5 == 3:
            sc.update(extrude_start=float(rng.uniform(0, 2)), extrude_end=0.0, fill_gaps=float(rng.choice([0.0, 1.5, 30.0])))
        out.append(sc)
    return out


def make_labels(rng, dur_sec, n, kind):
    """unsorted labels over [0, dur_sec) with overlaps, short and zero-length ones and gaps of exactly 5 s (fill_gaps)"""
    if kind == "empty":
        return []
    labs = []
    for _ in range(n):
        a = float(np.float32(rng.uniform(0, dur_sec)))
        labs.append((a, float(np.float32(a + rng.uniform(0.2, 8.0)))))
    for _ in range(n // 4):      # overlapping and nested: a long label around a few others
        a = float(np.float32(rng.uniform(0, dur_sec)))
        labs.append((a, float(np.float32(a + rng.uniform(10.0, 40.0)))))
    for _ in range(n // 4):      # shorter than every ignore threshold, and zero-length
        a = float(np.float32(rng.uniform(0, dur_sec)))
        labs.append((a, float(np.float32(a + rng.uniform(0.0, 0.1)))))
        labs.append((a, a))
    for k in range(4):           # gaps of exactly fill_gaps (integers: exact in f32)
        a = float(int(rng.uniform(0, max(dur_sec - 40, 1.0))))
        labs += [(a, a + 3.0), (a + 8.0, a + 10.0), (a + 15.0, a + 16.0)]
    labs.append(labs[0])         # a duplicate
    order = rng.permutation(len(labs))
    return [labs[i] for i in order]


def want_stats(fv, segs, labels, sc):
    """the yardstick: fvad_segment_to_sec per segment, then fvad_stats_from_segments"""
    secs = []
    for x in segs:
        s = fv.SpeechSegment()
        s.sample_from, s.sample_to = x[0], x[1]
        r = fv.lib().fvad_segment_to_sec(C.byref(s), FS)
        secs.append((r.from_sec, r.to_sec))
    return fv.single_stats_to_array(fv.stats_from_segments(secs, labels, sc))


def scored_sweep(fv, n_streams, nch, n_chunks, configs, seed, n_threads=16):
    sw = fv.VadSweep(n_streams, configs, n_channels=nch)
    bins, _ = sw.bands()
    band, rms = synth_inputs(n_streams, nch, n_chunks, bins, seed)
    sw.run(band, rms, n_threads=8)
    rng = np.random.default_rng(seed)
    dur = n_chunks * CHUNK / FS
    refs = [make_labels(rng, dur, int(dur / 6), "empty" if s == 1 else "mixed") for s in range(n_streams)]
    scs = stat_cfgs_of(configs, seed)
    sw.set_references(refs, scs)
    sw.score(n_threads)
    return sw, refs, scs


def assert_stats_equal_yardstick(fv, sw, refs, scs, n_configs):
    n_empty = 0
    for c in range(n_configs):
        got = sw.config_stats(c)
        segs = sw.segments(c)
        for s, ref in enumerate(refs):
            want = want_stats(fv, segs[s], ref, scs[c])
            assert np.array_equal(got[s].view(np.uint32), want.view(np.uint32)), (s, c, got[s], want)
            n_empty += len(segs[s]) == 0
    return n_empty


def test_batch_score_equals_stats_from_segments(fv):
    configs = score_configs(16, seed=1)
    sw, refs, scs = scored_sweep(fv, 5, 2, 160, configs, seed=7)
    n_empty = assert_stats_equal_yardstick(fv, sw, refs, scs, len(configs))
    assert n_empty >= 5                          # the last config's machines, at least
    assert sum(len(x) for c in range(len(configs)) for x in sw.segments(c)) > 300
    assert np.isnan(sw.config_stats(0)[1][4])    # the stream without labels: P = TP + 0 ... its rates as the reference has them
    # 1 thread gives the same bits as 16
    one = sw.config_stats(3).copy()
    sw.score(1)
    assert np.array_equal(sw.config_stats(3).view(np.uint32), one.view(np.uint32))


def test_plain_batch_and_mono_streams(fv):
    # a batch from fvad_vad_batch_create (one config) is scored the same way
    n_streams, n_chunks = 4, 120
    vb = fv.VadBatch(n_streams, n_channels=1)
    band, rms = synth_inputs(n_streams, 1, n_chunks, [(11, 43)], seed=3)
    segs = vb.run(np.ascontiguousarray(band[0]), rms)
    rng = np.random.default_rng(3)
    refs = [make_labels(rng, n_chunks * CHUNK / FS, 12, "mixed") for _ in range(n_streams)]
    sc = {"ignore_shorter_than_sec": float(np.float32(0.7)), **STAT}
    flat = np.ascontiguousarray(np.concatenate([np.asarray(r, np.float32).reshape(-1, 2) for r in refs]))
    offs = (fv.sz * (n_streams + 1))(*np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(int).tolist())
    scs = (fv.StatConfig * 1)(fv.StatConfig(sc["ignore_shorter_than_sec"], 5.0, 10.0, 5.0))
    lib = fv.lib()
    assert lib.fvad_vad_batch_set_references(vb.h, flat.ctypes.data_as(C.POINTER(fv.SegmentSec)), offs, scs) == 0
    assert lib.fvad_vad_batch_score(vb.h, 4) == 0
    out = (fv.SingleStats * n_streams)()
    assert lib.fvad_vad_batch_config_stats(vb.h, 0, out) == 0
    for s in range(n_streams):
        want = want_stats(fv, segs[s], refs[s], sc)
        assert np.array_equal(fv.single_stats_to_array(out[s]).view(np.uint32), want.view(np.uint32)), s


def test_two_hour_stream_sample_indices_past_2_24(fv):
    configs = [{}, {"speech_threshold_factor": 3.0, "long_term_speech_avg_sec": 30.0}, CONFIGS[4]]
    sw, refs, scs = scored_sweep(fv, 1, 1, 14400, configs, seed=12)
    assert max(x[1] for c in range(len(configs)) for x in sw.segments(c)[0]) > 1 << 24
    assert_stats_equal_yardstick(fv, sw, refs, scs, len(configs))


def test_argument_errors(fv):
    lib = fv.lib()
    E = fv.FVAD_ERR_INVALID_ARGUMENT
    sw = fv.VadSweep(2, [{}, {"speech_threshold_factor": 3.0}])
    refs = (fv.SegmentSec * 3)(fv.SegmentSec(1.0, 2.0), fv.SegmentSec(0.5, 4.0), fv.SegmentSec(3.0, 5.0))
    scs = (fv.StatConfig * 2)()
    offs = (fv.sz * 3)(0, 2, 3)
    out = (fv.SingleStats * 2)()
    # nothing scored yet, no references to score against
    assert lib.fvad_vad_batch_config_stats(sw.h, 0, out) == E
    assert lib.fvad_vad_batch_score(sw.h, 1) == E
    assert lib.fvad_vad_batch_set_references(None, refs, offs, scs) == E
    assert lib.fvad_vad_batch_set_references(sw.h, refs, None, scs) == E
    assert lib.fvad_vad_batch_set_references(sw.h, refs, offs, None) == E
    assert lib.fvad_vad_batch_set_references(sw.h, None, offs, scs) == E                  # labels announced, none given
    assert lib.fvad_vad_batch_set_references(sw.h, refs, (fv.sz * 3)(1, 2, 3), scs) == E  # offsets[0] != 0
    assert lib.fvad_vad_batch_set_references(sw.h, refs, (fv.sz * 3)(0, 2, 1), scs) == E  # not monotone
    nan = (fv.SegmentSec * 3)(fv.SegmentSec(1.0, 2.0), fv.SegmentSec(float("nan"), 4.0), fv.SegmentSec(3.0, 5.0))
    assert lib.fvad_vad_batch_set_references(sw.h, nan, offs, scs) == E
    assert lib.fvad_vad_batch_set_references(sw.h, None, (fv.sz * 3)(0, 0, 0), scs) == 0  # no labels at all is fine
    assert lib.fvad_vad_batch_set_references(sw.h, refs, offs, scs) == 0
    assert lib.fvad_vad_batch_config_stats(sw.h, 0, out) == E   # references set, nothing scored
    assert lib.fvad_vad_batch_score(sw.h, 2) == 0               # (no run yet: every machine has no segments)
    assert lib.fvad_vad_batch_config_stats(sw.h, 1, out) == 0
    assert lib.fvad_vad_batch_config_stats(sw.h, 2, out) == E   # past the configs
    assert lib.fvad_vad_batch_config_stats(sw.h, 0, None) == E
    assert lib.fvad_vad_batch_score(None, 1) == E
    assert lib.fvad_vad_batch_set_keep_segments(None, 0) == E
    # new references or a new run: the scores are of other segments, gone until scored again
    assert lib.fvad_vad_batch_set_references(sw.h, refs, offs, scs) == 0
    assert lib.fvad_vad_batch_config_stats(sw.h, 0, out) == E
    assert lib.fvad_vad_batch_score(sw.h, 2) == 0
    bins, _ = sw.bands()
    band, rms = synth_inputs(2, 1, 8, bins, seed=2)
    sw.run(band, rms)
    assert lib.fvad_vad_batch_config_stats(sw.h, 0, out) == E
    # keep_segments 0 only concerns device runs: a host run keeps its segments
    sw.keep_segments(False)
    sw.run(band, rms)
    assert lib.fvad_vad_batch_total_segments(sw.h) == sum(len(x) for x in sw.segments(0))
    sw.close()


# ------------------------------------------------------------------ run_grid's grid, without a GPU
def test_expand_grid_order_and_base(pkg):
    sim = pkg.simulator
    grid = {"base": {"max_speech_gap_sec": 2, "speech_threshold_factor": 1},
            "axes": {"speech_threshold_factor": [5, 7, 10], "initial_long_term_avg": [None, 0.01], "speech_min_freq": [300]}}
    cfgs = sim.expand_grid(grid)
    assert len(cfgs) == 6
    # axes in file order, the last axis fastest, each on top of base
    want = []
    for f in (5, 7, 10):
        for init in (None, 0.01):
            want.append(sim.vad_overrides({"max_speech_gap_sec": 2, "speech_threshold_factor": f, "initial_long_term_avg": init,
                                           "speech_min_freq": 300}))
    assert cfgs == want
    assert cfgs[0]["has_initial_long_term_avg"] == 0 and cfgs[1]["initial_long_term_avg"] == 0.01
    assert sim.expand_grid({"base": {"speech_threshold_factor": 4}}) == [{"speech_threshold_factor": 4.0}]
    # file order is JSON object order
    text = '{"axes": {"min_vad_duration_sec": [0.5, 1.0], "speech_threshold_factor": [3, 4]}}'
    assert [(c["min_vad_duration_sec"], c["speech_threshold_factor"]) for c in sim.expand_grid(json.loads(text))] == \
        [(0.5, 3.0), (0.5, 4.0), (1.0, 3.0), (1.0, 4.0)]


@pytest.mark.parametrize("grid,words", [
    ({"axes": {"speech_treshold_factor": [1, 2]}}, ["speech_treshold_factor", "speech_threshold_factor", "min_vad_duration_sec"]),
    ({"base": {"fft_size": 2048}}, ["fft_size", "valid fields"]),
    ({"axes": {"speech_threshold_factor": []}}, ["empty"]),
    ({"axes": {"speech_threshold_factor": 5}}, ["empty"]),
    ({"axes": {"speech_threshold_factor": list(range(200)), "max_speech_gap_sec": list(range(100))}}, ["20000", "GRID_MAX_CONFIGS"]),
    ({"axis": {"speech_threshold_factor": [1]}}, ["axis"]),
    ({"axes": {"speech_threshold_factor": ["high"]}}, ["numbers"]),
])
def test_grid_errors_before_any_gpu_work(pkg, tmp_path, grid, words):
    sim = pkg.simulator
    with pytest.raises(ValueError) as e:
        sim.expand_grid(grid)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    # run_grid refuses the grid before it opens the plan or a device (the plan file does not even exist)
    (tmp_path / "grid.json").write_text(json.dumps(grid))
    with pytest.raises(ValueError):
        sim.run_grid(str(tmp_path / "missing-plan.json"), str(tmp_path / "grid.json"), out=None)


def test_grid_stage_choices(pkg, tmp_path):
    sim = pkg.simulator
    grid = {"axes": {"speech_threshold_factor": [5, 7]}}
    with pytest.raises(ValueError, match="vad_on='device'"):
        sim.run_grid(str(tmp_path / "missing-plan.json"), grid, vad_on="host", score_on="device", out=None)
    with pytest.raises(ValueError, match="score_on"):
        sim.run_grid(str(tmp_path / "missing-plan.json"), grid, score_on="gpu", out=None)
    assert sim.GRID_MAX_CONFIGS >= 4096
    rows = [{"config": 0, "F": 0.5}, {"config": 1, "F": float("nan")}, {"config": 2, "F": 0.7}, {"config": 3, "F": 0.5}]
    assert [r["config"] for r in sim._ranked(rows)] == [2, 0, 3, 1]


def test_run_grid_refuses_nan_labels_before_any_gpu_work(pkg, tmp_path):
    # fvad_parse_audacity reads "nan"; the scorers walk labels sorted by start and refuse it.  run_grid says so while it reads the
    # plan, before it opens a device (here there is none: reaching the GPU part would raise FVAD_ERR_NO_DEVICE instead)
    from test_harness import write_wav
    sim = pkg.simulator
    pcm = np.zeros((1, 2 * CHUNK), np.float32)
    write_wav(str(tmp_path / "a.wav"), pcm)
    (tmp_path / "a.txt").write_text("1.0\t2.0\tspeech\nnan\t3.0\tspeech\n")
    plan = {"instances": [{"name": "a", "audio_path": "a.wav", "ref_path": "a.txt"}]}
    (tmp_path / "plan.json").write_text(json.dumps(plan))
    with pytest.raises(ValueError, match="NaN label"):
        sim.run_grid(str(tmp_path / "plan.json"), {"axes": {"speech_threshold_factor": [5, 7]}}, out=None)
