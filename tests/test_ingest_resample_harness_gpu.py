"""The harness over a corpus at other rates (ingest="device"): a plan of a mono 44.1 kHz PCM16 instance, a stereo 16 kHz f32
instance and a mono 48 kHz instance through run_sweep, run_grid and run_clips, against the SAME plan over 48 kHz f32 files that
hold the resampled lanes read back from the device -- reports, segments, manifests and clip bytes identical; the runs sliced one
chunk at a time against the unsliced ones, bit for bit; ingest="host" refused with the pointer; and an all-48 kHz plan running
the calls it ran before."""
import filecmp
import json
import os

import numpy as np
import pytest

from test_harness import write_wav
from test_vad_score_gpu import assert_bits

pytestmark = pytest.mark.gpu

GRID = {"base": {"speech_min_freq": 300, "speech_max_freq": 3000},
        "axes": {"speech_threshold_factor": [2.5, 4.0, 7.0], "min_vad_duration_sec": [0.2, 0.7]}}
# (name, rate, channels, format, seconds): a few chunks each, unequal, with a partial last chunk
STREAMS = (("cd", 44100, 1, "pcm16", 11.2), ("asr", 16000, 2, "f32", 9.7), ("native", 48000, 1, "pcm16", 10.4))


def at_rate(pcm, rate):
    """a 48 kHz stream as a file of `rate` would hold it (linear interpolation: the content is what matters here, not its quality)"""
    if rate == 48000:
        return pcm
    n = int(pcm.shape[1] * rate // 48000)
    t = np.arange(n) * (48000.0 / rate)
    return np.stack([np.interp(t, np.arange(pcm.shape[1]), c) for c in pcm]).astype(np.float32)


def write_corpus(pkg, d, files):
    """files {name: (pcm, rate, fmt, labels)} -> the plan's path; fft_size 960, so that a time slice may be one chunk"""
    insts = []
    for name, (pcm, rate, fmt, labels) in files.items():
        write_wav(str(d / f"{name}.wav"), pcm, sample_rate=rate, fmt=fmt)
        (d / f"{name}.txt").write_text(pkg.synth.labels_to_audacity(labels))
        insts.append({"name": name, "audio_path": f"{name}.wav", "ref_path": f"{name}.txt"})
    plan = {"instances": insts, "config": {"vad_config": {"fft_size": 960, "vad_machine_config": {"speech_threshold_factor": 4}}}}
    (d / "plan.json").write_text(json.dumps(plan))
    return str(d / "plan.json")


def device_lanes(sim, fv, ctx, paths):
    """the files' lanes as the harness ingests them, all in one batch -> [instance] float32 [channels][48 kHz frames]"""
    audio = [sim._RawAudio(*fv.wav_map_raw(p)) for p in paths]
    stride = max(a.n_frames for a in audio)
    L = sum(a.n_channels for a in audio)
    d = ctx.device_alloc(L * stride * 4)
    try:
        rows, l = [], 0
        for a in audio:
            rows.append(a.source(0, a.n_frames, l, 0, stride))
            l += a.n_channels
        sim._ingest_rows(ctx, audio, rows, d_lanes=d, n_lanes=L, lane_stride=stride, n_samples=stride)
        lanes = ctx.to_host(np.empty((L, stride), np.float32), d)
    finally:
        ctx.device_free(d)
    out, l = [], 0
    for a in audio:
        out.append(lanes[l:l + a.n_channels, :a.n_frames].copy())
        assert not np.any(lanes[l:l + a.n_channels, a.n_frames:])      # padded with zeros
        l += a.n_channels
    return out, audio


@pytest.fixture(scope="module")
def corpus(pkg, fv, gpu_ctx, tmp_path_factory):
    root = tmp_path_factory.mktemp("rates")
    sim = pkg.simulator
    for d in ("mixed", "as48", "native"):
        (root / d).mkdir()
    files = {}
    for i, (name, rate, nch, fmt, sec) in enumerate(STREAMS):
        pcm, labels = pkg.synth.make_stream(sec, seed=700 + i, n_channels=nch)
        files[name] = (at_rate(pcm, rate), rate, fmt, labels)
    mixed = write_corpus(pkg, root / "mixed", files)
    lanes, audio = device_lanes(sim, fv, gpu_ctx, [str(root / "mixed" / f"{n}.wav") for n in files])
    as48 = {name: (lanes[i] if rate != 48000 else pcm, 48000, "f32" if rate != 48000 else fmt, labels)
            for i, (name, (pcm, rate, fmt, labels)) in enumerate(files.items())}
    return {"root": root, "mixed": mixed, "as48": write_corpus(pkg, root / "as48", as48), "lanes": lanes, "audio": audio, "files": files,
            "native": write_corpus(pkg, root / "native", {"native": files["native"]})}


def test_the_resampled_instances_are_48_khz_instances(fv, pkg, gpu_ctx, corpus):
    a_cd, a_asr, a_nat = corpus["audio"]
    assert (a_cd.rate, a_cd.up, a_cd.down, a_cd.n_channels) == (44100, 160, 147, 1) and (a_asr.rate, a_asr.up, a_asr.down, a_asr.n_channels) == (16000, 3, 1, 2)
    assert a_cd.n_frames == -(-a_cd.file_frames * 160 // 147) and a_asr.n_frames == 3 * a_asr.file_frames and a_nat.rate == 48000
    assert a_cd.taps is pkg.simulator._RawAudio(a_cd.raw, dict(format=a_cd.format, n_channels=1, n_frames=5, bits=16, sample_rate=44100)).taps   # made once per rate
    # the resampled lanes follow the file: the same time axis (zero phase), the level of the 48 kHz original they were made from
    for lane, (pcm, rate, _, _) in zip(corpus["lanes"], (corpus["files"][n] for n in ("cd", "asr"))):
        src, _ = pkg.synth.make_stream(*[(s[4], 700 + i, s[2]) for i, s in enumerate(STREAMS) if s[1] == rate][0])
        n = min(lane.shape[1], src.shape[1]) - 4800
        err = lane[:, 2400:n].astype(np.float64) - src[:, 2400:n]
        assert np.sqrt(np.mean(err ** 2)) < 0.5 * np.sqrt(np.mean(src[:, 2400:n].astype(np.float64) ** 2))
    # the 48 kHz instance beside them: the lanes fvad_ingest alone gives, bit for bit
    alone, _ = device_lanes(pkg.simulator, fv, gpu_ctx, [str(corpus["root"] / "native" / "native.wav")])
    assert_bits(corpus["lanes"][2], alone[0])
    pcm16 = np.clip(np.round(corpus["files"]["native"][0] * 32768.0), -32768, 32767).astype(np.int16).astype(np.float32) * np.float32(1.0 / 32768.0)
    assert_bits(alone[0], pcm16)


def _same_grid(a, b, slices=True):
    assert_bits(a["stats"], b["stats"])
    assert a["configs"] == b["configs"] and (not slices or a["slices"] == b["slices"])
    assert json.dumps(a["rows"], sort_keys=True) == json.dumps(b["rows"], sort_keys=True)


def test_sweep_and_grid_equal_the_runs_over_the_resampled_files(pkg, gpu_ctx, corpus):
    sim = pkg.simulator
    with gpu_ctx.options(reproducible="1"):
        got = sim.run_sweep(corpus["mixed"], ctx=gpu_ctx, out=None, ingest="device")
        want = sim.run_sweep(corpus["as48"], ctx=gpu_ctx, out=None, ingest="device")
        assert got["segments"] == want["segments"] and [bytes(a) for a in got["aggregates"]] == [bytes(a) for a in want["aggregates"]]
        assert json.dumps(got["rows"], sort_keys=True) == json.dumps(want["rows"], sort_keys=True)
        assert sum(len(s) for per in got["segments"] for s in per) >= 2          # the machines found the speech
        whole = sim.run_grid(corpus["mixed"], GRID, ctx=gpu_ctx, out=None, vad_on="device", score_on="device", ingest="device")
        _same_grid(whole, sim.run_grid(corpus["as48"], GRID, ctx=gpu_ctx, out=None, vad_on="device", score_on="device", ingest="device"))
        assert float(whole["stats"][:, :, 1].sum()) > 0                          # true positives
        # one chunk a slice: every slice of a resampled instance is a row that gives the window of its outputs
        sliced = sim.run_grid(corpus["mixed"], GRID, ctx=gpu_ctx, out=None, vad_on="device", score_on="device", ingest="device", slice_chunks=1)
        assert sliced["slices"] > 10
        _same_grid(sliced, whole, slices=False)
        _same_grid(sliced, sim.run_grid(corpus["as48"], GRID, ctx=gpu_ctx, out=None, vad_on="device", score_on="device", ingest="device", slice_chunks=1))


def _same_clips(a, b, dir_a, dir_b):
    (text_a, res_a), (text_b, res_b) = a, b
    assert text_a == text_b
    for x, y in zip(res_a, res_b):
        assert x["segments"] == y["segments"] and x["audit"] == y["audit"] and x["clips"] == y["clips"]
    names = sorted(os.listdir(dir_a))
    assert names == sorted(os.listdir(dir_b))
    match, mismatch, errors = filecmp.cmpfiles(dir_a, dir_b, names, shallow=False)
    assert match == names and not mismatch and not errors
    return names


def test_clips_equal_the_clips_of_the_resampled_files(pkg, gpu_ctx, corpus):
    sim, root = pkg.simulator, corpus["root"]
    with gpu_ctx.options(reproducible="1"):
        runs = {tag: sim.run_clips(corpus[plan], str(root / tag), ctx=gpu_ctx, ingest="device", **kw)
                for tag, plan, kw in (("c-mixed", "mixed", {}), ("c-as48", "as48", {}), ("c-sliced", "mixed", {"slice_chunks": 1}))}
    names = _same_clips(runs["c-mixed"], runs["c-as48"], root / "c-mixed", root / "c-as48")
    assert sum(len(r["segments"]) for r in runs["c-mixed"][1]) >= 2 and any(n.startswith("cd-") and n.endswith(".wav") for n in names)
    _same_clips(runs["c-sliced"], runs["c-mixed"], root / "c-sliced", root / "c-mixed")
    # the manifests speak 48 kHz
    assert all(r["clips"]["sample_rate"] == 48000 for r in runs["c-mixed"][1])


def test_host_ingest_refuses_with_the_pointer(pkg, fv, gpu_ctx, corpus):
    sim = pkg.simulator
    for run in (lambda **kw: sim.run_sweep(corpus["mixed"], ctx=gpu_ctx, out=None, **kw),
                lambda **kw: sim.run_grid(corpus["mixed"], GRID, ctx=gpu_ctx, out=None, **kw),
                lambda **kw: sim.run_grid(corpus["mixed"], GRID, ctx=gpu_ctx, out=None, slice_chunks=1, vad_on="device", score_on="device", **kw),
                lambda **kw: sim.run_clips(corpus["mixed"], str(corpus["root"] / "refused"), ctx=gpu_ctx, **kw)):
        for kw in ({}, {"ingest": "host"}):
            with pytest.raises(fv.FvadError, match="--ingest device") as e:
                run(**kw)
            assert e.value.status == -9 and "44100" in str(e.value)


def test_a_48_khz_plan_runs_the_calls_it_ran_before(pkg, gpu_ctx, corpus):
    sim, ctx = pkg.simulator, gpu_ctx
    was = ctx.timing
    ctx.enable_timing(True)
    try:
        for plan, want in (("native", False), ("mixed", True)):
            for kw in ({}, {"slice_chunks": 1}):
                ctx.kernel_times()
                sim.run_grid(corpus[plan], GRID, ctx=ctx, out=None, vad_on="device", score_on="device", ingest="device", **kw)
                times = ctx.kernel_times()
                assert "ingest" in times and ("ingest_resample" in times) == want, (plan, kw, sorted(times))
    finally:
        ctx.enable_timing(was)
