"""run_denoise(rate=...) on the GPU (simulator.py --export-denoised --denoised-rate): the files it writes at 44.1 kHz and 16 kHz
against header + the float64 model of the resident denoised lanes (the f32 file within the computed bound, the PCM16 file the exact
conversion of the f32 file's values); sliced, device-ingest and combined runs against the resident one, byte for byte; "source"
over 44.1 kHz inputs; None and 48000 against what run_denoise writes without the option; and the refusals."""
import filecmp
import os

import numpy as np
import pytest

import egress_cases as ec
import ingest_resample_cases as rc
from test_ingest_resample_harness_gpu import at_rate, write_corpus
from test_vad_score_gpu import write_plan

pytestmark = pytest.mark.gpu

# mono and stereo, a few chunks each (40, 37 and 9 whole chunks, a partial last one): with slice_chunks=16 the stereo group's
# second member ends before the first slice boundary, the others cross two
STREAMS = [(1, "pcm16", 20.4), (2, "f32", 18.7), (2, "pcm16", 4.6)]
CHUNKS = (40, 37, 9)
RATES = {44100: (147, 160), 16000: (1, 3)}
FORMATS = {"pcm16": ec.PCM16, "f32": ec.F32}


@pytest.fixture(scope="module")
def ref(pkg, fv, gpu_ctx, tmp_path_factory):
    """the plan, the denoised lanes per instance through the existing path, and run_denoise's resident files per rate and format:
    computed once, shared, never changed"""
    sim, ctx = pkg.simulator, gpu_ctx
    root = tmp_path_factory.mktemp("denoise_rates")
    plan_path = write_plan(pkg, root, STREAMS)
    plan = sim.load_plan(plan_path)
    held = []

    def dalloc(nbytes):
        held.append(ctx.device_alloc(max(int(nbytes), 4)))
        return held[-1]

    with ctx.options(reproducible="1"):
        try:
            audio = [a for a, _ in sim._load_instances(plan, "host")]
            r = sim._denoise_resident(ctx, audio, plan["fft_size"], plan["vad_machine_config"], dalloc)
            den = ctx.to_host(np.empty((r.n_lanes, r.n_den), np.float32), r.d_den)
        finally:
            for d in held:
                ctx.device_free(d)
        lanes, l = [None] * len(audio), 0
        for i in r.order:
            nch = audio[i].shape[0]
            lanes[i] = np.ascontiguousarray(den[l:l + nch, :r.n_chunks[i] * 24000])
            l += nch
        manifests = {(rate, fmt): sim.run_denoise(plan_path, str(root / f"{rate}-{fmt}"), fmt=fmt, ctx=ctx, rate=rate) for rate in RATES for fmt in FORMATS}
    assert [x.shape for x in lanes] == [(nch, n * 24000) for (nch, _, _), n in zip(STREAMS, CHUNKS)]
    assert all(np.abs(x).max() > 1e-3 for x in lanes)
    return {"root": root, "plan": plan_path, "lanes": lanes, "manifests": manifests}


def read(path):
    with open(path, "rb") as f:
        return np.frombuffer(f.read(), np.uint8)


@pytest.mark.parametrize("rate", list(RATES))
def test_files_are_header_plus_the_model_of_the_resident_lanes(fv, ref, rate):
    up, down = RATES[rate]
    assert fv.resample_ratio(48000, rate) == (up, down)
    taps = fv.resample_design(up, down)
    m_ = max(up, down)
    for i, x in enumerate(ref["lanes"]):
        nch, n = x.shape
        frames = rc.out_frames(n, up, down)
        y, B = rc.resample_model(np.ascontiguousarray(x.T).astype(np.float64), taps, up, down, 0, frames)
        vals = None
        for fmt, code in (("f32", ec.F32), ("pcm16", ec.PCM16)):
            m = ref["manifests"][(rate, fmt)][i]
            assert m == {"name": f"stream{i}", "file": str(ref["root"] / f"{rate}-{fmt}" / f"stream{i}-denoised.wav"), "format": fmt, "channels": nch,
                         "frames": frames, "sample_rate": rate, "resample": {"up": up, "down": down, "half": 16, "cutoff": 0.45 / m_, "beta": 6.0}}
            got = read(m["file"])
            assert got.size == 44 + frames * nch * ec.SAMPLE_BYTES[code]
            assert got[:44].tobytes() == fv.wav_header(code, nch, rate, frames)
            assert fv.wav_probe(m["file"]) == {"format": code, "n_channels": nch, "sample_rate": rate, "data_offset": 44, "n_frames": frames,
                                               "bits": 8 * ec.SAMPLE_BYTES[code]}
            if fmt == "f32":   # held against the float64 model, within gamma(up, n_taps) * B + one ulp
                vals = got[44:].copy().view("<f4")
                rc.compare(np.ascontiguousarray(vals.reshape(frames, nch).T), y, B, up, taps.size, m["file"])
            else:              # the exact conversion of the f32 file's values
                ec.compare(got[44:], ec.encode(vals.view(np.uint32), code, False).reshape(-1), m["file"])


@pytest.mark.parametrize("rate,fmt", [(44100, "pcm16"), (44100, "f32"), (16000, "pcm16")])
@pytest.mark.parametrize("kw", [{"slice_chunks": 16}, {"ingest": "device"}, {"slice_chunks": 16, "ingest": "device"}],
                         ids=["sliced", "device-ingest", "sliced-device-ingest"])
def test_sliced_and_device_ingest_runs_write_the_same_bytes(pkg, gpu_ctx, ref, tmp_path, rate, fmt, kw):
    with gpu_ctx.options(reproducible="1", ingest_ring_bytes="1048576"):   # (every file crosses the ring in pieces)
        got = pkg.simulator.run_denoise(ref["plan"], str(tmp_path), fmt=fmt, ctx=gpu_ctx, rate=rate, **kw)
    want = ref["manifests"][(rate, fmt)]
    assert [{**m, "file": os.path.basename(m["file"])} for m in got] == [{**m, "file": os.path.basename(m["file"])} for m in want]
    names = sorted(os.listdir(ref["root"] / f"{rate}-{fmt}"))
    assert names == sorted(os.listdir(tmp_path)) and len(names) == len(STREAMS)
    match, mismatch, errors = filecmp.cmpfiles(ref["root"] / f"{rate}-{fmt}", tmp_path, names, shallow=False)
    assert match == names and not mismatch and not errors


def test_source_writes_each_instance_at_its_files_rate(pkg, fv, gpu_ctx, tmp_path):
    sim = pkg.simulator
    files = {}
    for i, (name, rate, nch, fmt, sec) in enumerate((("cd", 44100, 1, "pcm16", 5.2), ("cd2", 44100, 2, "f32", 3.7), ("native", 48000, 1, "pcm16", 2.4))):
        pcm, labels = pkg.synth.make_stream(sec, seed=900 + i, n_channels=nch)
        files[name] = (at_rate(pcm, rate), rate, fmt, labels)
    (tmp_path / "in").mkdir()
    plan = write_corpus(pkg, tmp_path / "in", files)
    with gpu_ctx.options(reproducible="1"):
        got = sim.run_denoise(plan, str(tmp_path / "out"), fmt="pcm16", ctx=gpu_ctx, ingest="device", rate="source")
        at48 = sim.run_denoise(plan, str(tmp_path / "out48"), fmt="pcm16", ctx=gpu_ctx, ingest="device")
        fixed = sim.run_denoise(plan, str(tmp_path / "out441"), fmt="pcm16", ctx=gpu_ctx, ingest="device", rate=44100)
    for m, m48, m441, (name, (_, rate, _, _)) in zip(got, at48, fixed, files.items()):
        up, down = fv.resample_ratio(48000, rate)
        assert m["sample_rate"] == rate and m["frames"] == rc.out_frames(m48["frames"], up, down) and m["channels"] == m48["channels"]
        assert ("resample" in m) == (rate != 48000) and "resample" not in m48
        p = fv.wav_probe(m["file"])
        assert (p["sample_rate"], p["n_frames"], p["n_channels"], p["format"]) == (m["sample_rate"], m["frames"], m["channels"], ec.PCM16)
        # the native instance left through fvad_egress: the file of the run without the option; the others are the fixed-rate run's
        assert filecmp.cmp(m["file"], (m48 if rate == 48000 else m441)["file"], shallow=False)
        assert m441["sample_rate"] == 44100


def test_none_and_48000_write_what_run_denoise_writes_today(pkg, fv, gpu_ctx, ref, tmp_path):
    sim = pkg.simulator
    with gpu_ctx.options(reproducible="1"):
        runs = {k: sim.run_denoise(ref["plan"], str(tmp_path / k), fmt="pcm16", ctx=gpu_ctx, **kw)
                for k, kw in (("plain", {}), ("none", {"rate": None}), ("r48000", {"rate": 48000}), ("source", {"rate": "source"}))}
    for i, x in enumerate(ref["lanes"]):
        nch, n = x.shape
        want = fv.wav_header(ec.PCM16, nch, 48000, n) + ec.encode(np.ascontiguousarray(x.T).reshape(-1).view(np.uint32), ec.PCM16, False).tobytes()
        for k, ms in runs.items():
            assert ms[i] == {"name": f"stream{i}", "file": str(tmp_path / k / f"stream{i}-denoised.wav"), "format": "pcm16", "channels": nch,
                             "frames": n, "sample_rate": 48000}
            ec.compare(read(ms[i]["file"]), np.frombuffer(want, np.uint8), ms[i]["file"])


def test_bad_rates_and_mode_combinations_raise_before_any_file_exists(pkg, ref, tmp_path):
    sim = pkg.simulator
    out = tmp_path / "never"
    for rate in (44101, 0, -44100, 7, True, "src", "44100", 44100.0, 1 << 32):
        with pytest.raises(ValueError):
            sim.run_denoise(ref["plan"], str(out), ctx=None, rate=rate)   # (no context is made: the check comes first)
    with pytest.raises(ValueError, match="--export-denoised"):
        sim.main(["-i", ref["plan"], "--denoised-rate", "44100"])
    for extra in (["--sweep"], ["--export-clips", str(out)]):
        with pytest.raises(ValueError, match="--export-denoised"):
            sim.main(["-i", ref["plan"], "--export-denoised", str(out), "--denoised-rate", "44100"] + extra)
    for bad in ("cd", "44.1k", "44101"):
        with pytest.raises(ValueError):
            sim.main(["-i", ref["plan"], "--export-denoised", str(out), "--denoised-rate", bad])
    assert not out.exists()
