"""run_denoise(source="network") on the GPU (simulator.py --export-denoised --denoised-source network): the files it writes at
48 kHz, 16 kHz and 44.1 kHz against header + the float64 model of every third sample of the resident denoised lanes (the
network's own output, lane[3 j + 2]) with the lagged default taps -- the f32 file within the computed bound, the PCM16 file the
exact conversion of the f32 file's values, the 16 kHz f32 file the samples themselves; sliced, device-ingest and combined runs
against the resident one, byte for byte; "source" over 44.1 kHz inputs; source="lanes" and no option against today's bytes; and
the refusals."""
import filecmp
import os

import numpy as np
import pytest

import egress_cases as ec
import egress_strided_cases as es
import ingest_resample_cases as rc
from test_ingest_resample_harness_gpu import at_rate, write_corpus
from test_vad_score_gpu import write_plan

pytestmark = pytest.mark.gpu

# test_egress_resample_harness_gpu.py's streams: mono and stereo, 40, 37 and 9 whole chunks and a partial last one
STREAMS = [(1, "pcm16", 20.4), (2, "f32", 18.7), (2, "pcm16", 4.6)]
CHUNKS = (40, 37, 9)
# rate -> (the file's rate, up, down, lag, lead)
RATES = {None: (48000, 3, 1, 2, 0), 16000: (16000, 1, 1, 0, 2), 44100: (44100, 441, 160, 294, 0)}
FORMATS = {"pcm16": ec.PCM16, "f32": ec.F32}


@pytest.fixture(scope="module")
def ref(pkg, fv, gpu_ctx, tmp_path_factory):
    """the plan, the denoised lanes per instance through the existing path, and run_denoise's resident files per rate and format:
    computed once, shared, never changed"""
    sim, ctx = pkg.simulator, gpu_ctx
    root = tmp_path_factory.mktemp("denoise_network")
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
        manifests = {(rate, fmt): sim.run_denoise(plan_path, str(root / f"{rate}-{fmt}"), fmt=fmt, ctx=ctx, rate=rate, source="network")
                     for rate in RATES for fmt in FORMATS}
    assert [x.shape for x in lanes] == [(nch, n * 24000) for (nch, _, _), n in zip(STREAMS, CHUNKS)]
    assert all(np.abs(x).max() > 1e-3 for x in lanes)
    return {"root": root, "plan": plan_path, "lanes": lanes, "manifests": manifests}


def read(path):
    with open(path, "rb") as f:
        return np.frombuffer(f.read(), np.uint8)


@pytest.mark.parametrize("rate", list(RATES), ids=str)
def test_files_are_header_plus_the_model_of_the_networks_samples(fv, ref, rate):
    R, up, down, lag, lead = RATES[rate]
    assert fv.resample_ratio(16000, R) == (up, down) and es.network_filter(R) == dict(up=up, down=down, lag=lag, lead=lead, n_taps=es.network_filter(R)["n_taps"])
    taps = np.array([1.0], np.float32) if R == 16000 else es.lagged(fv.resample_design(up, down), lag)
    for i, lanes in enumerate(ref["lanes"]):
        x = np.ascontiguousarray(lanes[:, 2::3])        # the network's own samples
        nch, n = x.shape
        assert n == CHUNKS[i] * 8000
        frames = rc.out_frames(n, up, down)
        assert frames == rc.out_frames(lanes.shape[1], *fv.resample_ratio(48000, R))   # the count the lanes path gives at R
        y, B = rc.resample_model(np.ascontiguousarray(x.T).astype(np.float64), taps, up, down, 0, frames)
        vals = None
        for fmt, code in (("f32", ec.F32), ("pcm16", ec.PCM16)):
            m = ref["manifests"][(rate, fmt)][i]
            want = {"name": f"stream{i}", "file": str(ref["root"] / f"{rate}-{fmt}" / f"stream{i}-denoised.wav"), "format": fmt, "channels": nch,
                    "frames": frames, "sample_rate": R, "source": "network", "lead": lead}
            if R != 16000:
                want["resample"] = {"up": up, "down": down, "half": 16, "cutoff": 0.45 / max(up, down), "beta": 6.0, "lag": lag}
            assert m == want
            got = read(m["file"])
            assert got.size == 44 + frames * nch * ec.SAMPLE_BYTES[code]
            assert got[:44].tobytes() == fv.wav_header(code, nch, R, frames)
            if fmt == "f32":   # held against the float64 model, within gamma(up, n_taps) * B + one ulp
                vals = got[44:].copy().view("<f4")
                assert not np.isnan(vals).any()
                rc.compare(np.ascontiguousarray(vals.reshape(frames, nch).T), y, B, up, taps.size, m["file"])
                if R == 16000:   # the network's samples themselves, -0.0 apart (fma(1, -0, +0) is +0)
                    assert np.array_equal((np.ascontiguousarray(x.T).reshape(-1) + np.float32(0.0)).view(np.uint32), vals.view(np.uint32))
            else:              # the exact conversion of the f32 file's values
                ec.compare(got[44:], ec.encode(vals.view(np.uint32), code, False).reshape(-1), m["file"])


@pytest.mark.parametrize("rate,fmt", [(None, "pcm16"), (44100, "f32"), (16000, "pcm16")], ids=str)
@pytest.mark.parametrize("kw", [{"slice_chunks": 16}, {"ingest": "device"}, {"slice_chunks": 16, "ingest": "device"}],
                         ids=["sliced", "device-ingest", "sliced-device-ingest"])
def test_sliced_and_device_ingest_runs_write_the_same_bytes(pkg, gpu_ctx, ref, tmp_path, rate, fmt, kw):
    with gpu_ctx.options(reproducible="1", ingest_ring_bytes="1048576"):   # (every file crosses the ring in pieces)
        got = pkg.simulator.run_denoise(ref["plan"], str(tmp_path), fmt=fmt, ctx=gpu_ctx, rate=rate, source="network", **kw)
    want = ref["manifests"][(rate, fmt)]
    assert [{**m, "file": os.path.basename(m["file"])} for m in got] == [{**m, "file": os.path.basename(m["file"])} for m in want]
    names = sorted(os.listdir(ref["root"] / f"{rate}-{fmt}"))
    assert names == sorted(os.listdir(tmp_path)) and len(names) == len(STREAMS)
    match, mismatch, errors = filecmp.cmpfiles(ref["root"] / f"{rate}-{fmt}", tmp_path, names, shallow=False)
    assert match == names and not mismatch and not errors


def test_source_rate_writes_the_fixed_rate_runs_files(pkg, fv, gpu_ctx, tmp_path):
    sim = pkg.simulator
    files = {}
    for i, (name, nch, fmt, sec) in enumerate((("cd", 1, "pcm16", 5.2), ("cd2", 2, "f32", 3.7))):
        pcm, labels = pkg.synth.make_stream(sec, seed=900 + i, n_channels=nch)
        files[name] = (at_rate(pcm, 44100), 44100, fmt, labels)
    (tmp_path / "in").mkdir()
    plan = write_corpus(pkg, tmp_path / "in", files)
    with gpu_ctx.options(reproducible="1"):
        got = sim.run_denoise(plan, str(tmp_path / "out"), fmt="pcm16", ctx=gpu_ctx, ingest="device", rate="source", source="network")
        fixed = sim.run_denoise(plan, str(tmp_path / "out441"), fmt="pcm16", ctx=gpu_ctx, ingest="device", rate=44100, source="network")
    for m, m441 in zip(got, fixed):
        assert {**m, "file": ""} == {**m441, "file": ""} and m["sample_rate"] == 44100 and m["resample"]["lag"] == 294 and m["lead"] == 0
        p = fv.wav_probe(m["file"])
        assert (p["sample_rate"], p["n_frames"], p["n_channels"], p["format"]) == (44100, m["frames"], m["channels"], ec.PCM16)
        assert filecmp.cmp(m["file"], m441["file"], shallow=False)


def test_lanes_and_no_option_write_what_run_denoise_writes_today(pkg, fv, gpu_ctx, ref, tmp_path):
    sim = pkg.simulator
    with gpu_ctx.options(reproducible="1"):
        runs = {k: sim.run_denoise(ref["plan"], str(tmp_path / k), fmt="pcm16", ctx=gpu_ctx, **kw)
                for k, kw in (("plain", {}), ("lanes", {"source": "lanes"}), ("lanes16", {"source": "lanes", "rate": 16000}), ("r16", {"rate": 16000}))}
    for i, x in enumerate(ref["lanes"]):
        nch, n = x.shape
        want = fv.wav_header(ec.PCM16, nch, 48000, n) + ec.encode(np.ascontiguousarray(x.T).reshape(-1).view(np.uint32), ec.PCM16, False).tobytes()
        for k in ("plain", "lanes"):
            m = runs[k][i]
            assert m == {"name": f"stream{i}", "file": str(tmp_path / k / f"stream{i}-denoised.wav"), "format": "pcm16", "channels": nch, "frames": n,
                         "sample_rate": 48000}                                                     # no new keys
            ec.compare(read(m["file"]), np.frombuffer(want, np.uint8), m["file"])
        a, b = runs["lanes16"][i], runs["r16"][i]
        assert {**a, "file": ""} == {**b, "file": ""} and sorted(a) == ["channels", "file", "format", "frames", "name", "resample", "sample_rate"]
        assert a["resample"] == {"up": 1, "down": 3, "half": 16, "cutoff": 0.45 / 3, "beta": 6.0}
        assert filecmp.cmp(a["file"], b["file"], shallow=False)


def test_refusals_happen_before_any_file_exists(pkg, ref, tmp_path):
    sim = pkg.simulator
    out = tmp_path / "never"
    for kw in (dict(source="network", rate=11025), dict(source="network", rate=44101), dict(source="network", rate=0), dict(source="network", rate=True),
               dict(source="network", rate="48000"), dict(source="nets"), dict(source=None), dict(source="network", kinds=("denoised", "original")),
               dict(source="network", kinds=("residual",)), dict(source="network", kinds=("mix",), mix=0.5)):
        with pytest.raises(ValueError):
            sim.run_denoise(ref["plan"], str(out), ctx=None, **kw)   # (no context is made: the check comes first)
    with pytest.raises(ValueError, match="--export-denoised"):
        sim.main(["-i", ref["plan"], "--denoised-source", "network"])
    with pytest.raises(ValueError):
        sim.main(["-i", ref["plan"], "--export-denoised", str(out), "--denoised-source", "network", "--denoised-rate", "11025"])
    with pytest.raises(ValueError):
        sim.main(["-i", ref["plan"], "--export-denoised", str(out), "--denoised-source", "network", "--denoised-kinds", "denoised,residual"])
    assert not out.exists()
