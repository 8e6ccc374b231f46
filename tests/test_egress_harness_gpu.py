"""run_denoise on the GPU (simulator.py --export-denoised): the files it writes against header + the numpy model's conversion
of the denoised lanes the existing path gives (_denoise_resident, copied back as f32); the f32 file against fvad_wav_write's;
sliced and device-ingest runs against the resident one; a PCM24 file it wrote back through fvad_wav_probe and the device-side
ingest; and the refusals."""
import filecmp
import json
import os

import numpy as np
import pytest

import egress_cases as ec
from test_ingest_gpu import STREAMS   # mono PCM16 33.9 s, stereo f32 61.1 s, stereo PCM16 20.2 s: unequal, a partial last chunk
from test_vad_parts_gpu import GRID
from test_vad_score_gpu import write_plan

pytestmark = pytest.mark.gpu

FORMATS = {"pcm16": ec.PCM16, "pcm24": ec.PCM24, "f32": ec.F32}


@pytest.fixture(scope="module")
def ref(pkg, fv, gpu_ctx, tmp_path_factory):
    """the plan, the denoised lanes per instance through the existing path, and run_denoise's resident files per format:
    computed once, shared, never changed"""
    sim, ctx = pkg.simulator, gpu_ctx
    root = tmp_path_factory.mktemp("denoise")
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
        manifests = {fmt: sim.run_denoise(plan_path, str(root / fmt), fmt=fmt, ctx=ctx) for fmt in FORMATS}
    assert [x.shape for x in lanes] == [(1, 33 * 24000 * 2 + 24000), (2, 122 * 24000), (2, 40 * 24000)]   # whole chunks: 67, 122, 40
    assert all(np.abs(x).max() > 1e-3 for x in lanes)
    return {"root": root, "plan": plan_path, "lanes": lanes, "manifests": manifests}


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_files_are_header_plus_the_models_conversion(fv, ref, fmt):
    code = FORMATS[fmt]
    for i, (m, x) in enumerate(zip(ref["manifests"][fmt], ref["lanes"])):
        nch, n = x.shape
        assert m == {"name": f"stream{i}", "file": str(ref["root"] / fmt / f"stream{i}-denoised.wav"), "format": fmt, "channels": nch,
                     "frames": n, "sample_rate": 48000}
        want = fv.wav_header(code, nch, 48000, n) + ec.encode(np.ascontiguousarray(x.T).reshape(-1).view(np.uint32), code, False).tobytes()
        got = read(m["file"])
        assert len(got) == len(want) == 44 + n * nch * ec.SAMPLE_BYTES[code]
        ec.compare(np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8), m["file"])
        assert fv.wav_probe(m["file"]) == {"format": code, "n_channels": nch, "sample_rate": 48000, "data_offset": 44, "n_frames": n,
                                           "bits": 8 * ec.SAMPLE_BYTES[code]}


def test_the_f32_file_is_fvad_wav_writes(fv, ref, tmp_path):
    for m, x in zip(ref["manifests"]["f32"], ref["lanes"]):
        p = str(tmp_path / "w.wav")
        fv.wav_write(p, x)
        assert filecmp.cmp(p, m["file"], shallow=False), m["file"]


def same_files(ref, fmt, out_dir):
    names = sorted(os.listdir(ref["root"] / fmt))
    assert names == sorted(os.listdir(out_dir)) and len(names) == len(STREAMS)
    match, mismatch, errors = filecmp.cmpfiles(ref["root"] / fmt, out_dir, names, shallow=False)
    assert match == names and not mismatch and not errors


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("kw", [{"slice_chunks": 16}, {"ingest": "device"}, {"slice_chunks": 16, "ingest": "device"}],
                         ids=["sliced", "device-ingest", "sliced-device-ingest"])
def test_sliced_and_device_ingest_runs_write_the_same_bytes(pkg, gpu_ctx, ref, tmp_path, fmt, kw):
    with gpu_ctx.options(reproducible="1", ingest_ring_bytes="1048576"):   # (every file crosses the ring in pieces, both ways)
        got = pkg.simulator.run_denoise(ref["plan"], str(tmp_path), fmt=fmt, ctx=gpu_ctx, **kw)
    assert [(m["name"], m["channels"], m["frames"], m["format"]) for m in got] == \
           [(m["name"], m["channels"], m["frames"], m["format"]) for m in ref["manifests"][fmt]]
    same_files(ref, fmt, tmp_path)


def test_a_24_bit_file_it_wrote_comes_back_through_the_device_ingest(pkg, fv, gpu_ctx, ref, tmp_path):
    sim = pkg.simulator
    src = json.loads(read(ref["plan"]))
    for inst, m in zip(src["instances"], ref["manifests"]["pcm24"]):
        assert fv.wav_probe(m["file"])["format"] == fv.INGEST_PCM24
        inst["audio_path"] = m["file"]
        inst["ref_path"] = str(ref["root"] / inst["ref_path"])
    plan24 = tmp_path / "plan.json"
    plan24.write_text(json.dumps(src))
    with gpu_ctx.options(reproducible="1"):
        got = sim.run_grid(str(plan24), GRID, ctx=gpu_ctx, out=None, vad_on="device", score_on="device", ingest="device")
        # (the seconds P, TP, FP, FN of every config and instance; the rates are NaN where a denoised file has no detection)
        assert len(got["rows"]) == len(got["configs"]) > 0 and got["stats"].shape[:2] == (len(got["configs"]), len(STREAMS))
        assert np.all(np.isfinite(got["stats"][:, :, :4])) and float(got["stats"][:, :, 0].sum()) > 0
        # and written once more as PCM24 from those files: what was quantised to 24 bits stays as it is through the denoiser's
        # input path -- the ingest's s / 8388608 and the egress' rint(y * 8388608) are inverses
        raw, info = fv.wav_map_raw(ref["manifests"]["pcm24"][1]["file"])
        n, nch = info["n_frames"], info["n_channels"]
        d_lanes, d_out = gpu_ctx.device_alloc(n * nch * 4), gpu_ctx.device_alloc(raw.size)
        try:
            gpu_ctx.ingest([(0, n, nch, ec.PCM24, 0, 0, n)], raw=[raw], d_lanes=d_lanes, n_lanes=nch, lane_stride=n, n_samples=n)
            gpu_ctx.egress([(0, n, nch, ec.PCM24, 0, 0)], d_lanes=d_lanes, n_lanes=nch, lane_stride=n, n_samples=n, out=d_out, out_bytes=raw.size)
            ec.compare(gpu_ctx.to_host(np.zeros(raw.size, np.uint8), d_out), np.asarray(raw), "a PCM24 file through ingest and egress")
        finally:
            gpu_ctx.device_free(d_lanes)
            gpu_ctx.device_free(d_out)


def test_bad_formats_and_mode_combinations_raise_before_any_work(pkg, ref, tmp_path):
    sim = pkg.simulator
    out = tmp_path / "never"
    for kw in ({"fmt": "flac"}, {"fmt": "pcm32"}, {"fmt": None}, {"ingest": "gpu"}, {"slice_chunks": 7}):
        with pytest.raises(ValueError):
            sim.run_denoise(ref["plan"], str(out), ctx=None, **kw)   # (no context is made: the check comes first)
    for extra in (["--sweep"], ["--sweep-grid", "g.json"], ["--export-clips", str(out)]):
        with pytest.raises(ValueError, match="--export-denoised"):
            sim.main(["-i", ref["plan"], "--export-denoised", str(out)] + extra)
    with pytest.raises(ValueError, match="--export-denoised"):
        sim.main(["-i", ref["plan"], "--denoised-format", "pcm24"])
    assert not out.exists()
