"""run_denoise(kinds=...) on the GPU (simulator.py --export-denoised --denoised-kinds): the original, residual and mix files it
writes against header + the numpy model over the two lane sets the existing path gives (_denoise_resident, copied back as
f32); the denoised kind against a plain run_denoise; the original file against the input's samples 482 frames later; sliced
and device-ingest runs against the resident one; kinds=None against a call without the argument; and one run with a unit-gain
model, whose residual must fall to the reconstruction ripple the CPU oracle showed (tests/test_nsnet2_delay_host.py)."""
import filecmp
import json
import os

import numpy as np
import pytest

import egress_cases as ec
import egress_mix_cases as mc
from test_ingest_gpu import STREAMS   # mono PCM16 33.9 s, stereo f32 61.1 s (122 chunks: slices with a halo), stereo PCM16 20.2 s
from test_vad_score_gpu import write_plan

pytestmark = pytest.mark.gpu

FORMATS = {"pcm16": ec.PCM16, "f32": ec.F32}
KINDS = ("denoised", "original", "residual", "mix")
MIX = 0.8
WEIGHTS = {"original": (np.float32(1.0), np.float32(0.0)), "residual": (np.float32(1.0), np.float32(-1.0)),
           "mix": (np.float32(1.0) - np.float32(MIX), np.float32(MIX))}


@pytest.fixture(scope="module")
def ref(pkg, fv, gpu_ctx, tmp_path_factory):
    """the plan, both lane sets per instance through the existing path, a plain run_denoise and the resident run with every
    kind, per format: computed once, shared, never changed"""
    sim, ctx = pkg.simulator, gpu_ctx
    root = tmp_path_factory.mktemp("kinds")
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
            pcm = ctx.to_host(np.empty((r.n_lanes, r.stride), np.float32), r.d_pcm)
        finally:
            for d in held:
                ctx.device_free(d)
        lanes, l = [None] * len(audio), 0
        for i in r.order:
            nch, n = audio[i].shape[0], r.n_chunks[i] * 24000
            lanes[i] = (np.ascontiguousarray(pcm[l:l + nch, :n]), np.ascontiguousarray(den[l:l + nch, :n]))
            l += nch
        plain = {fmt: sim.run_denoise(plan_path, str(root / f"plain-{fmt}"), fmt=fmt, ctx=ctx) for fmt in FORMATS}
        manifests = {fmt: sim.run_denoise(plan_path, str(root / fmt), fmt=fmt, ctx=ctx, kinds=KINDS, mix=MIX) for fmt in FORMATS}
    inputs = [a.astype(np.float32) * np.float32(1.0 / 32768.0) if a.dtype == np.int16 else a for a in audio]
    assert [x[1].shape for x in lanes] == [(1, 67 * 24000), (2, 122 * 24000), (2, 40 * 24000)]
    return {"root": root, "plan": plan_path, "lanes": lanes, "inputs": inputs, "plain": plain, "manifests": manifests}


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_files_are_header_plus_the_model(fv, ref, fmt):
    code, D = FORMATS[fmt], fv.nsnet2_delay(48000)
    assert D == 482
    for i, (m, (orig, den)) in enumerate(zip(ref["manifests"][fmt], ref["lanes"])):
        nch, n = den.shape
        assert m["name"] == f"stream{i}" and [e["kind"] for e in m["kinds"]] == list(KINDS)
        for e in m["kinds"]:
            kind = e["kind"]
            w = (None, None) if kind == "denoised" else tuple(float(x) for x in WEIGHTS[kind])
            assert e == {"file": str(ref["root"] / fmt / f"stream{i}-{kind}.wav"), "kind": kind, "w_orig": w[0], "w_den": w[1], "delay": D,
                         "frames": n, "format": fmt, "channels": nch, "sample_rate": 48000}
            got = np.frombuffer(read(e["file"]), np.uint8)
            assert got.size == 44 + n * nch * ec.SAMPLE_BYTES[code]
            assert got[:44].tobytes() == fv.wav_header(code, nch, 48000, n)
            if kind == "denoised":
                continue
            row = np.array([[0, n, nch, code, 0, 0, 0, min(D, n)]], np.uint64)
            want = mc.mix_model(orig, den, row, WEIGHTS[kind][0], WEIGHTS[kind][1], np.zeros(n * nch * ec.SAMPLE_BYTES[code], np.uint8))
            mc.compare(got[44:], want, row, e["file"])


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_the_denoised_kind_is_a_plain_run_denoises_file(ref, fmt):
    for m, p in zip(ref["manifests"][fmt], ref["plain"][fmt]):
        assert filecmp.cmp(m["kinds"][0]["file"], p["file"], shallow=False), p["file"]
        assert sorted(os.listdir(ref["root"] / f"plain-{fmt}")) == [f"stream{i}-denoised.wav" for i in range(len(STREAMS))]


def test_the_original_file_is_the_input_482_frames_later(ref):
    for m, x in zip(ref["manifests"]["f32"], ref["inputs"]):
        e = m["kinds"][1]
        assert e["kind"] == "original"
        nch, n = e["channels"], e["frames"]
        y = np.frombuffer(read(e["file"]), "<f4", offset=44).reshape(n, nch).T
        assert np.array_equal(y[:, 482:], x[:, :n - 482]) and not np.any(y[:, :482]) and np.abs(y).max() > 1e-3


def same_files(want_dir, out_dir, n):
    names = sorted(os.listdir(want_dir))
    assert names == sorted(os.listdir(out_dir)) and len(names) == n
    match, mismatch, errors = filecmp.cmpfiles(want_dir, out_dir, names, shallow=False)
    assert match == names and not mismatch and not errors, (mismatch, errors)


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("kw", [{"slice_chunks": 16}, {"ingest": "device"}, {"slice_chunks": 16, "ingest": "device"}],
                         ids=["sliced", "device-ingest", "sliced-device-ingest"])
def test_sliced_and_device_ingest_runs_write_the_same_bytes(pkg, gpu_ctx, ref, tmp_path, fmt, kw):
    with gpu_ctx.options(reproducible="1", ingest_ring_bytes="1048576"):   # (every file crosses the ring in pieces)
        got = pkg.simulator.run_denoise(ref["plan"], str(tmp_path), fmt=fmt, ctx=gpu_ctx, kinds=KINDS, mix=MIX, **kw)
    strip = lambda ms: [(m["name"], [{k: v for k, v in e.items() if k != "file"} for e in m["kinds"]]) for m in ms]
    assert strip(got) == strip(ref["manifests"][fmt])
    same_files(ref["root"] / fmt, tmp_path, len(STREAMS) * len(KINDS))


def test_kinds_none_is_the_call_without_the_argument(pkg, gpu_ctx, ref, tmp_path):
    with gpu_ctx.options(reproducible="1"):
        got = pkg.simulator.run_denoise(ref["plan"], str(tmp_path), fmt="pcm16", ctx=gpu_ctx, kinds=None, mix=None)
    assert [{k: v for k, v in m.items() if k != "file"} for m in got] == [{k: v for k, v in m.items() if k != "file"} for m in ref["plain"]["pcm16"]]
    assert all(set(m) == {"name", "file", "format", "channels", "frames", "sample_rate"} for m in got)
    same_files(ref["root"] / "plain-pcm16", tmp_path, len(STREAMS))


def test_a_subset_of_kinds_writes_only_those(pkg, gpu_ctx, ref, tmp_path):
    with gpu_ctx.options(reproducible="1"):
        got = pkg.simulator.run_denoise(ref["plan"], str(tmp_path), fmt="f32", ctx=gpu_ctx, kinds=["residual"], slice_chunks=32)
    assert sorted(os.listdir(tmp_path)) == [f"stream{i}-residual.wav" for i in range(len(STREAMS))]
    for m, w in zip(got, ref["manifests"]["f32"]):
        assert [e["kind"] for e in m["kinds"]] == ["residual"]
        assert filecmp.cmp(m["kinds"][0]["file"], w["kinds"][2]["file"], shallow=False)


def test_unit_gains_leave_only_the_reconstruction_ripple(pkg, fv, tmp_path):
    # a model whose every gain is 1.0f (the weights of test_nsnet2_delay_host.py, through fvad_load_nsnet2_weights): the
    # denoised audio is the input 482 samples late but for the sqrt-Hann ripple, so on the samples the up-sampler copies
    # (2 modulo 3) the residual falls far below the original.  The oracle showed 0.0018 against 0.5, a factor of 280; 50 is asked.
    x = (np.random.default_rng(5).standard_normal((1, 4 * 24000 + 1234)) * 0.1).astype(np.float32)
    fv.wav_write(str(tmp_path / "noise.wav"), x)
    (tmp_path / "noise.txt").write_text("")
    (tmp_path / "plan.json").write_text(json.dumps({"instances": [{"name": "noise", "audio_path": "noise.wav", "ref_path": "noise.txt"}]}))
    ctx = fv.Context(0)
    try:
        ctx.load_weights(mc.unit_gain_weights(fv))
        got = pkg.simulator.run_denoise(str(tmp_path / "plan.json"), str(tmp_path / "out"), fmt="f32", ctx=ctx, kinds=("original", "residual"))
    finally:
        ctx.close()
    orig, res = (np.frombuffer(read(e["file"]), "<f4", offset=44) for e in got[0]["kinds"])
    assert orig.size == res.size == 4 * 24000
    n = np.arange(24000, orig.size)
    n = n[n % 3 == 2]
    print(f"unit gains: residual max {np.abs(res[n]).max():.4g}, original max {np.abs(orig[n]).max():.4g}")
    assert np.abs(res[n]).max() * 50.0 <= np.abs(orig[n]).max()
    assert np.array_equal(orig[482:], x[0, :orig.size - 482])
