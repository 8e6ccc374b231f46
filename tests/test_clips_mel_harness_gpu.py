"""simulator.run_clips(features="logmel") on a `reproducible` context, over the mono + stereo plan of the other clip harness tests (90 s): features=None
writes byte for byte what a call without the argument writes; with features every other file keeps its bytes and every denoised
clip gains NAME-####-denoised.logmel.npy -- float32 [L // 160, 80] for the clip's L samples at 16 kHz -- and a "features" entry
in its manifest.  With denoised_rate=16000 as f32 the written WAV holds exactly the samples the features were taken from, so
each .npy must be (a) bit for bit what a direct fvad_clips_export_mel at step 1 gives over the WAV's own samples and (b) within
clip_mel_cases.TOL units of the float64 model of those samples.  features_norm="whisper" stands in the exact numpy-float32
relation to the raw features."""
import json
import os

import numpy as np
import pytest

import clip_mel_cases as mc

pytestmark = pytest.mark.gpu

FIELDS = {"file", "frames", "n_mels", "n_fft", "hop", "sample_rate", "first_sample", "best_channel", "max", "floor", "norm", "mel"}


@pytest.fixture(scope="module")
def corpus(pkg, fv, tmp_path_factory):
    root = tmp_path_factory.mktemp("logmel")
    synth = pkg.synth
    for name, (pcm, labels) in {"stereo": synth.make_stream(60.0, seed=41, n_channels=2), "mono": synth.make_stream(30.0, seed=300)}.items():
        fv.wav_write(str(root / f"{name}.wav"), pcm)
        (root / f"{name}.txt").write_text(synth.labels_to_audacity(labels))
    insts = [{"name": m, "audio_path": f"{m}.wav", "ref_path": f"{m}.txt"} for m in ("stereo", "mono")]
    (root / "plan.json").write_text(json.dumps({"instances": insts, "config": {"vad_config": {"vad_machine_config": {}}}}))
    return root


@pytest.fixture(scope="module")
def runs(pkg, gpu_ctx, corpus):
    out = {}
    with gpu_ctx.options(reproducible="1"):
        for tag, kw in (("plain", {}), ("none", dict(features=None)), ("logmel", dict(features="logmel")),
                        ("whisper", dict(features="logmel", features_norm="whisper"))):
            d = corpus / f"out-{tag}"
            out[tag] = (d, pkg.simulator.run_clips(str(corpus / "plan.json"), str(d), ctx=gpu_ctx, denoised_rate=16000, **kw))
    return out


def files(d):
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}


def test_features_none_changes_no_byte(runs):
    plain, none = files(runs["plain"][0]), files(runs["none"][0])
    assert plain == none and runs["plain"][1][0] == runs["none"][1][0]
    assert not any(f.endswith(".npy") for f in plain)
    # with features the other files keep their bytes, the manifests apart
    logmel = files(runs["logmel"][0])
    assert {f: b for f, b in logmel.items() if f.endswith(".wav")} == {f: b for f, b in plain.items() if f.endswith(".wav")}
    assert runs["logmel"][1][0] == runs["plain"][1][0]


def test_features_are_the_binding_call_and_the_model(fv, gpu_ctx, runs):
    d, (_, results) = runs["logmel"]
    w, M = mc.hann(400), fv.mel_design(16000, 400, 80, 0, 8000)   # the harness's own window and matrix
    n_feat, worst = 0, 0.0
    for r in results:
        m = r["clips"]
        assert json.loads((d / f"{m['name']}-clips.json").read_text()) == m
        for c in m["clips"]:
            if "denoised" not in c:
                assert "features" not in c
                continue
            e, den = c.get("features"), c["denoised"]
            if den["length"] < 201:
                assert e is None
                continue
            assert set(e) == FIELDS and e["file"] == den["file"].replace(".wav", ".logmel.npy")
            assert (e["n_mels"], e["n_fft"], e["hop"], e["sample_rate"], e["floor"], e["norm"]) == (80, 400, 160, 16000, 1e-10, None)
            assert e["mel"] == {"design": "slaney", "fmin": 0.0, "fmax": 8000.0}
            assert e["best_channel"] == den["best_channel"] and e["first_sample"] == den["first_sample"]
            x, sr = fv.wav_read(str(d / den["file"]))
            feat = np.load(d / e["file"])
            L = x.shape[1]
            assert sr == 16000 and L == den["length"] and feat.dtype == np.float32 and feat.shape == (L // 160, 80) and e["frames"] == L // 160
            assert np.float32(e["max"]) == feat.max()
            # (a) the binding on the WAV's own samples, at step 1: the same bits
            s = np.ascontiguousarray(x[0], np.float32)
            d_src = gpu_ctx.device_alloc(s.nbytes)
            try:
                gpu_ctx.to_device(d_src, s)
                res = gpu_ctx.clips_export_mel(d_src, False, 1, L, L, [[0, 1, 0, L]], w, M)
            finally:
                gpu_ctx.device_free(d_src)
            assert res["out"].tobytes() == feat.tobytes(), e["file"]
            # (b) the float64 model of those samples
            ref, U = mc.model(s, w, M, 160)
            worst = max(worst, mc.distance(feat, ref, U))
            n_feat += 1
        assert m["features_skipped"] == sum(1 for c in m["clips"] if "denoised" in c and "features" not in c)
    print(f"harness: worst distance {worst:.3f} units (tolerance {mc.TOL:.3f}) over {n_feat} clips")
    assert n_feat >= 4 and worst <= mc.TOL


def test_whisper_norm_is_the_float32_formula(runs):
    (d_raw, (_, raw)), (d_n, (_, normed)) = runs["logmel"], runs["whisper"]
    n = 0
    for r, q in zip(raw, normed):
        for c, cn in zip(r["clips"]["clips"], q["clips"]["clips"]):
            if "features" not in c:
                continue
            e, en = c["features"], cn["features"]
            assert en["norm"] == "whisper" and en["max"] == e["max"] and {k: v for k, v in en.items() if k != "norm"} == {k: v for k, v in e.items() if k != "norm"}
            x, y = np.load(d_raw / e["file"]), np.load(d_n / en["file"])
            want = (np.maximum(x, x.max() - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25)
            assert want.dtype == np.float32 and y.tobytes() == want.tobytes(), e["file"]
            n += 1
    assert n >= 4
