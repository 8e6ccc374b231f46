"""simulator.run_clips(features="fbank") on a `reproducible` context, over the mono + stereo plan of the other clip harness tests
(90 s): features=None writes byte for byte what a call without the argument writes, and a logmel run's and a fbank run's WAV
files are the plain run's; with "fbank" every denoised clip of 400 samples or more at 16 kHz gains NAME-####-denoised.fbank.npy --
float32 [1 + (L - 400) // 160, 80] -- and a "features" entry in its manifest that states every parameter.  With
denoised_rate=16000 as f32 the written WAV holds exactly the samples the features were taken from, so each .npy must be (a) bit
for bit what a direct fvad_clips_export_fbank at step 1 gives over the WAV's own samples and (b) within clip_fbank_cases.TOL units
of the float64 model of those samples.  features_norm="cmn" stands in the exact numpy-float32 relation to the raw features."""
import json
import os

import numpy as np
import pytest

import clip_fbank_cases as fc

pytestmark = pytest.mark.gpu

FIELDS = {"file", "kind", "frames", "n_mels", "win_length", "n_fft", "hop", "sample_rate", "first_sample", "best_channel", "window", "preemph",
          "remove_dc", "scale", "snip_edges", "log", "floor", "norm", "mel"}
SHAPE = fc.SHAPES[0]


@pytest.fixture(scope="module")
def corpus(pkg, fv, tmp_path_factory):
    root = tmp_path_factory.mktemp("fbank")
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
        for tag, kw in (("plain", {}), ("none", dict(features=None)), ("logmel", dict(features="logmel")), ("fbank", dict(features="fbank")),
                        ("cmn", dict(features="fbank", features_norm="cmn"))):
            d = corpus / f"out-{tag}"
            out[tag] = (d, pkg.simulator.run_clips(str(corpus / "plan.json"), str(d), ctx=gpu_ctx, denoised_rate=16000, **kw))
    return out


def files(d):
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}


def wavs(fs):
    return {f: b for f, b in fs.items() if f.endswith(".wav")}


def test_nothing_else_changes_a_byte(runs):
    plain, none, logmel, fbank = (files(runs[t][0]) for t in ("plain", "none", "logmel", "fbank"))
    assert plain == none and runs["plain"][1][0] == runs["none"][1][0]
    assert not any(f.endswith(".npy") for f in plain)
    # with features the other files keep their bytes, the manifests apart; each kind writes its own .npy only
    assert wavs(logmel) == wavs(plain) and wavs(fbank) == wavs(plain) and wavs(files(runs["cmn"][0])) == wavs(plain)
    assert runs["logmel"][1][0] == runs["plain"][1][0] and runs["fbank"][1][0] == runs["plain"][1][0]
    assert not any(f.endswith(".fbank.npy") for f in logmel) and not any(f.endswith(".logmel.npy") for f in fbank)
    assert any(f.endswith(".fbank.npy") for f in fbank) and any(f.endswith(".logmel.npy") for f in logmel)
    # a logmel manifest says nothing new
    for r in runs["logmel"][1][1]:
        for c in r["clips"]["clips"]:
            if "features" in c:
                assert set(c["features"]) == {"file", "frames", "n_mels", "n_fft", "hop", "sample_rate", "first_sample", "best_channel", "max", "floor",
                                              "norm", "mel"}


def test_features_are_the_binding_call_and_the_model(fv, gpu_ctx, runs):
    d, (_, results) = runs["fbank"]
    w, M = fc.povey(400), fv.mel_design_kaldi(16000, 512, 80, 20, 0)   # the harness's own window and matrix
    assert M.tobytes() == fc.matrix_for(SHAPE).tobytes() or np.abs(M - fc.matrix_for(SHAPE)).max() <= 2.0 ** -23
    n_feat, worst = 0, 0.0
    for r in results:
        m = r["clips"]
        assert json.loads((d / f"{m['name']}-clips.json").read_text()) == m
        for c in m["clips"]:
            if "denoised" not in c:
                assert "features" not in c
                continue
            e, den = c.get("features"), c["denoised"]
            if den["length"] < 400:
                assert e is None
                continue
            assert set(e) == FIELDS and e["file"] == den["file"].replace(".wav", ".fbank.npy") and e["kind"] == "fbank"
            assert (e["n_mels"], e["win_length"], e["n_fft"], e["hop"], e["sample_rate"], e["norm"]) == (80, 400, 512, 160, 16000, None)
            assert (e["window"], e["preemph"], e["remove_dc"], e["scale"], e["snip_edges"], e["log"]) == ("povey", 0.97, True, 32768.0, True, "ln")
            assert e["floor"] == 2.0 ** -23 and e["mel"] == {"design": "kaldi", "low_freq": 20.0, "high_freq": 0.0}
            assert e["best_channel"] == den["best_channel"] and e["first_sample"] == den["first_sample"]
            x, sr = fv.wav_read(str(d / den["file"]))
            feat = np.load(d / e["file"])
            L = x.shape[1]
            T = 1 + (L - 400) // 160
            assert sr == 16000 and L == den["length"] and feat.dtype == np.float32 and feat.shape == (T, 80) and e["frames"] == T
            # (a) the binding on the WAV's own samples, at step 1: the same bits
            s = np.ascontiguousarray(x[0], np.float32)
            d_src = gpu_ctx.device_alloc(s.nbytes)
            try:
                gpu_ctx.to_device(d_src, s)
                res = gpu_ctx.clips_export_fbank(d_src, False, 1, L, L, [[0, 1, 0, L]], w, M)   # (the binding's defaults are Kaldi's)
            finally:
                gpu_ctx.device_free(d_src)
            assert res["out"].tobytes() == feat.tobytes(), e["file"]
            # (b) the float64 model of those samples
            ref, U = fc.model(s, w, M, SHAPE, scale=32768.0)
            worst = max(worst, fc.distance(feat, ref, U))
            n_feat += 1
        assert m["features_skipped"] == sum(1 for c in m["clips"] if "denoised" in c and "features" not in c)
    print(f"harness: worst distance {worst:.3f} units (tolerance {fc.TOL:.3f}) over {n_feat} clips")
    assert n_feat >= 4 and worst <= fc.TOL


def test_cmn_is_the_float32_formula(runs):
    (d_raw, (_, raw)), (d_n, (_, normed)) = runs["fbank"], runs["cmn"]
    F, n = fc.tile_frames(400, 160), 0
    for r, q in zip(raw, normed):
        for c, cn in zip(r["clips"]["clips"], q["clips"]["clips"]):
            if "features" not in c:
                assert "features" not in cn
                continue
            e, en = c["features"], cn["features"]
            assert en["norm"] == "cmn" and set(en) == FIELDS | {"means"}
            assert {k: v for k, v in en.items() if k not in ("norm", "means")} == {k: v for k, v in e.items() if k != "norm"}
            x, y = np.load(d_raw / e["file"]), np.load(d_n / en["file"])
            total = np.zeros(80, np.float32)
            for t0 in range(0, len(x), F):   # a tile's frames over ascending t, then the tiles in order, one division
                s = np.zeros(80, np.float32)
                for t in range(t0, min(t0 + F, len(x))):
                    s = s + x[t]
                total = total + s
            mean = total / np.float32(len(x))
            assert mean.dtype == np.float32 and np.array(en["means"], np.float32).tobytes() == mean.tobytes(), e["file"]
            assert y.tobytes() == (x - mean).tobytes(), e["file"]
            n += 1
    assert n >= 4
