"""simulator.run_clips(original_filter="resample" / denoised_filter="resample") on a `reproducible` context, on the small plan of
test_clips_fir_harness_gpu.py (a 60 s stereo and a 30 s mono file, rebuilt here): original clips at 44100 and denoised clips at
22050 against the 48000 run, file by file.  Every file is the float64 model of clip_resample_cases.py / ingest_resample_cases.py
-- the 48 kHz file resampled as a finite signal with fvad_resample_design's default taps -- within the rounding bound of the f32
sum; headers, lengths and manifests carry the rates; segments and report are the 48000 run's.  Sliced (the smallest slice the
plan's frame size allows, 16 chunks, and 48 chunks) and with the files decoded on the device the bytes are the same; a PCM16
run's files are the f32 run's samples converted; what run_clips refuses with "resample"; and default and "fir" runs' bytes."""
import json
import os

import numpy as np
import pytest

import clip_cases as cc
import ingest_resample_cases as rr

pytestmark = pytest.mark.gpu

CHUNK = 24000
RATES = {"original": 44100, "denoised": 22050}
RATIOS = {44100: (147, 160), 22050: (147, 320)}
KW = dict(original_filter="resample", original_rate=44100, denoised_filter="resample", denoised_rate=22050)


@pytest.fixture(scope="module")
def corpus(pkg, fv, tmp_path_factory):
    root = tmp_path_factory.mktemp("resample")
    synth = pkg.synth
    for name, (pcm, labels) in {"stereo": synth.make_stream(60.0, seed=41, n_channels=2), "mono": synth.make_stream(30.0, seed=300)}.items():
        fv.wav_write(str(root / f"{name}.wav"), pcm)
        (root / f"{name}.txt").write_text(synth.labels_to_audacity(labels))
    insts = [{"name": m, "audio_path": f"{m}.wav", "ref_path": f"{m}.txt"} for m in ("stereo", "mono")]
    (root / "plan.json").write_text(json.dumps({"instances": insts, "config": {"vad_config": {"vad_machine_config": {}}}}))
    return root


@pytest.fixture(scope="module")
def runs(pkg, gpu_ctx, corpus):
    """run_clips once per distinct set of arguments -> (directory, text, results)"""
    cache = {}

    def get(tag, **kw):
        if tag not in cache:
            out = corpus / f"out-{tag}"
            with gpu_ctx.options(reproducible="1"):
                text, res = pkg.simulator.run_clips(str(corpus / "plan.json"), str(out), ctx=gpu_ctx, **kw)
            cache[tag] = (out, text, res)
        return cache[tag]
    return get


def files_of(d):
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}


def test_resampled_clips_against_the_48k_run(fv, runs):
    d48, text48, res48 = runs("48000")
    d, text, res = runs("resample", **KW)
    assert text == text48 and [r["segments"] for r in res] == [r["segments"] for r in res48]
    designs = {rate: fv.resample_design(*RATIOS[rate]) for rate in RATIOS}
    assert [len(designs[r]) for r in (44100, 22050)] == [5121, 10241]
    n_clips = 0
    for r48, r in zip(res48, res):
        m48, m = r48["clips"], r["clips"]
        assert json.loads((d / f"{m['name']}-clips.json").read_text()) == m
        assert {k: v for k, v in m.items() if k != "clips"} == {k: v for k, v in m48.items() if k != "clips"}
        for c48, c in zip(m48["clips"], m["clips"]):
            assert (c["segment"], c["start"], c["length"]) == (c48["segment"], c48["start"], c48["length"])
            for kind, rate in RATES.items():
                assert (kind in c) == (kind in c48)
                if kind not in c:
                    continue
                up, down = RATIOS[rate]
                e48, e, taps = c48[kind], c[kind], designs[rate]
                assert {k: e[k] for k in e48} == e48                       # the file's name, the pick and both RMS values
                assert e["sample_rate"] == rate and e["first_sample"] == c48["start"]
                assert e["filter"] == {"design": "kaiser_sinc_polyphase", "up": up, "down": down, "half": 16, "cutoff": 0.45 / down, "beta": 6.0,
                                       "taps": 32 * down + 1}
                x48, sr48 = fv.wav_read(str(d48 / e48["file"]))
                x, sr = fv.wav_read(str(d / e["file"]))
                assert (sr48, sr) == (48000, rate) and x.shape[0] == x48.shape[0] == 1 and x48.shape[1] == c48["length"]
                assert e["length"] == x.shape[1] == -(-c48["length"] * up // down)
                y, b = rr.resample_model(x48[0].astype(np.float64)[:, None], taps, up, down, 0, x.shape[1])
                rr.compare(np.ascontiguousarray(x[:1]), y, b, up, len(taps), e["file"])
                n_clips += 1
    assert n_clips >= 8


@pytest.mark.parametrize("slice_chunks,ingest", [(16, "host"), (48, "host"), (16, "device"), (None, "device")],
                         ids=["sliced-16", "sliced-48", "sliced-device", "device"])
def test_sliced_and_device_ingest_runs_write_the_same_bytes(runs, slice_chunks, ingest):
    d0, text0, _ = runs("resample", **KW)
    d, text, res = runs(f"resample-{slice_chunks}-{ingest}", slice_chunks=slice_chunks, ingest=ingest, **KW)
    assert text == text0 and files_of(d) == files_of(d0)
    if slice_chunks:
        E = slice_chunks * CHUNK
        assert any(c["start"] // E != (c["start"] + c["length"] - 1) // E for r in res for c in r["clips"]["clips"]), "no clip lies across a slice edge"


def test_a_pcm16_run_is_the_f32_run_converted(fv, runs):
    d0, _, res0 = runs("resample", **KW)
    d, _, res = runs("resample-pcm16", pcm16=True, **KW)
    n = 0
    for r0, r in zip(res0, res):
        for c0, c in zip(r0["clips"]["clips"], r["clips"]["clips"]):
            for kind, rate in RATES.items():
                if kind not in c:
                    continue
                assert {k: v for k, v in c[kind].items()} == {k: v for k, v in c0[kind].items()}
                x0, _ = fv.wav_read(str(d0 / c0[kind]["file"]))
                x, sr = fv.wav_read_i16(str(d / c[kind]["file"]))
                assert sr == rate and x[0].tobytes() == cc.convert(x0[0], True).tobytes()
                n += 1
    assert n >= 8


def test_what_run_clips_refuses_with_resample_is_refused_before_any_work(pkg, gpu_ctx, corpus):
    out = corpus / "out-refused"
    for kw in (dict(original_rate=48000, original_filter="resample"), dict(denoised_filter="resample"),
               dict(original_rate=44101, original_filter="resample"), dict(original_rate=0, original_filter="resample"),
               dict(denoised_rate="44100", denoised_filter="resample"), dict(denoised_rate=-44100, denoised_filter="resample"),
               dict(original_rate=44100.0, original_filter="resample"), dict(original_rate=1, original_filter="resample"),
               dict(original_rate=44100), dict(denoised_rate=44100), dict(original_rate=44100, original_filter="fir"),
               dict(original_rate=44100, original_filter="resampled")):
        with pytest.raises(ValueError):
            pkg.simulator.run_clips(str(corpus / "no-such-plan.json"), str(out), ctx=gpu_ctx, **kw)   # (the plan is never opened)
    assert not out.exists()


def test_the_other_rates_run(fv, runs):
    """32000 and 11025, and the rates the FIR gather offers too: headers and lengths"""
    d48, _, res48 = runs("48000")
    for tag, o_rate, d_rate in (("32-11", 32000, 11025), ("16-8", 16000, 8000)):
        d, _, res = runs(f"resample-{tag}", original_filter="resample", original_rate=o_rate, denoised_filter="resample", denoised_rate=d_rate)
        for r48, r in zip(res48, res):
            for c48, c in zip(r48["clips"]["clips"], r["clips"]["clips"]):
                for kind, rate in (("original", o_rate), ("denoised", d_rate)):
                    if kind in c:
                        x, sr = fv.wav_read(str(d / c[kind]["file"]))
                        up, down = fv.resample_ratio(48000, rate)
                        assert sr == rate and x.shape[1] == c[kind]["length"] == -(-c48["length"] * up // down) and np.isfinite(x).all()


def test_default_and_fir_runs_write_what_they_wrote(runs):
    d48, text48, _ = runs("48000")                                         # only the arguments run_clips had before
    d, text, _ = runs("48000-explicit", denoised_rate=48000, original_rate=48000, original_filter="none", denoised_filter="none")
    assert text == text48 and files_of(d) == files_of(d48)
    assert b'"filter"' not in b"".join(v for f, v in files_of(d).items() if f.endswith(".json"))
    # a "fir" run: the manifest's filter entry has the keys it had, and the resampled run at the same rate has the same pick
    df, textf, resf = runs("16000-fir", original_rate=16000, denoised_rate=16000, original_filter="fir")
    assert textf == text48
    for r in resf:
        for c in r["clips"]["clips"]:
            if "original" in c:
                assert c["original"]["filter"] == {"design": "kaiser_sinc", "half": 48, "cutoff": 0.45 / 3, "beta": 6.0, "taps": 97}
            assert "denoised" not in c or "filter" not in c["denoised"]
    df2, _, _ = runs("16000-fir-again", original_rate=16000, denoised_rate=16000, original_filter="fir", denoised_filter="none")
    assert files_of(df2) == files_of(df)
