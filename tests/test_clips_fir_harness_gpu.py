"""simulator.run_clips(original_filter="fir" / denoised_filter="fir") on a `reproducible` context, on the plan of
test_clips_stride_harness_gpu.py: the filtered clips against the unfiltered runs, file by file.  A filtered 16 kHz run has the
unfiltered 16 kHz run's manifests but for the "filter" key and files of the same lengths, and every file is the model of
clip_fir_cases.py -- the 48 kHz file filtered as a finite signal with the default taps, centres [skip::3] -- within the rounding
bound of the f32 sum.  Unsliced, in slices of 16 chunks (which cut clips across slice edges) and with the files decoded on the
device the bytes are the same.  The denoised kind at 24000 and 8000, what run_clips refuses, and a default run's bytes."""
import json
import os

import numpy as np
import pytest

import clip_fir_cases as fc

pytestmark = pytest.mark.gpu

N, CHUNK = 16, 24000
E = N * CHUNK
STEPS = {24000: 2, 16000: 3, 8000: 6}


@pytest.fixture(scope="module")
def corpus(pkg, fv, tmp_path_factory):
    """the mono + stereo plan of test_clips_sliced_gpu.py"""
    root = tmp_path_factory.mktemp("fir")
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


def check_filtered_kind(fv, kind, rate, c48, c, d48, d, taps):
    """one clip's filtered entry and file against the 48 kHz run's -> the largest error in units of the bound"""
    e48, e = c48[kind], c[kind]
    step = STEPS[rate]
    assert {k: e[k] for k in e48} == e48                                   # the file's name, the pick and both RMS values
    assert e["sample_rate"] == rate and e["filter"] == {"design": "kaiser_sinc", "half": 16 * step, "cutoff": 0.45 / step, "beta": 6.0, "taps": 32 * step + 1}
    skip = e["first_sample"] - c48["start"]
    assert 0 <= skip < step
    x48, sr48 = fv.wav_read(str(d48 / e48["file"]))
    x, sr = fv.wav_read(str(d / e["file"]))
    assert (sr48, sr) == (48000, rate) and x.shape[0] == x48.shape[0] == 1
    assert e["length"] == x.shape[1] == -(-(c48["length"] - skip) // step)
    y, b = fc.fir_centres(x48[0], taps, skip, step)
    tol = fc.gamma(len(taps)) * b + np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
    err = np.abs(x[0].astype(np.float64) - y)
    assert np.all(err <= tol), (e["file"], int(np.argmax(err - tol)))
    return skip


def test_filtered_original_clips_at_16k(fv, runs):
    d48, text48, res48 = runs("48000")
    d16, text16, res16 = runs("16000-none", original_rate=16000, denoised_rate=16000)
    df, textf, resf = runs("16000-fir", original_rate=16000, denoised_rate=16000, original_filter="fir")
    assert textf == text16 == text48 and [r["segments"] for r in resf] == [r["segments"] for r in res48]
    assert sorted(os.listdir(df)) == sorted(os.listdir(d16))
    taps = fv.clips_fir_design(3)
    n_clips = 0
    for r48, r16, rf in zip(res48, res16, resf):
        m48, m16, mf = r48["clips"], r16["clips"], rf["clips"]
        assert json.loads((df / f"{mf['name']}-clips.json").read_text()) == mf
        # the manifests are the unfiltered 16 kHz run's but for the filter key of the original kind
        stripped = json.loads(json.dumps(mf))
        for c in stripped["clips"]:
            if "original" in c:
                assert "filter" in c["original"]
                del c["original"]["filter"]
            assert "denoised" not in c or "filter" not in c["denoised"]
        assert stripped == m16
        for c48, c16, cf in zip(m48["clips"], m16["clips"], mf["clips"]):
            if "denoised" in cf:                                           # the unfiltered kind's file is the unfiltered run's
                assert (df / cf["denoised"]["file"]).read_bytes() == (d16 / c16["denoised"]["file"]).read_bytes()
            if "original" not in cf:
                continue
            assert os.path.getsize(df / cf["original"]["file"]) == os.path.getsize(d16 / c16["original"]["file"])
            skip = check_filtered_kind(fv, "original", 16000, c48, cf, d48, df, taps)
            assert cf["original"]["first_sample"] % 3 == 0 and skip == c16["original"]["first_sample"] - c48["start"]
            n_clips += 1
    assert n_clips >= 4


@pytest.mark.parametrize("slice_chunks,ingest", [(N, "host"), (N, "device"), (None, "device")], ids=["sliced", "sliced-device", "device"])
def test_sliced_and_device_ingest_runs_write_the_same_bytes(runs, slice_chunks, ingest):
    df, textf, resf = runs("16000-fir", original_rate=16000, denoised_rate=16000, original_filter="fir")
    d, text, res = runs(f"16000-fir-{slice_chunks}-{ingest}", original_rate=16000, denoised_rate=16000, original_filter="fir", slice_chunks=slice_chunks, ingest=ingest)
    assert text == textf and files_of(d) == files_of(df)
    if slice_chunks:
        assert any(c["start"] // E != (c["start"] + c["length"] - 1) // E for r in res for c in r["clips"]["clips"]), "no clip lies across a slice edge"


def test_both_kinds_filtered_at_24k_and_8k(fv, runs):
    d48, text48, res48 = runs("48000")
    for tag, o_rate, d_rate in (("24-8", 24000, 8000), ("8-24", 8000, 24000)):
        d, text, res = runs(tag, original_rate=o_rate, denoised_rate=d_rate, original_filter="fir", denoised_filter="fir", slice_chunks=N if tag == "8-24" else None)
        assert text == text48
        n = 0
        for r48, r in zip(res48, res):
            for c48, c in zip(r48["clips"]["clips"], r["clips"]["clips"]):
                for kind, rate in (("original", o_rate), ("denoised", d_rate)):
                    assert (kind in c) == (kind in c48)
                    if kind in c:
                        check_filtered_kind(fv, kind, rate, c48, c, d48, d, fv.clips_fir_design(STEPS[rate]))
                        assert c[kind]["first_sample"] % STEPS[rate] == 0
                        n += 1
        assert n >= 8


def test_what_run_clips_refuses_is_refused_before_any_work(pkg, gpu_ctx, corpus):
    out = corpus / "out-refused"
    for kw in (dict(original_rate=48000, original_filter="fir"), dict(denoised_filter="fir"), dict(original_rate=24000), dict(denoised_rate=8000),
               dict(original_rate=44100, original_filter="fir"), dict(original_rate=16000, original_filter="iir"),
               dict(denoised_rate=24000, original_filter="fir", original_rate=16000)):
        with pytest.raises(ValueError):
            pkg.simulator.run_clips(str(corpus / "no-such-plan.json"), str(out), ctx=gpu_ctx, **kw)   # (the plan is never opened)
    assert not out.exists()


def test_a_default_run_writes_what_it_wrote(runs):
    d48, text48, _ = runs("48000")                                         # only the arguments run_clips had before
    d, text, _ = runs("48000-explicit", denoised_rate=48000, original_rate=48000, original_filter="none", denoised_filter="none")
    assert text == text48 and files_of(d) == files_of(d48)
    assert b'"filter"' not in b"".join(v for f, v in files_of(d).items() if f.endswith(".json"))
    d16, _, _ = runs("16000-none", original_rate=16000, denoised_rate=16000)
    d16e, _, _ = runs("16000-explicit", original_rate=16000, denoised_rate=16000, original_filter="none", denoised_filter="none")
    assert files_of(d16e) == files_of(d16)
