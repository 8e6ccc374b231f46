"""simulator.run_clips(features=F, slice_chunks=16, features_sliced=True): the features of a run sliced in time (8 s slices), on
a `reproducible` context, against the unsliced run_clips(features=F) file by file -- the same file lists, every .npy and .wav
byte-identical, the manifests equal, features_skipped included -- for both families, plain and normalised.

The corpus is test_clips_sliced_gpu.py's in shape: a 60 s stereo stream and a 30 s mono stream, host ingest, f32 clips.  Where
the clips sit relative to the slice edges is asserted on the UNSLICED result, so that no comparison passes emptily: a clip with
features (a) wholly inside a slice, (b) across one edge, (c) with its pre-roll across an edge, and with max_speech_gap_sec 10
(d) across two edges."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

N, CHUNK = 16, 24000
E = N * CHUNK                      # a slice edge every 384 000 samples
PRE = 2 * 48000                    # the pre-roll of a segment


@pytest.fixture(scope="module")
def corpus(pkg, fv, tmp_path_factory):
    root = tmp_path_factory.mktemp("feat-sliced")
    synth = pkg.synth
    for name, (pcm, labels) in {"stereo": synth.make_stream(60.0, seed=41, n_channels=2), "mono": synth.make_stream(30.0, seed=300)}.items():
        fv.wav_write(str(root / f"{name}.wav"), pcm)
        (root / f"{name}.txt").write_text(synth.labels_to_audacity(labels))

    def plan(name, members, vad):
        insts = [{"name": m, "audio_path": f"{m}.wav", "ref_path": f"{m}.txt"} for m in members]
        (root / f"{name}.json").write_text(json.dumps({"instances": insts, "config": {"vad_config": {"vad_machine_config": vad}}}))
        return str(root / f"{name}.json")

    return {"default": plan("default", ["stereo", "mono"], {}), "merged": plan("merged", ["mono", "stereo"], {"max_speech_gap_sec": 10.0}), "root": root}


@pytest.fixture(scope="module")
def unsliced(pkg, gpu_ctx, corpus):
    """run_clips without slices, once per (plan, features, norm) -> (text, results, directory)"""
    cache = {}

    def get(plan, features, norm):
        key = (plan, features, norm)
        if key not in cache:
            out = corpus["root"] / f"unsliced-{plan}-{features}-{norm}"
            with gpu_ctx.options(reproducible="1"):
                text, results = pkg.simulator.run_clips(corpus[plan], str(out), ctx=gpu_ctx, features=features, features_norm=norm)
            cache[key] = (text, results, out)
        return cache[key]
    return get


def _same_as_unsliced(pkg, gpu_ctx, corpus, unsliced, plan, features, norm):
    text, results, ref_dir = unsliced(plan, features, norm)
    out = corpus["root"] / f"sliced-{plan}-{features}-{norm}"
    kw = {} if features is None else dict(features=features, features_norm=norm, features_sliced=True)
    with gpu_ctx.options(reproducible="1"):
        got_text, got = pkg.simulator.run_clips(corpus[plan], str(out), ctx=gpu_ctx, slice_chunks=N, **kw)
    assert got_text == text
    assert [r["segments"] for r in got] == [r["segments"] for r in results]
    assert [r["clips"] for r in got] == [r["clips"] for r in results]
    names = sorted(os.listdir(ref_dir))
    assert sorted(os.listdir(out)) == names
    n_npy = sum(n.endswith(".npy") for n in names)
    assert sum(n.endswith(".wav") for n in names) >= 2 and (n_npy >= 1 if features else n_npy == 0)
    for n in names:
        a, b = (ref_dir / n).read_bytes(), (out / n).read_bytes()
        if n.endswith(".json"):
            assert json.loads(a) == json.loads(b), n
        else:
            assert a == b, n
    for r in results:
        assert ("features_skipped" in r["clips"]) == (features is not None)
    return results


def _featured(results):
    """(from, to) of the segments whose clip has features"""
    return [(int(s[0]), int(s[1])) for r in results for s, c in zip(r["segments"], r["clips"]["clips"]) if "features" in c]


@pytest.mark.parametrize("features,norm", [("logmel", None), ("logmel", "whisper"), ("fbank", None), ("fbank", "cmn")])
def test_sliced_features_are_the_unsliced_files(pkg, gpu_ctx, corpus, unsliced, features, norm):
    results = _same_as_unsliced(pkg, gpu_ctx, corpus, unsliced, "default", features, norm)
    segs = _featured(results)
    assert len(segs) >= 4
    assert any(a // E == (b - 1) // E for a, b in segs), "(a) a clip with features wholly inside a slice"
    assert any((b - 1) // E == a // E + 1 for a, b in segs), "(b) a clip with features across one edge"
    assert any(a > 0 and a // E < (a + PRE) // E for a, b in segs), "(c) a clip with features whose pre-roll crosses an edge"
    suffix = {"logmel": ".logmel.npy", "fbank": ".fbank.npy"}[features]
    for r in results:
        for c in r["clips"]["clips"]:
            if "features" in c:
                assert "denoised" in c and c["features"]["file"] == c["denoised"]["file"].replace(".wav", suffix) and c["features"]["norm"] == norm
                assert c["features"]["first_sample"] % 3 == 2 and 0 <= c["features"]["first_sample"] - c["start"] < 3


def test_features_of_a_clip_across_several_edges(pkg, gpu_ctx, corpus, unsliced):
    results = _same_as_unsliced(pkg, gpu_ctx, corpus, unsliced, "merged", "logmel", None)
    assert any((b - 1) // E >= a // E + 2 for a, b in _featured(results)), "(d) a clip with features across two edges"


def test_without_features_the_sliced_run_writes_what_it_wrote(pkg, gpu_ctx, corpus, unsliced):
    results = _same_as_unsliced(pkg, gpu_ctx, corpus, unsliced, "default", None, None)
    assert all("features" not in c for r in results for c in r["clips"]["clips"])


def test_the_refusal_without_the_opt_in_stays(pkg, gpu_ctx, corpus):
    with pytest.raises(ValueError, match="split-source"):
        pkg.simulator.run_clips(corpus["default"], str(corpus["root"] / "never"), ctx=gpu_ctx, features="logmel", slice_chunks=N)
    assert not (corpus["root"] / "never").exists()
