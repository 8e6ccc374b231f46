"""simulator.run_clips(slice_chunks=16): the speech clips of a run sliced in time (8 s slices), on a `reproducible` context --
against the oracle's two recorders, and against the unsliced run_clips file by file: the WAV files byte-identical, the manifests,
segments and report equal, in both ingest modes and both output formats.

The plans are chosen so that the clips sit every way they can relative to the slice edges; each way is asserted on the UNSLICED
result, so that no comparison passes emptily:
  (a) wholly inside a slice; (b) across one edge; (c) its pre-roll reaching back across an edge at which the machine was closed;
  (d) across two edges and more (max_speech_gap_sec 10 merges the utterances of 18 .. 52 s into one segment);
  (e) reported before a slice's end and ending behind it (max_speech_gap_sec 0.5: a segment closes 0.5 s after its speech and
      ends 2 s after it), with the stream cut 100 samples behind a segment's end, inside a chunk: the original audio reaches
      that end, the denoised audio does not -- the skipped counts must be the unsliced run's."""
import json
import os

import numpy as np
import pytest

import orc
from test_clips_gpu import _oracle_margins_ok
from test_gpu import assert_audio

pytestmark = pytest.mark.gpu

N, CHUNK = 16, 24000
E = N * CHUNK                      # a slice edge every 384 000 samples
PRE = 2 * 48000                    # the pre-roll and the tail of a segment (VADMachine.zig:312-325)
CUT = 1820416 + 100                # 100 samples behind the third segment's end (test_clips_gpu.py)


@pytest.fixture(scope="module")
def corpus(pkg, fv, tmp_path_factory):
    """the files and plans: {plan name: path}, the stereo stream itself"""
    root = tmp_path_factory.mktemp("sliced")
    synth = pkg.synth
    stereo, labels2 = synth.make_stream(60.0, seed=41, n_channels=2)
    mono, labels1 = synth.make_stream(30.0, seed=300)
    files = {"stereo": (stereo, labels2), "mono": (mono, labels1), "cut": (np.ascontiguousarray(stereo[:, :CUT]), labels2)}
    for name, (pcm, labels) in files.items():
        fv.wav_write(str(root / f"{name}.wav"), pcm)
        (root / f"{name}.txt").write_text(synth.labels_to_audacity(labels))

    def plan(name, members, vad):
        insts = [{"name": m, "audio_path": f"{m}.wav", "ref_path": f"{m}.txt"} for m in members]
        (root / f"{name}.json").write_text(json.dumps({"instances": insts, "config": {"vad_config": {"vad_machine_config": vad}}}))
        return str(root / f"{name}.json")

    return {"default": plan("default", ["stereo", "mono"], {}), "merged": plan("merged", ["mono", "stereo"], {"max_speech_gap_sec": 10.0}),
            "short-gap": plan("short-gap", ["cut", "mono"], {"max_speech_gap_sec": 0.5}), "oracle": plan("oracle", ["stereo"], {}),
            "root": root, "stereo": stereo}


@pytest.fixture(scope="module")
def unsliced(pkg, gpu_ctx, corpus):
    """run_clips without slices, once per (plan, format) -> (text, results, directory)"""
    cache = {}

    def get(plan, pcm16):
        if (plan, pcm16) not in cache:
            out = corpus["root"] / f"unsliced-{plan}-{int(pcm16)}"
            with gpu_ctx.options(reproducible="1"):
                text, results = pkg.simulator.run_clips(corpus[plan], str(out), pcm16=pcm16, ctx=gpu_ctx)
            cache[(plan, pcm16)] = (text, results, out)
        return cache[(plan, pcm16)]
    return get


def _segments(results):
    return [(int(s[0]), int(s[1])) for r in results for s in r["segments"]]


def _same_as_unsliced(pkg, gpu_ctx, corpus, unsliced, plan, pcm16, ingest, tag, gap_sec=2.0):
    text, results, ref_dir = unsliced(plan, pcm16)
    out = corpus["root"] / f"sliced-{plan}-{tag}"
    info = {}
    with gpu_ctx.options(reproducible="1"):
        got_text, got = pkg.simulator.run_clips(corpus[plan], str(out), pcm16=pcm16, ctx=gpu_ctx, ingest=ingest, slice_chunks=N, info=info)
    assert got_text == text
    assert [r["segments"] for r in got] == [r["segments"] for r in results]
    assert [r["audit"] for r in got] == [r["audit"] for r in results]
    assert [r["clips"] for r in got] == [r["clips"] for r in results]
    names = sorted(os.listdir(ref_dir))
    assert sorted(os.listdir(out)) == names and sum(n.endswith(".wav") for n in names) >= 2
    for n in names:
        a, b = (ref_dir / n).read_bytes(), (out / n).read_bytes()
        if n.endswith(".json"):
            assert json.loads(a) == json.loads(b), n
        else:
            assert a == b, n
    # the held tails follow the clips, not the corpus: a lane holds at most the longest clip from its pre-roll to the frame that
    # closes it (max_speech_gap_sec behind its speech) and the slice that frame lies in -- in two buffers for each kind, for the
    # two lanes of the larger group
    longest = max(b - a for a, b in _segments(results))
    print("held tails:", info["held_peak_bytes"], "bytes at most;", info["slices"], "slices")
    assert 0 < info["held_peak_bytes"] <= 2 * 2 * 2 * (longest + int(gap_sec * 48000) + E + PRE) * 4 and info["slices"] >= 8
    return results


@pytest.mark.parametrize("pcm16", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("ingest", ["host", "device"])
def test_sliced_clips_are_the_unsliced_files(pkg, gpu_ctx, corpus, unsliced, ingest, pcm16):
    results = _same_as_unsliced(pkg, gpu_ctx, corpus, unsliced, "default", pcm16, ingest, f"{ingest}-{int(pcm16)}")
    segs = _segments(results)
    assert any(a // E == (b - 1) // E for a, b in segs), "(a) a clip wholly inside a slice"
    assert any((b - 1) // E == a // E + 1 for a, b in segs), "(b) a clip across one edge"
    # (c): the speech starts behind an edge (the machine was closed there) and the pre-roll begins in front of it
    assert any(a > 0 and a // E < (a + PRE) // E for a, b in segs), "(c) a pre-roll across an edge"
    assert all(r["clips"]["original_skipped"] == r["clips"]["denoised_skipped"] == 0 for r in results)
    assert all("original" in c and "denoised" in c for r in results for c in r["clips"]["clips"])


def test_a_clip_across_several_edges(pkg, gpu_ctx, corpus, unsliced):
    results = _same_as_unsliced(pkg, gpu_ctx, corpus, unsliced, "merged", False, "host", "host-0", gap_sec=10.0)
    assert any((b - 1) // E >= a // E + 2 for a, b in _segments(results)), "(d) a clip across two edges"


def test_a_clip_pending_past_a_slices_end_and_the_skipped_counts(pkg, gpu_ctx, corpus, unsliced):
    results = _same_as_unsliced(pkg, gpu_ctx, corpus, unsliced, "short-gap", False, "host", "host-0")
    # (e): the machine closes the segment 0.5 s (and at most a frame) after its speech, 1.5 s before the clip's end; an edge lies between
    assert any((b - PRE + 24000 + 1024) // E < (b - 1) // E for a, b in _segments(results)), "(e) a clip pending past a slice's end"
    m = results[0]["clips"]
    assert (m["original_skipped"], m["denoised_skipped"]) == (0, 1) and "denoised" not in m["clips"][2] and "original" in m["clips"][2]


def test_sliced_clips_match_the_oracle_recorders(pkg, fv, gpu_ctx, weights7, corpus):
    pcm = corpus["stereo"]
    ref = orc.Pipeline(weights7, n_channels=2, keep_denoised=True)
    ref.push(pcm)
    recs = ref.recordings()
    _oracle_margins_ok(ref.recordings_of(0), pcm)
    _oracle_margins_ok(ref.recordings_of(1), ref.denoised())
    out = corpus["root"] / "sliced-oracle"
    with gpu_ctx.options(reproducible="1"):
        _, results = pkg.simulator.run_clips(corpus["oracle"], str(out), ctx=gpu_ctx, slice_chunks=N)
    m = results[0]["clips"]
    assert len(m["clips"]) == len(recs) >= 2 and m["original_skipped"] == m["denoised_skipped"] == 0
    for c, (start, best_o, clip_o, best_d, clip_d) in zip(m["clips"], recs):
        for kind, best, clip in (("original", best_o, clip_o), ("denoised", best_d, clip_d)):
            assert (c["start"], c["length"], c[kind]["best_channel"]) == (start, len(clip), best), (kind, c["segment"])
        got_o, _ = fv.wav_read(str(out / c["original"]["file"]))
        got_d, _ = fv.wav_read(str(out / c["denoised"]["file"]))
        assert got_o[0].tobytes() == clip_o.tobytes()                    # original audio: bit-exact
        assert_audio(got_d[0], clip_d, what="denoised clip")
