"""simulator.run_clips(denoised_rate=16000, original_rate=16000) on a `reproducible` context: the clips at the denoiser's own rate
against the same call at 48000, file by file -- every 16 kHz file is the 48 kHz file's [skip::3] with skip from the manifest's
first_sample, says 16000 in its header, and has the 48 kHz file's pick and RMS values; the skipped counts are equal.  As f32 and
as PCM16, unsliced and in slices of 16 chunks (which cut clips across slice edges), and once with the files decoded on the device.

For the denoised f32 clips the dropped samples carried nothing: the interpolator's fused lerp (resample.zig:32-79,
test_gpu.py::test_nsnet2_denoise_other_input_rates_match_oracle's formula) of each kept sample and the one before it reproduces
the 48 kHz clip's two samples in between, wherever both lie in one 24 000-sample chunk."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, CHUNK = 16, 24000
E = N * CHUNK
NEW_KEYS = {"sample_rate", "first_sample", "length"}
PHASE = {"denoised": 2, "original": 0}


@pytest.fixture(scope="module")
def corpus(pkg, fv, tmp_path_factory):
    """the mono + stereo plan of test_clips_sliced_gpu.py"""
    root = tmp_path_factory.mktemp("rates")
    synth = pkg.synth
    for name, (pcm, labels) in {"stereo": synth.make_stream(60.0, seed=41, n_channels=2), "mono": synth.make_stream(30.0, seed=300)}.items():
        fv.wav_write(str(root / f"{name}.wav"), pcm)
        (root / f"{name}.txt").write_text(synth.labels_to_audacity(labels))
    insts = [{"name": m, "audio_path": f"{m}.wav", "ref_path": f"{m}.txt"} for m in ("stereo", "mono")]
    (root / "plan.json").write_text(json.dumps({"instances": insts, "config": {"vad_config": {"vad_machine_config": {}}}}))
    return root


def _lerp_between(d16, first_sample):
    """the two 48 kHz samples between kept samples m - 1 and m, for every m whose two kept samples lie in one chunk ->
    (m, [2][len(m)] float32)"""
    p = first_sample + 3 * np.arange(len(d16))
    m = np.flatnonzero(p[1:] // CHUNK == p[:-1] // CHUNK) + 1
    a, b = d16[m - 1], d16[m]
    out = []
    for j in range(2):
        t = np.float32(j + 1) / np.float32(3)
        out.append(((b - a).astype(np.float64) * np.float64(t) + a.astype(np.float64)).astype(np.float32))
    return m, out


@pytest.mark.parametrize("pcm16,slice_chunks,ingest", [(False, None, "host"), (True, None, "host"), (False, N, "host"), (True, N, "host"), (False, N, "device")],
                         ids=["f32", "pcm16", "f32-sliced", "pcm16-sliced", "f32-sliced-device"])
def test_clips_at_16k_are_every_third_sample_of_the_48k_clips(pkg, fv, gpu_ctx, corpus, pcm16, slice_chunks, ingest):
    tag = f"{int(pcm16)}-{slice_chunks}-{ingest}"
    dirs = {rate: corpus / f"out-{rate}-{tag}" for rate in (48000, 16000)}
    runs = {}
    with gpu_ctx.options(reproducible="1"):
        for rate, out in dirs.items():
            runs[rate] = pkg.simulator.run_clips(str(corpus / "plan.json"), str(out), pcm16=pcm16, ctx=gpu_ctx, ingest=ingest, slice_chunks=slice_chunks,
                                                 denoised_rate=rate, original_rate=rate)
    (text48, res48), (text16, res16) = runs[48000], runs[16000]
    assert text16 == text48 and [r["segments"] for r in res16] == [r["segments"] for r in res48]
    assert sorted(os.listdir(dirs[16000])) == sorted(os.listdir(dirs[48000]))
    read = fv.wav_read_i16 if pcm16 else fv.wav_read
    n_clips = n_lerp = 0
    across = False
    for r48, r16 in zip(res48, res16):
        m48, m16 = r48["clips"], r16["clips"]
        assert json.loads((dirs[16000] / f"{m16['name']}-clips.json").read_text()) == m16
        assert (m16["original_skipped"], m16["denoised_skipped"]) == (m48["original_skipped"], m48["denoised_skipped"])
        assert len(m16["clips"]) == len(m48["clips"]) >= 2
        for c48, c16 in zip(m48["clips"], m16["clips"]):
            assert (c16["segment"], c16["start"], c16["length"]) == (c48["segment"], c48["start"], c48["length"])
            across = across or c48["start"] // E != (c48["start"] + c48["length"] - 1) // E
            for kind in ("original", "denoised"):
                assert (kind in c16) == (kind in c48)
                if kind not in c48:
                    continue
                e48, e16 = c48[kind], c16[kind]
                assert not NEW_KEYS & set(e48)                             # a default-rate run has none of the new keys
                assert {k: e16[k] for k in e48} == e48                     # the file's name, the pick and both RMS values
                assert set(e16) == set(e48) | NEW_KEYS and e16["sample_rate"] == 16000
                skip = e16["first_sample"] - c48["start"]
                assert 0 <= skip < 3 and e16["first_sample"] % 3 == PHASE[kind]
                x48, sr48 = read(str(dirs[48000] / e48["file"]))
                x16, sr16 = read(str(dirs[16000] / e16["file"]))
                assert (sr48, sr16) == (48000, 16000) and x16.shape[0] == x48.shape[0] == 1
                assert x16[0].tobytes() == x48[0][skip::3].tobytes() and e16["length"] == x16.shape[1] == -(-(c48["length"] - skip) // 3)
                n_clips += 1
                if kind == "denoised" and not pcm16:
                    m, want = _lerp_between(x16[0], e16["first_sample"])
                    at = skip + 3 * (m - 1)                                # kept sample m - 1 in the 48 kHz clip
                    for j in range(2):
                        assert np.array_equal(x48[0][at + 1 + j], want[j]), (e48["file"], j)
                    n_lerp += len(m)
    assert n_clips >= 8 and (pcm16 or n_lerp > 10000)
    assert across or slice_chunks is None, "no clip lies across a slice edge"
