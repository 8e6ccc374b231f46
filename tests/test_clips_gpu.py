"""The batch Recorder on the GPU (fvad_clips_export_device / fvad_clips_export, csrc/kernels_clips.hip) against the float64
model and the case table of clip_cases.py, against the CPU oracle's recorders, and through simulator.run_clips.

Sources are 12 lanes of 120 000 samples with NaN (f32) or a sentinel (PCM16) everywhere outside the clips' ranges -- a kernel
that used a sample it must not read would show it --, the lanes an odd stride apart so that no lane start is 16-byte aligned;
the device output is filled with canaries that must survive everywhere outside the clips' samples."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import clip_cases as cc
import orc
from test_gpu import assert_audio

pytestmark = pytest.mark.gpu

INVALID, OUT_OF_RANGE, TOO_SMALL = -100, -6, -106
STRIDE = cc.N_SAMPLES + 5
CANARY = {False: np.frombuffer(np.uint32(0x7FC0BEEF).tobytes(), np.float32)[0], True: np.int16(0x5A5A)}
SLACK = 64            # canary samples behind the plan's total


class Device:
    """the case table's source in one format on the device, and a canary-filled output buffer"""

    def __init__(self, ctx, pcm16):
        self.ctx, self.pcm16 = ctx, pcm16
        self.clips, self.names = cc.case_table()
        self.src = cc.mask_outside(cc.make_source(pcm16), self.clips)
        host = np.full((cc.N_LANES, STRIDE), cc.SENTINEL if pcm16 else np.nan, self.src.dtype)
        host[:, :cc.N_SAMPLES] = self.src
        self.d_src = ctx.device_alloc(host.nbytes)
        ctx.to_device(self.d_src, host)
        self.cap = 4000000 + SLACK    # (the table's clips are 0.4 M samples; 300 of them at random stay below 4 M)
        self.d_out = ctx.device_alloc(self.cap * 4)
        self.host_out = np.zeros(1024, np.float32)   # for the host form's refused calls (never written)

    def close(self):
        self.ctx.device_free(self.d_src)
        self.ctx.device_free(self.d_out)

    def fill(self, out_pcm16):
        self.ctx.to_device(self.d_out, np.full(self.cap, CANARY[out_pcm16], np.int16 if out_pcm16 else np.float32))

    def read(self, out_pcm16):
        return self.ctx.to_host(np.zeros(self.cap, np.int16 if out_pcm16 else np.float32), self.d_out)

    def export(self, clips, out_pcm16):
        """fvad_clips_export_device into the canary-filled buffer -> the result with `samples` cut from the output, after
        checking that every sample outside the clips' is still a canary"""
        self.fill(out_pcm16)
        clips = np.asarray(clips, np.uint64).reshape(-1, 4)
        res = self.ctx.clips_export(self.d_src, self.pcm16, cc.N_LANES, STRIDE, cc.N_SAMPLES, clips, out_pcm16=out_pcm16,
                                    d_out=self.d_out, out_capacity=self.cap)
        out = self.read(out_pcm16)
        touched = np.zeros(self.cap, bool)
        res["samples"] = []
        for (_, _, a, b), o in zip(clips.astype(np.int64), res["offsets"].astype(np.int64)):
            res["samples"].append(out[o:o + b - a].copy())
            touched[o:o + b - a] = True
        assert out[~touched].tobytes() == np.full(int((~touched).sum()), CANARY[out_pcm16], out.dtype).tobytes(), "a canary outside the clips' samples changed"
        return res

    def raw(self, clips, out_pcm16=False, d_src="own", src_format=None, n_lanes=cc.N_LANES, n_samples=cc.N_SAMPLES, d_out="own",
            cap=None, out_format=None, host=False):
        """the C call itself -> status"""
        fv = self.ctx_binding
        clips = np.ascontiguousarray(np.asarray(clips, np.uint64).reshape(-1, 4))
        fn = fv.lib().fvad_clips_export if host else fv.lib().fvad_clips_export_device
        return fn(self.ctx.h, fv.vp(self.d_src if d_src == "own" else d_src), int(self.pcm16) if src_format is None else src_format,
                  n_lanes, STRIDE, n_samples, clips.ctypes.data_as(C.POINTER(C.c_uint64)) if len(clips) else None, len(clips),
                  int(out_pcm16) if out_format is None else out_format,
                  fv.vp((self.host_out.ctypes.data if host else self.d_out) if d_out == "own" else d_out),
                  self.cap if cap is None else cap, None, None, None, None)


@pytest.fixture(scope="module", params=[False, True], ids=["from-f32", "from-pcm16"])
def dev(request, fv, gpu_ctx):
    d = Device(gpu_ctx, request.param)
    d.ctx_binding = fv
    yield d
    d.close()


@pytest.fixture(scope="module")
def expected():
    """the model's results, computed once per format pair"""
    cache = {}

    def get(dev, out_pcm16):
        key = (dev.pcm16, out_pcm16)
        if key not in cache:
            cache[key] = cc.model_export(dev.src, dev.clips, out_pcm16)
        return cache[key]
    return get


@pytest.mark.parametrize("out_pcm16", [False, True], ids=["to-f32", "to-pcm16"])
def test_case_table_matches_the_model(dev, expected, out_pcm16):
    # every length, alignment, tile boundary, channel count, overlap and duplicate of the table, in all four format pairs:
    # picks, offsets and sample bits exact (equal formats: the source's bits; the two conversions: the rules in numpy, bit for
    # bit), both RMS within one f32 ulp
    got = dev.export(dev.clips, out_pcm16)
    want = expected(dev, out_pcm16)
    print("max |rms - model| in ulps:", np.max(np.abs(got["best_rms"].astype(np.float64) - want["best_rms"]) / np.maximum(np.spacing(want["best_rms"]), 1e-45)))
    cc.compare(got, want, f"pcm16 {dev.pcm16} -> {out_pcm16}")
    if dev.pcm16 == out_pcm16:
        for (l0, _, a, b), ch, s in zip(dev.clips.astype(np.int64), got["best_channel"], got["samples"]):
            assert s.tobytes() == dev.src[l0 + ch, a:b].tobytes()


def test_the_pick_and_silence(dev):
    got = dev.export(dev.clips, False)
    for s, (_, C_) in cc.STREAMS.items():
        for p in range(C_):                                   # the channel scaled by 1 - 2^-10, in every position
            i = dev.names[f"scaled-{s}-{p}"]
            assert got["best_channel"][i] == p and (C_ == 1 or got["best_rms"][i] < got["runner_up_rms"][i])
        i = dev.names[f"tie-{s}"]                             # a negated copy is an exact tie: the lower index stands
        assert got["best_channel"][i] == (0 if C_ <= 2 else 1) and got["runner_up_rms"][i].tobytes() == got["best_rms"][i].tobytes()
    i = dev.names["silence"]                                  # digital silence: exactly +0.0, channel 0
    zero = np.float32(0.0).tobytes()
    assert got["best_channel"][i] == 0 and got["best_rms"][i].tobytes() == zero and got["runner_up_rms"][i].tobytes() == zero


@pytest.mark.parametrize("out_pcm16", [False, True], ids=["to-f32", "to-pcm16"])
def test_a_clip_is_the_same_bits_whatever_else_is_in_the_call(dev, out_pcm16):
    rng = np.random.default_rng(11)
    table = dev.clips
    for name in ("dup", "last", f"tie-D"):
        i = dev.names[name]
        alone = dev.export(table[i:i + 1], out_pcm16)
        others = table[rng.integers(0, len(table), 300)]
        at = 137
        among = dev.export(np.concatenate([others[:at], table[i:i + 1], others[at:]]), out_pcm16)
        rev = dev.export(table[::-1], out_pcm16)
        j = len(table) - 1 - i
        for res, k in ((among, at), (rev, j)):
            for f in ("best_channel", "best_rms", "runner_up_rms"):
                assert res[f][k].tobytes() == alone[f][0].tobytes(), (name, f)
            assert res["samples"][k].tobytes() == alone["samples"][0].tobytes(), name
    a, b = dev.export(table, out_pcm16), dev.export(table, out_pcm16)        # two identical calls: identical bits
    assert all(a[f].tobytes() == b[f].tobytes() for f in ("best_channel", "best_rms", "runner_up_rms", "offsets"))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a["samples"], b["samples"]))


def test_host_export_equals_device_export(dev):
    for out_pcm16 in (False, True):
        d = dev.export(dev.clips, out_pcm16)
        h = dev.ctx.clips_export(dev.d_src, dev.pcm16, cc.N_LANES, STRIDE, cc.N_SAMPLES, dev.clips, out_pcm16=out_pcm16)
        assert all(h[f].tobytes() == d[f].tobytes() for f in ("best_channel", "best_rms", "runner_up_rms", "offsets"))
        touched = np.zeros(h["total"], bool)
        for (_, _, a, b), o, s in zip(dev.clips.astype(np.int64), h["offsets"].astype(np.int64), d["samples"]):
            assert h["out"][o:o + b - a].tobytes() == s.tobytes()
            touched[o:o + b - a] = True
        assert not h["out"][~touched].any()                   # the padding between slots comes back as zeros


def test_errors_come_back_before_any_launch(dev, fv):
    dev.fill(False)
    ok = [(1, 1, 0, 100), (2, 2, 50, 60)]
    l0, C_ = cc.STREAMS["D"]
    for what, status, kw in (
            ("sample_to past n_samples", OUT_OF_RANGE, dict(clips=[ok[0], (1, 1, 10, cc.N_SAMPLES + 1)])),
            ("lanes past n_lanes", OUT_OF_RANGE, dict(clips=[ok[0], (l0 + 1, C_, 0, 10)])),
            ("first_lane past n_lanes", OUT_OF_RANGE, dict(clips=[(cc.N_LANES, 1, 0, 10)])),
            ("capacity below the plan's total", TOO_SMALL, dict(clips=ok, cap=111)),
            ("NULL source", INVALID, dict(clips=ok, d_src=0)),
            ("NULL output", INVALID, dict(clips=ok, d_out=0)),
            ("bad source format", INVALID, dict(clips=ok, src_format=2)),
            ("bad output format", INVALID, dict(clips=ok, out_format=-1)),
            ("misaligned output", INVALID, dict(clips=ok, d_out=dev.d_out + 4)),
            ("sample_to <= sample_from", INVALID, dict(clips=[ok[0], (1, 1, 10, 10)])),
            ("no channels", INVALID, dict(clips=[ok[0], (1, 0, 10, 20)]))):
        assert dev.raw(**kw) == status, what
        if "d_out" not in kw or kw["d_out"] == 0:             # (a host buffer has no alignment rule)
            assert dev.raw(host=True, **dict(kw, cap=min(kw.get("cap", 1024), 1024))) == status, what + " (host form)"
    assert dev.raw([]) == 0 and dev.raw([], host=True) == 0   # no clips: nothing to do
    out = dev.read(False)
    assert out.tobytes() == np.full(dev.cap, CANARY[False], np.float32).tobytes()   # every canary untouched by the refused calls
    assert not dev.host_out.any()
    assert dev.raw(ok, cap=112) == 0                          # exactly the plan's total: 100 + 12 (a slot of 10, padded)


def test_kernel_times_name_the_three_kernels(dev):
    dev.ctx.enable_timing(True)
    try:
        dev.ctx.kernel_times()                                # (drop what earlier calls left)
        dev.export(dev.clips, False)
        times = dev.ctx.kernel_times()
    finally:
        dev.ctx.enable_timing(False)
    assert {"clip_rms", "clip_pick", "clip_gather"} <= set(times) and all(times[k] > 0 for k in ("clip_rms", "clip_pick", "clip_gather"))


# ------------------------------------------------------------------ against the oracle's two recorders
def _engine_segments(fv, ctx, pcm, overrides=None):
    """the engine's segments and denoised audio of one stream: fvad_engine_run, then the host VAD stage"""
    res = ctx.engine_run([pcm[c] for c in range(pcm.shape[0])], want_denoised=True)
    vb = fv.VadBatch(1, n_channels=pcm.shape[0], overrides=overrides)
    try:
        segs = vb.run(np.stack([r["band_sum"] for r in res]), np.stack([r["chunk_rms"] for r in res]))[0]
    finally:
        vb.close()
    return segs, np.stack([r["denoised"] for r in res])


def _export_both(fv, ctx, pcm, den, segs):
    """both exports of one stream's segments from device-resident lanes (lane 0 is a dummy: first_lane = 1)"""
    out = {}
    for kind, audio in (("original", pcm), ("denoised", den)):
        n = audio.shape[1]
        host = np.zeros((audio.shape[0] + 1, n), np.float32)
        host[1:] = audio
        d = ctx.device_alloc(host.nbytes)
        try:
            ctx.to_device(d, host)
            clips, skipped = fv.clips_from_segments(segs, 1, audio.shape[0], n)
            res = ctx.clips_export(d, False, host.shape[0], n, n, clips)
        finally:
            ctx.device_free(d)
        res["clips"], res["skipped"] = clips, skipped
        res["samples"] = [res["out"][int(o):int(o) + int(c[3] - c[2])] for c, o in zip(clips, res["offsets"])]
        out[kind] = res
    return out


def _oracle_margins_ok(recs, audio):
    # the oracle picks by a sequential f32 sum, the library by f64: its pick is only a yardstick where the two channels' RMS
    # differ by at least 1 % (they do: the synthetic stream gives channel 1 a gain of 0.6 .. 0.9)
    for start, _, clip in recs:
        r = [np.sqrt(np.mean(audio[c, start:start + len(clip)].astype(np.float64) ** 2)) for c in range(audio.shape[0])]
        assert abs(r[0] - r[1]) >= 0.01 * min(r), (start, r)


def test_clips_match_the_oracle_recorders(fv, gpu_ctx, weights7, pkg):
    pcm, _ = pkg.synth.make_stream(60.0, seed=41, n_channels=2)      # test_pipeline_recordings_match_oracle's stream
    ref = orc.Pipeline(weights7, n_channels=2, keep_denoised=True)
    ref.push(pcm)
    recs = ref.recordings()
    _oracle_margins_ok(ref.recordings_of(0), pcm)
    _oracle_margins_ok(ref.recordings_of(1), ref.denoised())
    segs, den = _engine_segments(fv, gpu_ctx, pcm)
    got = _export_both(fv, gpu_ctx, pcm, den, segs)
    assert len(recs) == len(segs) >= 2 and got["original"]["skipped"] == got["denoised"]["skipped"] == 0
    for k, (start, best_o, clip_o, best_d, clip_d) in enumerate(recs):
        for kind, best, clip in (("original", best_o, clip_o), ("denoised", best_d, clip_d)):
            g = got[kind]
            assert (int(g["clips"][k][2]), int(g["clips"][k][3] - g["clips"][k][2]), int(g["best_channel"][k])) == (start, len(clip), best), (kind, k)
        assert got["original"]["samples"][k].tobytes() == clip_o.tobytes()                 # original audio: bit-exact
        d = got["denoised"]
        assert d["samples"][k].tobytes() == den[d["best_channel"][k], start:start + len(clip_d)].tobytes()   # the engine's own bits
        assert_audio(d["samples"][k], clip_d, what="denoised clip")


def test_a_segment_past_the_denoised_end_has_no_denoised_clip(fv, gpu_ctx, weights7, pkg):
    # max_speech_gap_sec 0.5: a segment closes 0.5 s after its speech and ends 2 s after it (VADMachine.zig:319-323).  The stream
    # is cut 100 samples behind the third segment's end, inside a chunk: the original audio reaches that end, the denoised audio
    # (whole chunks) does not -- one clip fewer on the denoised side, as the oracle's denoised recorder has
    ov = {"max_speech_gap_sec": 0.5}
    pcm, _ = pkg.synth.make_stream(60.0, seed=41, n_channels=2)
    pcm = np.ascontiguousarray(pcm[:, :1820416 + 100])
    ref = orc.Pipeline(weights7, n_channels=2, keep_denoised=True, vad_overrides=ov)
    ref.push(pcm)
    ro, rd = ref.recordings_of(0), ref.recordings_of(1)
    assert len(ro) == 3 and len(rd) == 2
    _oracle_margins_ok(ro, pcm)
    _oracle_margins_ok(rd, ref.denoised())
    segs, den = _engine_segments(fv, gpu_ctx, pcm, overrides=ov)
    assert den.shape[1] < segs[2][1] <= pcm.shape[1]
    got = _export_both(fv, gpu_ctx, pcm, den, segs)
    assert (got["original"]["skipped"], got["denoised"]["skipped"]) == (0, 1)
    for kind, recs in (("original", ro), ("denoised", rd)):
        g = got[kind]
        assert len(g["samples"]) == len(recs)
        for k, (start, best, clip) in enumerate(recs):
            assert (int(g["clips"][k][2]), len(g["samples"][k]), int(g["best_channel"][k])) == (start, len(clip), best), (kind, k)
            if kind == "original":
                assert g["samples"][k].tobytes() == clip.tobytes()
            else:
                assert_audio(g["samples"][k], clip, what="denoised clip")


# ------------------------------------------------------------------ the harness
@pytest.mark.parametrize("pcm16", [False, True], ids=["f32", "pcm16"])
def test_run_clips_writes_the_plans_clips(pkg, fv, gpu_ctx, tmp_path, pcm16):
    synth, sim = pkg.synth, pkg.simulator
    insts, audio = [], []
    for i, nch in enumerate((1, 2)):                                  # one mono and one stereo instance, 30 s each
        pcm, labels = synth.make_stream(30.0, seed=300 + i, n_channels=nch)
        fv.wav_write(str(tmp_path / f"s{i}.wav"), pcm)
        (tmp_path / f"s{i}.txt").write_text(synth.labels_to_audacity(labels))
        insts.append({"name": f"stream{i}", "audio_path": f"s{i}.wav", "ref_path": f"s{i}.txt"})
        audio.append(pcm)
    (tmp_path / "plan.json").write_text(json.dumps({"instances": insts, "config": {"vad_config": {}}}))
    out_dir = tmp_path / "clips"
    # "reproducible": one NSNet2 kernel selection for every launch, so that the denoised audio of run_clips' one resident batch,
    # of run_plan's batch and of the per-instance runs below is the same bits (fvad_ctx_set_option)
    with gpu_ctx.options(reproducible="1"):
        text, results = sim.run_clips(str(tmp_path / "plan.json"), str(out_dir), pcm16=pcm16, ctx=gpu_ctx)
        text_plan, results_plan = sim.run_plan(str(tmp_path / "plan.json"), ctx=gpu_ctx, out=None)
        dens = [np.stack([x["denoised"] for x in gpu_ctx.engine_run([c for c in pcm], want_denoised=True)]) for pcm in audio]
    assert text == text_plan and [r["segments"] for r in results] == [r["segments"] for r in results_plan]
    n_files = 0
    for r, pcm, den in zip(results, audio, dens):
        m = json.loads((out_dir / f"{r['name']}-clips.json").read_text())
        assert m == r["clips"] and len(m["clips"]) == len(r["segments"]) >= 1
        n_den = den.shape[1]
        assert m["original_skipped"] == sum(s[1] > pcm.shape[1] for s in r["segments"])
        assert m["denoised_skipped"] == sum(s[1] > n_den for s in r["segments"])
        for c, s in zip(m["clips"], r["segments"]):
            assert (c["start"], c["length"]) == (s[0], s[1] - s[0])
            for kind, src in (("original", pcm), ("denoised", den)):
                if s[1] > src.shape[1]:
                    assert kind not in c
                    continue
                n_files += 1
                # the file is the export: the same lanes exported here, read back with fvad_wav_read
                want = cc.model_export(src, [(0, src.shape[0], s[0], s[1])], pcm16)
                assert c[kind]["best_channel"] == want["best_channel"][0]
                assert cc.within_one_ulp(np.float32(c[kind]["best_rms"]), want["best_rms"][0])
                assert cc.within_one_ulp(np.float32(c[kind]["runner_up_rms"]), want["runner_up_rms"][0])
                got, sr = fv.wav_read(str(out_dir / c[kind]["file"]))
                assert sr == 48000 and got.shape == (1, c["length"])
                assert got[0].tobytes() == cc.as_f32(want["samples"][0]).tobytes(), (r["name"], kind)
                assert c[kind]["file"] == "{}-{:04d}-{}.wav".format(r["name"], c["segment"], kind)
    assert n_files >= 4 and len(os.listdir(out_dir)) == n_files + 2
