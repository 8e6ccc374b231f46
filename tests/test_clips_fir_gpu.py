"""The filtered Recorder on the GPU (fvad_clips_export_fir(_device), fvad_clips_export_split_fir(_device),
csrc/kernels_clips_fir.hip): clip_fir_cases.py's table -- per (step, H) of (1, 2), (2, 5), (3, 48), (6, 7), (16, 256) and per phase
the clips on both sides of one and two gather tiles at the 8 sample alignments, clips shorter than the filter, and clips at the
source's first and last samples -- through all four call forms and all four format pairs.

Against the float64 model: the f32 -> f32 export within g sum |taps[k]| |x| + one f32 ulp per output (clip_fir_cases.compare).
Against other calls, bit for bit: split = contiguous, host output = device output, a clip alone = the clip among others,
PCM16 out = rint(clamp(f32 out * 32768)), a PCM16 source = an f32 source holding s / 32768; the pick and both RMS values =
the full-rate export's.  Every device export goes into a canary-filled buffer."""
import ctypes as C

import numpy as np
import pytest

import clip_cases as cc
import clip_fir_cases as fc
import clip_split_cases as sc
import clip_stride_cases as st

pytestmark = pytest.mark.gpu

INVALID, OUT_OF_RANGE, TOO_SMALL = -100, -6, -106
STRIDE = cc.N_SAMPLES + 5
CANARY = {False: np.frombuffer(np.uint32(0x7FC0BEEF).tobytes(), np.float32)[0], True: np.int16(0x5A5A)}
TABLE = fc.Table()
KINDS = ("f32", "pcm16", "twin")          # twin: the f32 source that holds the PCM16 source's s / 32768


class Device:
    """the table's lanes on the device in the three source kinds, and a canary-filled output"""

    def __init__(self, fv, ctx):
        self.fv, self.ctx, self.bufs = fv, ctx, []
        i16 = TABLE.source(True)
        self.src = {"f32": TABLE.source(False), "pcm16": i16, "twin": cc.as_f32(i16)}
        self.cap = max(cc.plan(TABLE.clips[c.idx], p)[1] for c in TABLE.cases for p in (False, True)) + 64   # the largest case at full rate
        self.host, self.d_src = {}, {}
        for k, s in self.src.items():
            self.host[k] = np.full((cc.N_LANES, STRIDE), cc.SENTINEL if k == "pcm16" else np.nan, s.dtype)
            self.host[k][:, :cc.N_SAMPLES] = s
            self.d_src[k] = self.up(self.host[k])
        self.d_out = self.up(np.zeros(self.cap, np.float32))
        self.host_out = np.zeros(1024, np.float32)

    def up(self, arr):
        d = self.ctx.device_alloc(arr.nbytes)
        self.bufs.append(d)
        self.ctx.to_device(d, np.ascontiguousarray(arr))
        return d

    def free(self, *ds):
        for d in ds:
            self.bufs.remove(d)
            self.ctx.device_free(d)

    def close(self):
        self.free(*list(self.bufs))

    def fill(self, out_pcm16):
        self.ctx.to_device(self.d_out, np.full(self.cap, CANARY[out_pcm16], np.int16 if out_pcm16 else np.float32))

    def read(self, out_pcm16):
        return self.ctx.to_host(np.zeros(self.cap, np.int16 if out_pcm16 else np.float32), self.d_out)

    def cut(self, res, lens, out_pcm16):
        """`samples` cut from the device output; everything outside the clips' samples must still be the canary"""
        out = self.read(out_pcm16)
        touched = np.zeros(self.cap, bool)
        res["samples"] = []
        for n, o in zip(lens, res["offsets"].astype(np.int64)):
            res["samples"].append(out[o:o + int(n)].copy())
            touched[o:o + int(n)] = True
        assert out[~touched].tobytes() == np.full(int((~touched).sum()), CANARY[out_pcm16], out.dtype).tobytes(), "a canary outside the clips' samples changed"
        return res

    def export(self, kind, clips, skips, step, taps, out_pcm16=False):
        self.fill(out_pcm16)
        res = self.ctx.clips_export(self.d_src[kind], kind == "pcm16", cc.N_LANES, STRIDE, cc.N_SAMPLES, clips, out_pcm16=out_pcm16,
                                    d_out=self.d_out, out_capacity=self.cap, step=step, skips=skips, taps=taps)
        return self.cut(res, res["out_lens"] if "out_lens" in res else clips[:, 3] - clips[:, 2], out_pcm16)

    def export_host(self, kind, clips, skips, step, taps, out_pcm16=False):
        return self.ctx.clips_export(self.d_src[kind], kind == "pcm16", cc.N_LANES, STRIDE, cc.N_SAMPLES, clips, out_pcm16=out_pcm16,
                                     step=step, skips=skips, taps=taps)

    def export_split(self, kind, a, b, rows, skips, step, taps, out_pcm16=False):
        self.fill(out_pcm16)
        res = self.ctx.clips_export_split(a, b, kind == "pcm16", rows, out_pcm16=out_pcm16, d_out=self.d_out, out_capacity=self.cap,
                                          step=step, skips=skips, taps=taps)
        return self.cut(res, res["out_lens"], out_pcm16)

    def raw(self, clips, step, skips, taps, n_taps=None, cap=None, host=False, d_out="own", out_format=0):
        """fvad_clips_export_fir(_device) itself on the f32 source -> status"""
        fv = self.fv
        clips = np.ascontiguousarray(np.asarray(clips, np.uint64).reshape(-1, 4))
        skips = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32))
        taps = None if taps is None else np.ascontiguousarray(np.asarray(taps, np.float32))
        fn = fv.lib().fvad_clips_export_fir if host else fv.lib().fvad_clips_export_fir_device
        return fn(self.ctx.h, fv.vp(self.d_src["f32"]), 0, cc.N_LANES, STRIDE, cc.N_SAMPLES, clips.ctypes.data_as(C.POINTER(C.c_uint64)), len(clips),
                  out_format, fv.vp((self.host_out.ctypes.data if host else self.d_out) if d_out == "own" else d_out),
                  ((1024 if host else self.cap) if cap is None else cap), None, None, None, None, step,
                  None if skips is None else skips.ctypes.data_as(C.POINTER(C.c_uint32)), fv.fptr(taps),
                  (0 if taps is None else len(taps)) if n_taps is None else n_taps)

    def raw_split(self, lay, d_a, d_b, rows, step, skips, taps, n_taps=None, cap=None, host=False):
        fv = self.fv
        rows = np.ascontiguousarray(np.asarray(rows, np.uint64).reshape(-1, sc.FIELDS))
        skips = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32))
        taps = None if taps is None else np.ascontiguousarray(np.asarray(taps, np.float32))
        a, b = lay.a(d_a), lay.b(d_b)
        fn = fv.lib().fvad_clips_export_split_fir if host else fv.lib().fvad_clips_export_split_fir_device
        return fn(self.ctx.h, fv.vp(a[0]), a[1], a[2], a[3], fv.vp(b[0]), b[1], b[2], b[3], 0, rows.ctypes.data_as(C.POINTER(C.c_uint64)), len(rows), 0,
                  fv.vp(self.host_out.ctypes.data if host else self.d_out), (1024 if host else self.cap) if cap is None else cap, None, None, None, None,
                  step, None if skips is None else skips.ctypes.data_as(C.POINTER(C.c_uint32)), fv.fptr(taps),
                  (0 if taps is None else len(taps)) if n_taps is None else n_taps)


@pytest.fixture(scope="module")
def dev(fv, gpu_ctx):
    d = Device(fv, gpu_ctx)
    yield d
    for k in KINDS:                                                       # the sources are as they were
        assert d.ctx.to_host(np.zeros_like(d.host[k]), d.d_src[k]).tobytes() == d.host[k].tobytes()
    d.close()


def same_bits(got, want, what, fields=("best_channel", "best_rms", "runner_up_rms", "offsets")):
    for f in fields:
        assert np.asarray(got[f]).tobytes() == np.asarray(want[f]).tobytes(), (what, f)
    assert len(got["samples"]) == len(want["samples"])
    for i, (g, w) in enumerate(zip(got["samples"], want["samples"])):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, "samples of clip", i)


def host_form(h, d, what):
    """the host form's result h against the device form's d (with `samples`): the same bits, zeros between the slots"""
    assert all(h[f].tobytes() == d[f].tobytes() for f in ("best_channel", "best_rms", "runner_up_rms", "offsets", "out_lens")), what
    touched = np.zeros(h["total"], bool)
    for o, s in zip(h["offsets"].astype(np.int64), d["samples"]):
        assert h["out"][o:o + len(s)].tobytes() == s.tobytes(), what
        touched[o:o + len(s)] = True
    assert not h["out"][~touched].any(), what


def as_pcm16(res):
    """Convert<int16_t, float> over an f32 result's samples"""
    return [cc.convert(s, True) for s in res["samples"]]


@pytest.mark.parametrize("kind", ["f32", "pcm16"])
def test_the_table_through_the_contiguous_forms(dev, kind):
    for case in TABLE.cases:
        what = f"{case}, from {kind}"
        clips, skips = TABLE.clips[case.idx], TABLE.skips(case)
        got = dev.export(kind, clips, skips, case.step, case.taps)
        if kind == "f32":
            fc.compare(got, fc.model_export_fir(dev.src["f32"], clips, skips, case.step, case.taps), what)
        else:                                                             # a PCM16 source is its f32 twin, bit for bit
            same_bits(got, dev.export("twin", clips, skips, case.step, case.taps), what + " against its f32 twin")
        # the slots are the strided plan's; the pick and both RMS values are the full-rate export's bits
        out_lens, offsets, total = dev.fv.clips_plan_strided(clips[:, 3] - clips[:, 2], skips, case.step, False)
        assert np.array_equal(got["offsets"], offsets) and np.array_equal(got["out_lens"], out_lens) and got["total"] == total
        full = dev.export(kind, clips, None, 1, None)
        same_bits(dict(got, samples=[]), dict(full, samples=[]), what + " against the full-rate export", ("best_channel", "best_rms", "runner_up_rms"))
        # PCM16 out is the f32 output converted
        p = dev.export(kind, clips, skips, case.step, case.taps, out_pcm16=True)
        same_bits(p, dict(got, samples=as_pcm16(got)), what + " to PCM16", ("best_channel", "best_rms", "runner_up_rms"))
        assert np.array_equal(p["offsets"], dev.fv.clips_plan_strided(clips[:, 3] - clips[:, 2], skips, case.step, True)[1])
        host_form(dev.export_host(kind, clips, skips, case.step, case.taps), got, what)
        host_form(dev.export_host(kind, clips, skips, case.step, case.taps, out_pcm16=True), p, what + " to PCM16")
    assert len(TABLE.cases) == 28 and all(len(c.edge) == 40 for c in TABLE.cases)


@pytest.mark.parametrize("kind", ["f32", "pcm16"])
def test_the_table_through_the_split_forms(dev, kind):
    for case in TABLE.cases:
        what = f"split, {case}, from {kind}"
        lay, skips = fc.split_case(TABLE, case, dev.src[kind])
        d_a, d_b = dev.up(lay.A), dev.up(lay.B)
        try:
            whole = dev.export(kind, TABLE.clips[lay.base], skips, case.step, case.taps)     # the same clips in one piece
            got = dev.export_split(kind, lay.a(d_a), lay.b(d_b), lay.rows, skips, case.step, case.taps)
            same_bits(got, whole, what)
            if kind == "f32":
                fc.compare(got, fc.model_export_split_fir(lay, skips, case.step, case.taps), what)
            p = dev.export_split(kind, lay.a(d_a), lay.b(d_b), lay.rows, skips, case.step, case.taps, out_pcm16=True)
            same_bits(p, dict(got, samples=as_pcm16(got)), what + " to PCM16", ("best_channel", "best_rms", "runner_up_rms"))
            for out_pcm16, d in ((False, got), (True, p)):
                h = dev.ctx.clips_export_split(lay.a(d_a), lay.b(d_b), kind == "pcm16", lay.rows, out_pcm16=out_pcm16, step=case.step, skips=skips, taps=case.taps)
                host_form(h, d, what)
            if case.phase == 0:
                # the first slice has no held buffer: d_a NULL, the rows whose seam is 0
                first = np.flatnonzero(lay.sigma == 0)
                alone = dev.export_split(kind, (None, 0, 0, 0), lay.b(d_b), lay.rows[first], skips[first], case.step, case.taps)
                same_bits(alone, {k: ([v[i] for i in first] if k == "samples" else np.asarray(v)[first]) for k, v in whole.items()
                                  if k in ("best_channel", "best_rms", "runner_up_rms", "samples")}, what + ", d_a NULL", ("best_channel", "best_rms", "runner_up_rms"))
        finally:
            dev.free(d_a, d_b)
        assert len(lay.rows) >= 20 and (lay.rows[:, 3] < case.H).any() and (lay.rows[:, 6] < case.H).any()


@pytest.mark.parametrize("out_pcm16", [False, True], ids=["to-f32", "to-pcm16"])
def test_a_clip_is_the_same_bits_whatever_else_is_in_the_call(dev, out_pcm16):
    rng = np.random.default_rng(11)
    case = TABLE.cases[1 + 2 + 1]                                         # step 3, H 48, phase 1
    assert (case.step, case.H, case.phase) == (3, 48, 1)
    clips, skips = TABLE.clips[case.idx], TABLE.skips(case)
    whole = dev.export("f32", clips, skips, 3, case.taps, out_pcm16)
    rev = dev.export("f32", clips[::-1], skips[::-1], 3, case.taps, out_pcm16)
    picks = [int(np.flatnonzero(case.idx == k)[0]) for k in (int(case.named[2]), int(case.edge[27]), int(case.short[-1]))]
    for r in picks:
        alone = dev.export("f32", clips[r:r + 1], skips[r:r + 1], 3, case.taps, out_pcm16)
        o = rng.integers(0, len(clips), 12)
        among = dev.export("f32", np.concatenate([clips[o[:5]], clips[r:r + 1], clips[o[5:]]]), np.concatenate([skips[o[:5]], skips[r:r + 1], skips[o[5:]]]), 3, case.taps, out_pcm16)
        for res, k in ((among, 5), (whole, r), (rev, len(clips) - 1 - r)):
            for f in ("best_channel", "best_rms", "runner_up_rms"):
                assert res[f][k].tobytes() == alone[f][0].tobytes(), (r, f)
            assert res["samples"][k].tobytes() == alone["samples"][0].tobytes(), r
    same_bits(dev.export("f32", clips, skips, 3, case.taps, out_pcm16), whole, "a second call")


def test_special_taps(dev):
    for case in (TABLE.cases[1], TABLE.cases[4], TABLE.cases[8]):        # steps 2, 3 and 6
        clips, skips = TABLE.clips[case.idx], TABLE.skips(case)
        strided = dev.export("f32", clips, skips, case.step, None)
        # one tap of 1 is the strided export, as values (-0 becomes +0)
        one = dev.export("f32", clips, skips, case.step, [1.0])
        same_bits(one, dict(strided, samples=[s + np.float32(0.0) for s in strided["samples"]]), f"{case}, taps [1]")
        # a 1 in the first of five taps is clip sample c - 2 (0 in front of the clip), in the last c + 2 (0 behind it)
        full = dev.export("f32", clips, None, 1, None)
        for taps, shift in (([1, 0, 0, 0, 0], -2), ([0, 0, 0, 0, 1], 2)):
            got = dev.export("f32", clips, skips, case.step, taps)
            want = []
            for x, k in zip(full["samples"], skips):
                xp = np.concatenate([np.zeros(2, np.float32), x + np.float32(0.0), np.zeros(2, np.float32)])
                want.append(xp[2 + shift + int(k):2 + shift + len(x):case.step])
            same_bits(got, dict(strided, samples=want), f"{case}, taps {taps}")
    # step 1 is a plain FIR: the model again, on one tile and a bit
    case = TABLE.cases[0]
    clips = TABLE.clips[case.edge[16:32]]
    fc.compare(dev.export("f32", clips, None, 1, case.taps), fc.model_export_fir(dev.src["f32"], clips, np.zeros(len(clips), np.uint32), 1, case.taps), "step 1, skips NULL")


def tone_clip(dev, freq, n=4800):
    x = (0.5 * np.sin(2 * np.pi * freq / 48000.0 * np.arange(n))).astype(np.float32)
    d = dev.up(x)
    return x, d


def test_the_filter_removes_what_the_stride_folds_into_the_band(dev):
    taps = dev.fv.clips_fir_design(3)
    H, g = (len(taps) - 1) // 2, fc.gamma(len(taps))
    bound = g * float(np.abs(taps).sum()) * 0.5                           # |x| <= 0.5: the rounding of a 97-term fma chain
    drop = -(-H // 3)
    for freq, alias in ((10000.0, True), (3000.0, False)):
        x, d = tone_clip(dev, freq)
        try:
            kw = dict(d_src=d, src_pcm16=False, n_lanes=1, lane_stride=len(x), n_samples=len(x), clips=[(0, 1, 0, len(x))], step=3)
            y = dev.ctx.clips_export(taps=taps, **kw)["out"]
            s = dev.ctx.clips_export(skips=[0], **kw)["out"]
        finally:
            dev.free(d)
        assert len(y) == len(s) == 1600
        mag = float(fc.response(taps, freq / 48000.0)[0])
        if alias:
            # 10 kHz is above the 8 kHz Nyquist frequency of the export: the stride folds it to 6 kHz at full level
            assert np.sqrt(np.mean(s.astype(np.float64) ** 2)) > 0.35
            rms = np.sqrt(np.mean(y[drop:-drop].astype(np.float64) ** 2))
            assert rms <= mag * 0.5 / np.sqrt(2.0) + bound, (rms, mag)
            assert mag < 10 ** (-68 / 20)
        else:
            # 3 kHz passes: the filter's delay is zero (the taps are centred), so the samples are the stride's within the ripple
            err = np.abs(y[drop:-drop].astype(np.float64) - s[drop:-drop])
            assert err.max() <= abs(1.0 - mag) * 0.5 + bound, (err.max(), mag)


def test_refused_calls_write_nothing(dev):
    dev.fill(False)
    ok = [(1, 1, 100, 200), (2, 2, 50000, 59000)]
    taps = fc.case_taps(3, 48)
    total = st.plan_strided([100, 9000], [1, 2], 3, False)[2]
    nan = taps.copy()
    nan[17] = np.nan
    past = [ok[0], (1, 1, 100, cc.N_SAMPLES + 1)]
    for what, status, kw in (
            ("NULL taps", INVALID, dict(clips=ok, step=3, skips=None, taps=None, n_taps=97)),
            ("no taps", INVALID, dict(clips=ok, step=3, skips=None, taps=taps, n_taps=0)),
            ("an even n_taps", INVALID, dict(clips=ok, step=3, skips=None, taps=taps, n_taps=96)),
            ("n_taps above the maximum", INVALID, dict(clips=ok, step=3, skips=None, taps=np.zeros(515, np.float32))),
            ("a tap that is not finite", INVALID, dict(clips=ok, step=3, skips=None, taps=nan)),
            ("an infinite tap", INVALID, dict(clips=ok, step=1, skips=None, taps=[np.inf])),
            ("the taps' rule comes before a range's", INVALID, dict(clips=past, step=3, skips=None, taps=nan)),
            ("step 0", INVALID, dict(clips=ok, step=0, skips=None, taps=taps)),
            ("step above the limit", INVALID, dict(clips=ok, step=17, skips=None, taps=taps)),
            ("a skip equal to the step", INVALID, dict(clips=ok, step=3, skips=[0, 3], taps=taps)),
            ("a clip that keeps no sample", INVALID, dict(clips=[ok[0], (1, 1, 100, 102)], step=3, skips=[0, 2], taps=taps)),
            ("a clip's own rule", INVALID, dict(clips=[ok[0], (1, 0, 100, 200)], step=3, skips=[0, 0], taps=taps)),
            ("NULL output", INVALID, dict(clips=ok, step=3, skips=None, taps=taps, d_out=0)),
            ("bad output format", INVALID, dict(clips=ok, step=3, skips=None, taps=taps, out_format=2)),
            ("a clip past n_samples", OUT_OF_RANGE, dict(clips=past, step=3, skips=[0, 0], taps=taps)),
            ("lanes past n_lanes", OUT_OF_RANGE, dict(clips=[ok[0], (cc.N_LANES - 1, 2, 0, 10)], step=3, skips=[0, 0], taps=taps)),
            ("capacity below the strided total", TOO_SMALL, dict(clips=ok, step=3, skips=[1, 2], taps=taps, cap=total - 1))):
        assert dev.raw(**kw) == status, what
        assert "fvad_clips_export" in dev.fv.lib().fvad_last_error(dev.ctx.h).decode(), what
        if "d_out" not in kw or kw["d_out"] == 0:
            assert dev.raw(host=True, **dict(kw, cap=min(kw.get("cap", 1024), 1024))) == status, what + " (host form)"
    # every clip the table lists as keeping no sample, alone and among others
    for case in TABLE.cases:
        for k in case.refused:
            skip = TABLE.skips(case, [k])
            assert dev.raw([TABLE.clips[k]], case.step, skip, case.taps) == INVALID, (case, k)
            assert dev.raw([ok[0], TABLE.clips[k]], case.step, [0, skip[0]], case.taps) == INVALID, (case, k)
    assert sum(len(c.refused) for c in TABLE.cases) > 10
    # the split form: the same rules, after the rows' own and the strided ones, before the ranges'
    case = TABLE.cases[5]
    lay, skips = fc.split_case(TABLE, case, dev.src["f32"])
    d_a, d_b = dev.up(lay.A), dev.up(lay.B)
    try:
        r = lay.rows[(lay.rows[:, 3] > 0) & (lay.rows[:, 6] > 0)][:2]
        beyond = r.copy()
        beyond[1, 2] = lay.a_samples                                      # a piece past A's samples
        lens = [int(r[0, 3] + r[0, 6]), int(r[1, 3] + r[1, 6])]
        for what, status, kw in (
                ("NULL taps", INVALID, dict(rows=r, step=3, skips=None, taps=None, n_taps=5)),
                ("an even n_taps", INVALID, dict(rows=r, step=3, skips=None, taps=taps, n_taps=2)),
                ("n_taps above the maximum", INVALID, dict(rows=r, step=3, skips=None, taps=np.zeros(515, np.float32))),
                ("a tap that is not finite", INVALID, dict(rows=r, step=3, skips=None, taps=nan)),
                ("the taps' rule comes before a range's", INVALID, dict(rows=beyond, step=3, skips=None, taps=nan)),
                ("step 0", INVALID, dict(rows=r, step=0, skips=None, taps=taps)),
                ("a skip equal to the step", INVALID, dict(rows=r, step=3, skips=[2, 3], taps=taps)),
                ("a piece past its buffer", OUT_OF_RANGE, dict(rows=beyond, step=3, skips=None, taps=taps)),
                ("capacity below the strided total", TOO_SMALL, dict(rows=r, step=3, skips=None, taps=taps, cap=st.plan_strided(lens, None, 3, False)[2] - 1))):
            assert dev.raw_split(lay, d_a, d_b, **kw) == status, what
            assert "fvad_clips_export_split" in dev.fv.lib().fvad_last_error(dev.ctx.h).decode(), what
            assert dev.raw_split(lay, d_a, d_b, host=True, **dict(kw, cap=min(kw.get("cap", 1024), 1024))) == status, what + " (host form)"
        # nothing was written by any refused call
        assert dev.read(False).tobytes() == np.full(dev.cap, CANARY[False], np.float32).tobytes()
        assert not dev.host_out.any()
        assert dev.raw_split(lay, d_a, d_b, r, 3, None, taps, cap=st.plan_strided(lens, None, 3, False)[2]) == 0
    finally:
        dev.free(d_a, d_b)
    assert dev.raw([], 3, None, taps) == 0 and dev.raw([], 0, None, None, host=True) == 0      # no clips: nothing to do
    assert dev.raw(ok, 3, [1, 2], taps, cap=total) == 0                   # exactly the strided total


def test_kernel_times_name_the_filtered_gathers(dev):
    case = TABLE.cases[3]
    lay, skips = fc.split_case(TABLE, case, dev.src["f32"])
    d_a, d_b = dev.up(lay.A), dev.up(lay.B)
    dev.ctx.enable_timing(True)
    try:
        dev.ctx.kernel_times()                                            # (drop what earlier calls left)
        dev.export("f32", TABLE.clips[case.idx], TABLE.skips(case), case.step, case.taps)
        times = dev.ctx.kernel_times()
        assert {"clip_rms", "clip_pick", "clip_gather_fir"} <= set(times) and not {"clip_gather", "clip_gather_strided"} & set(times) and times["clip_gather_fir"] > 0
        dev.export_split("f32", lay.a(d_a), lay.b(d_b), lay.rows, skips, case.step, case.taps)
        times = dev.ctx.kernel_times()
        assert {"clip_rms_split", "clip_pick", "clip_gather_fir_split"} <= set(times) and not {"clip_gather_split", "clip_gather_strided_split"} & set(times)
        dev.export("f32", TABLE.clips[case.idx[:3]], None, 1, [1.0])     # step 1 is still the filtered gather
        assert "clip_gather_fir" in dev.ctx.kernel_times()
    finally:
        dev.ctx.enable_timing(False)
        dev.free(d_a, d_b)
