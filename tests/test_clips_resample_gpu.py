"""The resampled Recorder on the GPU (fvad_clips_export_resampled(_device), fvad_clips_export_split_resampled(_device),
csrc/kernels_clips_resample.hip): clip_resample_cases.py's tables -- per ratio of 2/3, 5/7, 7/5, 1/3, 147/160 (short and at the
default length) and 147/640 the clips on both sides of one and two gather tiles at the 8 sample alignments, clips shorter than the
filter's reach, and clips at the source's first and last samples -- through all four call forms and all four format pairs.

Against the float64 model: the f32 -> f32 export within g sum |tap| |x| + one f32 ulp per output (clip_resample_cases.compare;
computed, not measured).  Against other calls, bit for bit: split = contiguous at every seam, host output = device output,
reversed clip order, a clip alone, a rerun, PCM16 out = rint(clamp(f32 out * 32768)), a PCM16 source = an f32 source holding
s / 32768; the pick and both RMS values = the full-rate export's.  Every clip of stream E has NaN (the sentinel) directly in
front of and behind it, and every device export goes into a canary-filled buffer."""
import ctypes as C

import numpy as np
import pytest

import clip_cases as cc
import clip_resample_cases as rc
import clip_split_cases as sc
import ingest_resample_cases as rr

pytestmark = pytest.mark.gpu

INVALID, OUT_OF_RANGE, TOO_SMALL = -100, -6, -106
CANARY = {False: np.frombuffer(np.uint32(0x7FC0BEEF).tobytes(), np.float32)[0], True: np.int16(0x5A5A)}
KINDS = ("f32", "pcm16", "twin")          # twin: the f32 source that holds the PCM16 source's s / 32768
IDS = [f"{u}-{d}-half{h}-{k}" for u, d, h, k in rc.CASES]


class Device:
    """one table's lanes on the device in the three source kinds, and a canary-filled output"""

    def __init__(self, fv, ctx, table):
        self.fv, self.ctx, self.t, self.bufs = fv, ctx, table, []
        self.stride = table.n_samples + 5
        i16 = table.source(True)
        self.src = {"f32": table.source(False), "pcm16": i16, "twin": cc.as_f32(i16)}
        # the table at full rate and at the table's ratio, in either output format
        self.cap = max(max(cc.plan(table.clips, p)[1], rc.plan(table.out_lens, p)[1]) for p in (False, True)) + 64
        self.host, self.d_src = {}, {}
        for k, s in self.src.items():
            self.host[k] = np.full((rc.N_LANES, self.stride), cc.SENTINEL if k == "pcm16" else np.nan, s.dtype)
            self.host[k][:, :table.n_samples] = s
            self.d_src[k] = self.up(self.host[k])
        self.d_out = self.up(np.zeros(self.cap, np.float32))
        self.host_out = np.zeros(1024, np.float32)
        self.want = rc.model_export(self.src["f32"], table.clips, table.taps, table.up, table.down)   # computed once, shared
        self.got = {}

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

    def kw(self, up, down, taps):
        t = self.t
        return dict(up=t.up if up is None else up, down=t.down if down is None else down, taps=t.taps if taps is None else taps)

    def export(self, kind, clips, out_pcm16=False, up=None, down=None, taps=None, full=False):
        self.fill(out_pcm16)
        res = self.ctx.clips_export(self.d_src[kind], kind == "pcm16", rc.N_LANES, self.stride, self.t.n_samples, clips, out_pcm16=out_pcm16,
                                    d_out=self.d_out, out_capacity=self.cap, **({} if full else self.kw(up, down, taps)))
        return self.cut(res, clips[:, 3] - clips[:, 2] if full else res["out_lens"], out_pcm16)

    def export_host(self, kind, clips, out_pcm16=False):
        return self.ctx.clips_export(self.d_src[kind], kind == "pcm16", rc.N_LANES, self.stride, self.t.n_samples, clips, out_pcm16=out_pcm16,
                                     **self.kw(None, None, None))

    def export_split(self, kind, a, b, rows, out_pcm16=False):
        self.fill(out_pcm16)
        res = self.ctx.clips_export_split(a, b, kind == "pcm16", rows, out_pcm16=out_pcm16, d_out=self.d_out, out_capacity=self.cap,
                                          **self.kw(None, None, None))
        return self.cut(res, res["out_lens"], out_pcm16)

    def whole(self, kind):
        """the table through the contiguous device form, f32 out: run once per kind, shared"""
        if kind not in self.got:
            self.got[kind] = self.export(kind, self.t.clips)
        return self.got[kind]

    def raw(self, clips, up, down, taps, n_taps=None, cap=None, host=False, d_out="own", out_format=0):
        """fvad_clips_export_resampled(_device) itself on the f32 source -> status"""
        fv = self.fv
        clips = np.ascontiguousarray(np.asarray(clips, np.uint64).reshape(-1, 4))
        taps = None if taps is None else np.ascontiguousarray(np.asarray(taps, np.float32))
        fn = fv.lib().fvad_clips_export_resampled if host else fv.lib().fvad_clips_export_resampled_device
        return fn(self.ctx.h, fv.vp(self.d_src["f32"]), 0, rc.N_LANES, self.stride, self.t.n_samples, clips.ctypes.data_as(C.POINTER(C.c_uint64)), len(clips),
                  out_format, fv.vp((self.host_out.ctypes.data if host else self.d_out) if d_out == "own" else d_out),
                  ((1024 if host else self.cap) if cap is None else cap), None, None, None, None, up, down, fv.fptr(taps),
                  (0 if taps is None else len(taps)) if n_taps is None else n_taps)

    def raw_split(self, lay, d_a, d_b, rows, up, down, taps, n_taps=None, cap=None, host=False):
        fv = self.fv
        rows = np.ascontiguousarray(np.asarray(rows, np.uint64).reshape(-1, sc.FIELDS))
        taps = None if taps is None else np.ascontiguousarray(np.asarray(taps, np.float32))
        a, b = lay.a(d_a), lay.b(d_b)
        fn = fv.lib().fvad_clips_export_split_resampled if host else fv.lib().fvad_clips_export_split_resampled_device
        return fn(self.ctx.h, fv.vp(a[0]), a[1], a[2], a[3], fv.vp(b[0]), b[1], b[2], b[3], 0, rows.ctypes.data_as(C.POINTER(C.c_uint64)), len(rows), 0,
                  fv.vp(self.host_out.ctypes.data if host else self.d_out), (1024 if host else self.cap) if cap is None else cap, None, None, None, None,
                  up, down, fv.fptr(taps), (0 if taps is None else len(taps)) if n_taps is None else n_taps)


@pytest.fixture(scope="module", params=rc.CASES, ids=IDS)
def dev(request, fv, gpu_ctx):
    d = Device(fv, gpu_ctx, rc.Table(*request.param))
    yield d
    for k in KINDS:                                                       # the sources, NaN guards included, are as they were
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


def test_the_table_within_the_bound(dev):
    t = dev.t
    got = dev.whole("f32")
    rc.compare(got, dev.want, f"{t}")
    assert all(np.isfinite(s).all() for s in got["samples"]), "a read outside a clip reached an output"
    out_lens, offsets, total = dev.fv.clips_plan_resampled(t.clips[:, 3] - t.clips[:, 2], t.up, t.down, False)
    assert np.array_equal(got["offsets"], offsets) and np.array_equal(got["out_lens"], out_lens) and got["total"] == total
    assert np.array_equal(out_lens, t.out_lens) and dev.fv.clips_resample_tile(t.up, t.down, t.n_taps) == t.To
    assert len(t.edge) == 40 and len(t.short) >= 4


def test_pick_and_rms_are_the_full_rate_exports(dev):
    for kind in ("f32", "pcm16"):
        full = dev.export(kind, dev.t.clips, full=True)
        same_bits(dict(dev.whole(kind), samples=[]), dict(full, samples=[]), f"{dev.t} from {kind}", ("best_channel", "best_rms", "runner_up_rms"))


def test_the_formats(dev):
    t = dev.t
    got = dev.whole("f32")
    # a PCM16 source is its f32 twin, bit for bit
    same_bits(dev.whole("pcm16"), dev.whole("twin"), f"{t}: PCM16 against its f32 twin")
    rc.compare(dev.whole("pcm16"), rc.model_export(dev.src["pcm16"], t.clips, t.taps, t.up, t.down), f"{t} from PCM16")
    # PCM16 out is the f32 output converted
    for kind in ("f32", "pcm16"):
        p = dev.export(kind, t.clips, out_pcm16=True)
        same_bits(p, dict(dev.whole(kind), samples=as_pcm16(dev.whole(kind))), f"{t} from {kind} to PCM16", ("best_channel", "best_rms", "runner_up_rms"))
        assert np.array_equal(p["offsets"], dev.fv.clips_plan_resampled(t.clips[:, 3] - t.clips[:, 2], t.up, t.down, True)[1])
        host_form(dev.export_host(kind, t.clips, out_pcm16=True), p, f"{t} from {kind} to PCM16, host form")
    host_form(dev.export_host("f32", t.clips), got, f"{t}, host form")


@pytest.mark.parametrize("kind", ["f32", "pcm16"])
def test_the_split_forms_at_every_seam(dev, kind):
    t = dev.t
    what = f"split, {t}, from {kind}"
    lay = rc.split_case(t, dev.src[kind])
    d_a, d_b = dev.up(lay.A), dev.up(lay.B)
    try:
        base = dev.whole(kind)
        whole = {k: ([v[i] for i in lay.base] if k == "samples" else np.asarray(v)[lay.base]) for k, v in base.items()
                 if k in ("best_channel", "best_rms", "runner_up_rms", "samples")}
        got = dev.export_split(kind, lay.a(d_a), lay.b(d_b), lay.rows)
        same_bits(got, whole, what, ("best_channel", "best_rms", "runner_up_rms"))
        assert np.array_equal(got["offsets"], rc.plan(t.out_lens[lay.base], False)[0])
        if kind == "f32":
            rc.compare(got, rc.model_export_split(lay, t.taps, t.up, t.down), what)
        p = dev.export_split(kind, lay.a(d_a), lay.b(d_b), lay.rows, out_pcm16=True)
        same_bits(p, dict(got, samples=as_pcm16(got)), what + " to PCM16", ("best_channel", "best_rms", "runner_up_rms"))
        for out_pcm16, d in ((False, got), (True, p)):
            h = dev.ctx.clips_export_split(lay.a(d_a), lay.b(d_b), kind == "pcm16", lay.rows, out_pcm16=out_pcm16, **dev.kw(None, None, None))
            host_form(h, d, what)
        # the first slice has no held buffer: d_a NULL, the rows whose seam is 0
        first = np.flatnonzero(lay.sigma == 0)
        alone = dev.export_split(kind, (None, 0, 0, 0), lay.b(d_b), lay.rows[first])
        same_bits(alone, {k: ([v[i] for i in first] if k == "samples" else np.asarray(v)[first]) for k, v in whole.items()}, what + ", d_a NULL",
                  ("best_channel", "best_rms", "runner_up_rms"))
    finally:
        dev.free(d_a, d_b)
    assert len(lay.rows) >= 20 and (lay.rows[:, 3] < t.R).any() and (lay.rows[:, 6] < t.R).any()


def test_a_clip_is_the_same_bits_whatever_else_is_in_the_call(dev):
    t = dev.t
    rng = np.random.default_rng(11)
    whole = dev.whole("f32")
    same_bits(dev.export("f32", t.clips), whole, "a second call")
    rev = dev.export("f32", t.clips[::-1])
    same_bits(dict(rev, samples=rev["samples"][::-1]), dict(whole, samples=whole["samples"]), "reversed order", ())
    for f in ("best_channel", "best_rms", "runner_up_rms"):
        assert rev[f][::-1].tobytes() == whole[f].tobytes(), f
    for r in (int(t.named[2]), int(t.edge[27]), int(t.edge[35]), int(t.short[-1]), int(t.short[0])):
        alone = dev.export("f32", t.clips[r:r + 1])
        o = rng.integers(0, len(t.clips), 6)
        among = dev.export("f32", np.concatenate([t.clips[o[:3]], t.clips[r:r + 1], t.clips[o[3:]]]))
        for res, k in ((among, 3), (whole, r)):
            for f in ("best_channel", "best_rms", "runner_up_rms"):
                assert res[f][k].tobytes() == alone[f][0].tobytes(), (r, f)
            assert res["samples"][k].tobytes() == alone["samples"][0].tobytes(), r


def test_one_tap_of_one_at_ratio_one_is_the_full_rate_export(dev):
    clips = dev.t.clips
    full = dev.export("f32", clips, full=True)
    one = dev.export("f32", clips, up=1, down=1, taps=[1.0])
    same_bits(one, dict(full, samples=[s + np.float32(0.0) for s in full["samples"]]), "1/1, taps [1]")   # (as values: -0 becomes +0)
    p = dev.export("pcm16", clips, out_pcm16=True, up=1, down=1, taps=[1.0])
    same_bits(p, dev.export("pcm16", clips, out_pcm16=True, full=True), "1/1, taps [1], PCM16")


def test_refused_calls_launch_nothing(dev):
    t = dev.t
    if (t.up, t.down, t.half) != (2, 3, 4):
        return                                                            # the rules do not depend on the ratio: once
    dev.fill(False)
    ok = [(1, 1, 100, 200), (2, 2, 50000, 59000)]
    taps = t.taps
    total = rc.plan([rc.out_len(100, 2, 3), rc.out_len(9000, 2, 3)], False)[1]
    nan = taps.copy()
    nan[7] = np.nan
    past = [ok[0], (1, 1, 100, t.n_samples + 1)]
    dev.ctx.enable_timing(True)
    try:
        dev.ctx.kernel_times()
        for what, status, kw in (
                ("up 0", INVALID, dict(clips=ok, up=0, down=3, taps=taps)),
                ("up above the maximum", INVALID, dict(clips=ok, up=641, down=3, taps=taps)),
                ("down 0", INVALID, dict(clips=ok, up=2, down=0, taps=taps)),
                ("the ratio's rule comes before the taps'", INVALID, dict(clips=ok, up=0, down=3, taps=None, n_taps=0)),
                ("NULL taps", INVALID, dict(clips=ok, up=2, down=3, taps=None, n_taps=25)),
                ("no taps", INVALID, dict(clips=ok, up=2, down=3, taps=taps, n_taps=0)),
                ("an even n_taps", INVALID, dict(clips=ok, up=2, down=3, taps=taps, n_taps=24)),
                ("n_taps above the maximum", INVALID, dict(clips=ok, up=2, down=3, taps=np.zeros(rc.TAPS_MAX + 2, np.float32))),
                ("a tap that is not finite", INVALID, dict(clips=ok, up=2, down=3, taps=nan)),
                ("a window that fits no tile", INVALID, dict(clips=ok, up=1, down=48000, taps=taps)),
                ("the taps' rule comes before a range's", INVALID, dict(clips=past, up=2, down=3, taps=nan)),
                ("a clip's own rule", INVALID, dict(clips=[ok[0], (1, 0, 100, 200)], up=2, down=3, taps=taps)),
                ("an empty clip", INVALID, dict(clips=[ok[0], (1, 1, 100, 100)], up=2, down=3, taps=taps)),
                ("NULL output", INVALID, dict(clips=ok, up=2, down=3, taps=taps, d_out=0)),
                ("bad output format", INVALID, dict(clips=ok, up=2, down=3, taps=taps, out_format=2)),
                ("a clip past n_samples", OUT_OF_RANGE, dict(clips=past, up=2, down=3, taps=taps)),
                ("lanes past n_lanes", OUT_OF_RANGE, dict(clips=[ok[0], (rc.N_LANES - 1, 2, 0, 10)], up=2, down=3, taps=taps)),
                ("capacity below the resampled total", TOO_SMALL, dict(clips=ok, up=2, down=3, taps=taps, cap=total - 1))):
            assert dev.raw(**kw) == status, what
            assert "fvad_clips_export" in dev.fv.lib().fvad_last_error(dev.ctx.h).decode(), what
            if "d_out" not in kw or kw["d_out"] == 0:
                assert dev.raw(host=True, **dict(kw, cap=min(kw.get("cap", 1024), 1024))) == status, what + " (host form)"
        # the split form: the same rules, after the rows' own, before the ranges'
        lay = rc.split_case(t, dev.src["f32"])
        d_a, d_b = dev.up(lay.A), dev.up(lay.B)
        try:
            r = lay.rows[(lay.rows[:, 3] > 0) & (lay.rows[:, 6] > 0) & (lay.rows[:, 3] + lay.rows[:, 6] < 100)][:2]
            beyond = r.copy()
            beyond[1, 2] = lay.a_samples                                  # a piece past A's samples
            lens = [int(r[0, 3] + r[0, 6]), int(r[1, 3] + r[1, 6])]
            split_total = rc.plan([rc.out_len(n, 2, 3) for n in lens], False)[1]
            for what, status, kw in (
                    ("up 0", INVALID, dict(rows=r, up=0, down=3, taps=taps)),
                    ("NULL taps", INVALID, dict(rows=r, up=2, down=3, taps=None, n_taps=5)),
                    ("an even n_taps", INVALID, dict(rows=r, up=2, down=3, taps=taps, n_taps=2)),
                    ("a tap that is not finite", INVALID, dict(rows=r, up=2, down=3, taps=nan)),
                    ("the taps' rule comes before a range's", INVALID, dict(rows=beyond, up=2, down=3, taps=nan)),
                    ("a piece past its buffer", OUT_OF_RANGE, dict(rows=beyond, up=2, down=3, taps=taps)),
                    ("capacity below the resampled total", TOO_SMALL, dict(rows=r, up=2, down=3, taps=taps, cap=split_total - 1))):
                assert dev.raw_split(lay, d_a, d_b, **kw) == status, what
                assert "fvad_clips_export_split" in dev.fv.lib().fvad_last_error(dev.ctx.h).decode(), what
                assert dev.raw_split(lay, d_a, d_b, host=True, **dict(kw, cap=min(kw.get("cap", 1024), 1024))) == status, what + " (host form)"
            # no refused call launched anything or wrote anything
            times = dev.ctx.kernel_times()
            assert not {"clip_rms", "clip_rms_split", "clip_pick", "clip_gather_resampled", "clip_gather_resampled_split"} & set(times), times
            assert dev.read(False).tobytes() == np.full(dev.cap, CANARY[False], np.float32).tobytes()
            assert not dev.host_out.any()
            assert dev.raw_split(lay, d_a, d_b, r, 2, 3, taps, cap=split_total) == 0
            times = dev.ctx.kernel_times()
            assert {"clip_rms_split", "clip_pick", "clip_gather_resampled_split"} <= set(times) and not {"clip_gather_split", "clip_gather_fir_split"} & set(times)
        finally:
            dev.free(d_a, d_b)
        assert dev.raw([], 2, 3, taps) == 0 and dev.raw([], 0, 0, None, host=True) == 0      # no clips: nothing to do
        assert "clip_gather_resampled" not in dev.ctx.kernel_times()
        assert dev.raw(ok, 2, 3, taps, cap=total) == 0                    # exactly the resampled total
        times = dev.ctx.kernel_times()
        assert {"clip_rms", "clip_pick", "clip_gather_resampled"} <= set(times) and not {"clip_gather", "clip_gather_fir", "clip_gather_strided"} & set(times)
        assert times["clip_gather_resampled"] > 0
    finally:
        dev.ctx.enable_timing(False)


@pytest.mark.parametrize("kind", ["f32", "pcm16"])
def test_a_table_that_stays_in_global_memory(gpu_ctx, kind):
    """clip_resample_cases.long_table_case: a table of more than TABLE_LDS entries, which no table of CASES has, through both
    sources and all four format pairs.  The contiguous f32 output against the float64 model within the bound, PCM16 out = the f32
    output converted, split = contiguous bit for bit with the seam inside the second tile's window."""
    up, down, half, tk = rc.LONG_TABLE
    taps = rc.case_taps(up, down, half, tk)
    To = rc.tile_out(up, down, len(taps))
    assert -(-len(taps) // up) * up > rc.TABLE_LDS
    src, clips, lay = rc.long_table_case(kind == "pcm16")
    n, seam = int(clips[0, 3] - clips[0, 2]), int(lay.sigma[0])
    n_out = rc.out_len(n, up, down)
    lo2, hi2 = rr.window(up, down, len(taps), n, To, n_out - To)
    assert To < n_out <= 2 * To and rr.window(up, down, len(taps), n, 0, To)[1] <= seam and lo2 < seam < hi2
    cap = n_out + 16
    want = rc.model_export(src, clips, taps, up, down)                    # computed once, shared by the four exports below
    bufs = [gpu_ctx.device_alloc(a.nbytes) for a in (src, lay.A, lay.B)] + [gpu_ctx.device_alloc(cap * 4)]
    d_src, d_a, d_b, d_out = bufs
    try:
        for d, a in zip(bufs, (src, lay.A, lay.B)):
            gpu_ctx.to_device(d, np.ascontiguousarray(a))

        def export(split, out_pcm16):
            dt = np.int16 if out_pcm16 else np.float32
            gpu_ctx.to_device(d_out, np.full(cap, CANARY[out_pcm16], dt))
            kw = dict(out_pcm16=out_pcm16, d_out=d_out, out_capacity=cap, up=up, down=down, taps=taps)
            res = (gpu_ctx.clips_export_split(lay.a(d_a), lay.b(d_b), kind == "pcm16", lay.rows, **kw) if split else
                   gpu_ctx.clips_export(d_src, kind == "pcm16", 2, src.shape[1], src.shape[1], clips, **kw))
            out = gpu_ctx.to_host(np.zeros(cap, dt), d_out)
            assert int(res["out_lens"][0]) == n_out and out[n_out:].tobytes() == np.full(cap - n_out, CANARY[out_pcm16], dt).tobytes()
            return dict(res, samples=[out[:n_out].copy()])

        got = export(False, False)
        rc.compare(got, want, f"{up}/{down} half {half} from {kind}")
        assert np.isfinite(got["samples"][0]).all(), "a read outside the clip reached an output"
        p = export(False, True)
        same_bits(p, dict(got, samples=as_pcm16(got)), "to PCM16", ("best_channel", "best_rms", "runner_up_rms"))
        for out_pcm16, whole in ((False, got), (True, p)):
            same_bits(export(True, out_pcm16), whole, f"split at {seam}, PCM16 out {out_pcm16}")
    finally:
        for d in bufs:
            gpu_ctx.device_free(d)


def test_the_index_width(fv, gpu_ctx):
    """o * down passes 2^32 inside one clip: PCM16 mono at 147/640, half 1; the model on the first and the last tile only"""
    up, down = 147, 640
    taps = rc.case_taps(up, down, 1, "sinc")
    n_taps, To = len(taps), rc.tile_out(147, 640, 1281)
    n = -(-(1 << 32) // down) * down // up + To * down // up
    n_out = rc.out_len(n, up, down)
    assert (n_out - 1) * down > (1 << 32) + (To - 8) * down and n_out * 4 + n * 2 < 96 << 20
    x = np.random.default_rng(3).integers(-15000, 15000, n + 2).astype(np.int16)
    x[0] = x[-1] = cc.SENTINEL
    d_src, d_out = gpu_ctx.device_alloc(x.nbytes), gpu_ctx.device_alloc((n_out + 16) * 4)
    try:
        gpu_ctx.to_device(d_src, x)
        gpu_ctx.to_device(d_out, np.full(n_out + 16, CANARY[False], np.float32))
        res = gpu_ctx.clips_export(d_src, True, 1, len(x), len(x), [(0, 1, 1, 1 + n)], d_out=d_out, out_capacity=n_out + 16, up=up, down=down, taps=taps)
        out = gpu_ctx.to_host(np.zeros(n_out + 16, np.float32), d_out)
    finally:
        gpu_ctx.device_free(d_src)
        gpu_ctx.device_free(d_out)
    assert int(res["out_lens"][0]) == n_out and out[n_out:].tobytes() == np.full(16, CANARY[False], np.float32).tobytes()
    clip = x[1:1 + n].astype(np.float64) / 32768.0
    last0 = (n_out - 1) // To * To
    for o0, cnt in ((0, To), (last0, n_out - last0)):
        lo, hi = rr.window(up, down, n_taps, n, o0, cnt)
        y, B = rr.resample_model(clip[lo:hi, None], taps, up, down, o0, cnt, frame_base=lo, file_frames=n)
        rr.compare(out[None, o0:o0 + cnt], y, B, up, n_taps, f"outputs from {o0}")
    assert np.isfinite(out[:n_out]).all() and np.abs(out[:n_out]).max() > 0.03
