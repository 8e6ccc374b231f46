"""The strided Recorder on the GPU (fvad_clips_export_strided(_device), fvad_clips_export_split_strided(_device),
csrc/kernels_clips_strided.hip): clip_stride_cases.py's table -- every clip of clip_cases.py at steps 2, 3 and 6 at every phase,
and per (step, phase) the clips on both sides of one and two gather tiles at the 8 sample alignments -- through all four call
forms and all four format pairs.

The yardstick is fvad_clips_export_device on the same lanes, computed once per format pair: a strided clip's pick and both RMS
values must be its bits and the samples its samples[skip::step].  Both are also held against the float64 model as
test_clips_gpu.py does (RMS within one f32 ulp).  Every device export goes into a canary-filled buffer."""
import ctypes as C

import numpy as np
import pytest

import clip_cases as cc
import clip_split_cases as sc
import clip_stride_cases as st

pytestmark = pytest.mark.gpu

INVALID, OUT_OF_RANGE, TOO_SMALL = -100, -6, -106
STRIDE = cc.N_SAMPLES + 5
CANARY = {False: np.frombuffer(np.uint32(0x7FC0BEEF).tobytes(), np.float32)[0], True: np.int16(0x5A5A)}
SLACK = 64
TABLE = st.Table()


class Device:
    """one source format on the device: the table's lanes and a canary-filled output"""

    def __init__(self, fv, ctx, pcm16):
        self.fv, self.ctx, self.pcm16 = fv, ctx, pcm16
        self.src = TABLE.source(pcm16)
        self.cap = max(cc.plan(TABLE.clips, False)[1], cc.plan(TABLE.clips, True)[1]) + SLACK
        self.host = np.full((cc.N_LANES, STRIDE), cc.SENTINEL if pcm16 else np.nan, self.src.dtype)
        self.host[:, :cc.N_SAMPLES] = self.src
        self.bufs = []
        self.d_src = self.up(self.host)
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

    def export_full(self, out_pcm16):
        self.fill(out_pcm16)
        res = self.ctx.clips_export(self.d_src, self.pcm16, cc.N_LANES, STRIDE, cc.N_SAMPLES, TABLE.clips, out_pcm16=out_pcm16,
                                    d_out=self.d_out, out_capacity=self.cap)
        return self.cut(res, TABLE.clips[:, 3] - TABLE.clips[:, 2], out_pcm16)

    def export(self, clips, skips, step, out_pcm16):
        self.fill(out_pcm16)
        res = self.ctx.clips_export(self.d_src, self.pcm16, cc.N_LANES, STRIDE, cc.N_SAMPLES, clips, out_pcm16=out_pcm16,
                                    d_out=self.d_out, out_capacity=self.cap, step=step, skips=skips)
        return self.cut(res, res["out_lens"], out_pcm16)

    def export_split(self, a, b, rows, skips, step, out_pcm16):
        self.fill(out_pcm16)
        res = self.ctx.clips_export_split(a, b, self.pcm16, rows, out_pcm16=out_pcm16, d_out=self.d_out, out_capacity=self.cap,
                                          step=step, skips=skips)
        return self.cut(res, res["out_lens"], out_pcm16)

    def raw(self, clips, step, skips, out_pcm16=False, src_format=None, d_out="own", cap=None, out_format=None, host=False, n_samples=cc.N_SAMPLES):
        """fvad_clips_export_strided(_device) itself -> status"""
        fv = self.fv
        clips = np.ascontiguousarray(np.asarray(clips, np.uint64).reshape(-1, 4))
        skips = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32))
        fn = fv.lib().fvad_clips_export_strided if host else fv.lib().fvad_clips_export_strided_device
        return fn(self.ctx.h, fv.vp(self.d_src), int(self.pcm16) if src_format is None else src_format, cc.N_LANES, STRIDE, n_samples,
                  clips.ctypes.data_as(C.POINTER(C.c_uint64)), len(clips), int(out_pcm16) if out_format is None else out_format,
                  fv.vp((self.host_out.ctypes.data if host else self.d_out) if d_out == "own" else d_out),
                  self.cap if cap is None else cap, None, None, None, None, step,
                  None if skips is None else skips.ctypes.data_as(C.POINTER(C.c_uint32)))

    def raw_split(self, lay, d_a, d_b, rows, step, skips, cap=None, host=False):
        fv = self.fv
        rows = np.ascontiguousarray(np.asarray(rows, np.uint64).reshape(-1, sc.FIELDS))
        skips = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32))
        a, b = lay.a(d_a), lay.b(d_b)
        fn = fv.lib().fvad_clips_export_split_strided if host else fv.lib().fvad_clips_export_split_strided_device
        return fn(self.ctx.h, fv.vp(a[0]), a[1], a[2], a[3], fv.vp(b[0]), b[1], b[2], b[3], int(self.pcm16),
                  rows.ctypes.data_as(C.POINTER(C.c_uint64)), len(rows), 0, fv.vp(self.host_out.ctypes.data if host else self.d_out),
                  (1024 if host else self.cap) if cap is None else cap, None, None, None, None, step,
                  None if skips is None else skips.ctypes.data_as(C.POINTER(C.c_uint32)))


@pytest.fixture(scope="module", params=[False, True], ids=["from-f32", "from-pcm16"])
def dev(request, fv, gpu_ctx):
    d = Device(fv, gpu_ctx, request.param)
    yield d
    # the sources are as they were
    assert d.ctx.to_host(np.zeros_like(d.host), d.d_src).tobytes() == d.host.tobytes()
    d.close()


@pytest.fixture(scope="module")
def full():
    """fvad_clips_export_device over the whole table and the float64 model, once per format pair"""
    cache = {}

    def get(dev, out_pcm16):
        key = (dev.pcm16, out_pcm16)
        if key not in cache:
            cache[key] = (dev.export_full(out_pcm16), cc.model_export(dev.src, TABLE.clips, out_pcm16))
            cc.compare(*cache[key], "the full-rate export against the model")
        return cache[key]
    return get


def assert_same_bits(got, want, what):
    for f in ("best_channel", "best_rms", "runner_up_rms", "offsets"):
        assert np.asarray(got[f]).tobytes() == np.asarray(want[f]).tobytes(), (what, f)
    assert got["total"] == want["total"], what
    assert len(got["samples"]) == len(want["samples"])
    for i, (g, w) in enumerate(zip(got["samples"], want["samples"])):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, "samples of clip", i)


def assert_host_form(h, d, what):
    """the host form's result h against the device form's d (with `samples`): the same bits, zeros between the slots"""
    assert all(h[f].tobytes() == d[f].tobytes() for f in ("best_channel", "best_rms", "runner_up_rms", "offsets", "out_lens")), what
    touched = np.zeros(h["total"], bool)
    for o, s in zip(h["offsets"].astype(np.int64), d["samples"]):
        assert h["out"][o:o + len(s)].tobytes() == s.tobytes(), what
        touched[o:o + len(s)] = True
    assert not h["out"][~touched].any(), what


def lens_of(idx):
    return (TABLE.clips[idx, 3] - TABLE.clips[idx, 2]).astype(np.int64)


@pytest.mark.parametrize("out_pcm16", [False, True], ids=["to-f32", "to-pcm16"])
def test_the_table_through_the_contiguous_forms(dev, full, out_pcm16):
    device, model = full(dev, out_pcm16)
    for case in TABLE.cases:
        what = f"{case}, pcm16 {dev.pcm16} -> {out_pcm16}"
        clips, skips = TABLE.clips[case.idx], TABLE.skips(case)
        got = dev.export(clips, skips, case.step, out_pcm16)
        assert_same_bits(got, st.strided_of(device, case.idx, skips, case.step, out_pcm16, lens_of(case.idx)), what)
        cc.compare(got, st.strided_of(model, case.idx, skips, case.step, out_pcm16, lens_of(case.idx)), what)
        out_lens, offsets, total = dev.fv.clips_plan_strided(lens_of(case.idx), skips, case.step, out_pcm16)
        assert np.array_equal(got["offsets"], offsets) and np.array_equal(got["out_lens"], out_lens) and got["total"] == total
        h = dev.ctx.clips_export(dev.d_src, dev.pcm16, cc.N_LANES, STRIDE, cc.N_SAMPLES, clips, out_pcm16=out_pcm16, step=case.step, skips=skips)
        assert_host_form(h, got, what)
    assert len(TABLE.cases) == 11 and all(len(c.edge) == 40 for c in TABLE.cases)


@pytest.mark.parametrize("out_pcm16", [False, True], ids=["to-f32", "to-pcm16"])
def test_the_table_through_the_split_forms(dev, full, out_pcm16):
    device, model = full(dev, out_pcm16)
    for case in TABLE.cases:
        what = f"split, {case}, pcm16 {dev.pcm16} -> {out_pcm16}"
        lay, skips = st.split_case(TABLE, case, dev.src)
        d_a, d_b = dev.up(lay.A), dev.up(lay.B)
        try:
            got = dev.export_split(lay.a(d_a), lay.b(d_b), lay.rows, skips, case.step, out_pcm16)
            lens = (lay.rows[:, 3] + lay.rows[:, 6]).astype(np.int64)
            assert_same_bits(got, st.strided_of(device, lay.base, skips, case.step, out_pcm16, lens), what)
            cc.compare(got, st.strided_of(model, lay.base, skips, case.step, out_pcm16, lens), what)
            h = dev.ctx.clips_export_split(lay.a(d_a), lay.b(d_b), dev.pcm16, lay.rows, out_pcm16=out_pcm16, step=case.step, skips=skips)
            assert_host_form(h, got, what)
            if case.phase == 0:
                # the first slice has no held buffer: d_a NULL, the rows whose seam is 0
                first = np.flatnonzero(lay.sigma == 0)
                alone = dev.export_split((None, 0, 0, 0), lay.b(d_b), lay.rows[first], skips[first], case.step, out_pcm16)
                assert_same_bits(alone, st.strided_of(device, lay.base[first], skips[first], case.step, out_pcm16, lens[first]), what + ", d_a NULL")
        finally:
            dev.free(d_a, d_b)
        # the seams around the first kept sample and around a kept sample in the middle are in the table
        k, n = int(skips[0]), int(lens[0])
        assert {max(k - 1, 0), k, k + 1} <= set(lay.sigma[lay.base == lay.base[0]]) and len(lay.rows) > 250


@pytest.mark.parametrize("out_pcm16", [False, True], ids=["to-f32", "to-pcm16"])
def test_step_1_is_the_full_rate_export(dev, full, out_pcm16):
    device, _ = full(dev, out_pcm16)
    zeros = np.zeros(len(TABLE.clips), np.uint32)
    for skips in (zeros, None):
        dev.fill(out_pcm16)
        got = dev.ctx._clips_export_strided("fvad_clips_export_strided", (dev.fv.vp(dev.d_src), int(dev.pcm16), cc.N_LANES, STRIDE, cc.N_SAMPLES),
                                            TABLE.clips, lens_of(slice(None)), out_pcm16, dev.d_out, dev.cap, 1, skips)
        assert_same_bits(dev.cut(got, got["out_lens"], out_pcm16), device, "step 1")
    case = TABLE.cases[0]
    lay, _ = st.split_case(TABLE, case, dev.src)
    d_a, d_b = dev.up(lay.A), dev.up(lay.B)
    try:
        want = dev.ctx.clips_export_split(lay.a(d_a), lay.b(d_b), dev.pcm16, lay.rows, out_pcm16=out_pcm16)
        got = dev.ctx.clips_export_split(lay.a(d_a), lay.b(d_b), dev.pcm16, lay.rows, out_pcm16=out_pcm16, step=1, skips=np.zeros(len(lay.rows), np.uint32))
        assert all(got[f].tobytes() == want[f].tobytes() for f in ("best_channel", "best_rms", "runner_up_rms", "offsets", "out"))
        assert got["total"] == want["total"]
    finally:
        dev.free(d_a, d_b)


def test_equal_formats_move_every_bit_pattern(fv, gpu_ctx):
    # random 32-bit patterns (NaNs of every payload, both infinities, denormals), -0 and the smallest denormals on kept samples,
    # and the same for 16-bit patterns, contiguous and across a seam, at steps 2, 3 and 6
    rng = np.random.default_rng(3)
    for pcm16 in (False, True):
        word, dt = (np.uint16, np.int16) if pcm16 else (np.uint32, np.float32)
        n, lanes = 3 * st.TILE + 77, 3
        X = rng.integers(0, np.iinfo(word).max, (lanes, n), dtype=word, endpoint=True)
        if not pcm16:
            X[:, 2:20:3] = np.array([0x80000000, 0x00000001, 0x7FA00001, 0xFFC12345, 0x80000001, 0x007FFFFF], np.uint32)
            assert np.isnan(X.view(np.float32)).sum() > 50
        clips = [(l, 1, a, b) for l, (a, b) in enumerate([(0, n), (5, n - 7), (2, n - 1)])]
        na = st.TILE + 5
        rows = [(1, l, a, na - a, l, 0, b - na) for l, _, a, b in clips]
        d_x, d_a, d_b = (gpu_ctx.device_alloc(X.nbytes) for _ in range(3))
        d_out = gpu_ctx.device_alloc(n * lanes * 4)
        try:
            gpu_ctx.to_device(d_x, X.view(dt))
            gpu_ctx.to_device(d_a, np.ascontiguousarray(X[:, :na]).view(dt))
            gpu_ctx.to_device(d_b, np.ascontiguousarray(X[:, na:]).view(dt))
            for step in st.STEPS:
                skips = fv.clips_phase_skips([c[2] for c in clips], step, 2 % step)
                for split in (False, True):
                    if split:
                        res = gpu_ctx.clips_export_split((d_a, lanes, na, na), (d_b, lanes, n - na, n - na), pcm16, rows, out_pcm16=pcm16,
                                                         d_out=d_out, step=step, skips=skips)
                    else:
                        res = gpu_ctx.clips_export(d_x, pcm16, lanes, n, n, clips, out_pcm16=pcm16, d_out=d_out, step=step, skips=skips)
                    out = gpu_ctx.to_host(np.zeros(res["total"], dt), d_out).view(word)
                    for (l, _, a, b), k, o in zip(clips, skips, res["offsets"].astype(np.int64)):
                        want = X[l, a + int(k):b:step]
                        assert (a + int(k)) % step == 2 % step and out[o:o + len(want)].tobytes() == want.tobytes(), (pcm16, step, split, l)
        finally:
            for d in (d_x, d_a, d_b, d_out):
                gpu_ctx.device_free(d)


@pytest.mark.parametrize("out_pcm16", [False, True], ids=["to-f32", "to-pcm16"])
def test_a_clip_is_the_same_bits_whatever_else_is_in_the_call(dev, out_pcm16):
    rng = np.random.default_rng(11)
    case = TABLE.cases[4]                                                 # step 3, phase 2
    assert (case.step, case.phase) == (3, 2)
    clips, skips = TABLE.clips[case.idx], TABLE.skips(case)
    whole = dev.export(clips, skips, 3, out_pcm16)
    rev = dev.export(clips[::-1], skips[::-1], 3, out_pcm16)
    picks = [int(np.flatnonzero(case.idx == k)[0]) for k in (TABLE.names["dup"], TABLE.names["tie-D"], int(case.edge[27]))]
    for r in picks:
        alone = dev.export(clips[r:r + 1], skips[r:r + 1], 3, out_pcm16)
        o = rng.integers(0, len(clips), 150)
        among = dev.export(np.concatenate([clips[o[:71]], clips[r:r + 1], clips[o[71:]]]), np.concatenate([skips[o[:71]], skips[r:r + 1], skips[o[71:]]]), 3, out_pcm16)
        for res, k in ((among, 71), (whole, r), (rev, len(clips) - 1 - r)):
            for f in ("best_channel", "best_rms", "runner_up_rms"):
                assert res[f][k].tobytes() == alone[f][0].tobytes(), (r, f)
            assert res["samples"][k].tobytes() == alone["samples"][0].tobytes(), r
    assert_same_bits(dev.export(clips, skips, 3, out_pcm16), whole, "a second call")


def test_refused_calls_write_nothing(dev):
    dev.fill(False)
    ok = [(1, 1, 100, 200), (2, 2, 50000, 59000)]
    total = st.plan_strided([100, 9000], [1, 2], 3, False)[2]
    for what, status, kw in (
            ("step 0", INVALID, dict(clips=ok, step=0, skips=None)),
            ("step above the limit", INVALID, dict(clips=ok, step=st.STEP_MAX + 1, skips=[0, 0])),
            ("a skip equal to the step", INVALID, dict(clips=ok, step=3, skips=[0, 3])),
            ("a skip with step 1", INVALID, dict(clips=ok, step=1, skips=[1, 0])),
            ("a clip that keeps no sample", INVALID, dict(clips=[ok[0], (1, 1, 100, 102)], step=3, skips=[0, 2])),
            ("the step's rule comes before a range's", INVALID, dict(clips=[ok[0], (1, 1, 100, cc.N_SAMPLES + 1)], step=0, skips=None)),
            ("a skip's rule comes before a range's", INVALID, dict(clips=[(1, 1, 100, cc.N_SAMPLES + 1), ok[1]], step=3, skips=[0, 3])),
            ("a clip's own rule", INVALID, dict(clips=[ok[0], (1, 0, 100, 200)], step=3, skips=[0, 0])),
            ("NULL output", INVALID, dict(clips=ok, step=3, skips=None, d_out=0)),
            ("bad output format", INVALID, dict(clips=ok, step=3, skips=None, out_format=2)),
            ("a clip past n_samples", OUT_OF_RANGE, dict(clips=[ok[0], (1, 1, 100, cc.N_SAMPLES + 1)], step=3, skips=[0, 0])),
            ("lanes past n_lanes", OUT_OF_RANGE, dict(clips=[ok[0], (cc.N_LANES - 1, 2, 0, 10)], step=3, skips=[0, 0])),
            ("capacity below the strided total", TOO_SMALL, dict(clips=ok, step=3, skips=[1, 2], cap=total - 1))):
        assert dev.raw(**kw) == status, what
        assert "fvad_clips_export" in dev.fv.lib().fvad_last_error(dev.ctx.h).decode(), what
        if "d_out" not in kw or kw["d_out"] == 0:
            assert dev.raw(host=True, **dict(kw, cap=min(kw.get("cap", 1024), 1024))) == status, what + " (host form)"
    # every clip the table lists as keeping no sample, alone and among others
    for case in TABLE.cases:
        for k in case.refused:
            skip = TABLE.skips(case, [k])
            assert dev.raw([TABLE.clips[k]], case.step, skip) == INVALID, (case, k)
            assert dev.raw([ok[0], TABLE.clips[k]], case.step, [0, skip[0]]) == INVALID, (case, k)
    assert sum(len(c.refused) for c in TABLE.cases) > 20
    # the split form: the same new rules, after the rows' own and before the ranges'
    lay, skips = st.split_case(TABLE, TABLE.cases[2], dev.src)
    d_a, d_b = dev.up(lay.A), dev.up(lay.B)
    try:
        r = lay.rows[(lay.rows[:, 3] > 0) & (lay.rows[:, 6] > 0)][:2]
        past = r.copy()
        past[1, 2] = lay.a_samples                                        # a piece past A's samples
        n1 = int(r[1, 3] + r[1, 6])
        for what, status, kw in (
                ("step 0", INVALID, dict(rows=r, step=0, skips=None)),
                ("step above the limit", INVALID, dict(rows=r, step=17, skips=None)),
                ("a skip equal to the step", INVALID, dict(rows=r, step=3, skips=[2, 3])),
                ("a skip's rule comes before a range's", INVALID, dict(rows=past, step=3, skips=[3, 0])),
                ("a row's own rule", INVALID, dict(rows=[tuple(r[0]), (0,) + tuple(r[1][1:])], step=3, skips=None)),
                ("a piece past its buffer", OUT_OF_RANGE, dict(rows=past, step=3, skips=None)),
                ("capacity below the strided total", TOO_SMALL, dict(rows=r, step=3, skips=None, cap=st.plan_strided([int(r[0, 3] + r[0, 6]), n1], None, 3, False)[2] - 1))):
            assert dev.raw_split(lay, d_a, d_b, **kw) == status, what
            assert "fvad_clips_export_split" in dev.fv.lib().fvad_last_error(dev.ctx.h).decode(), what
            assert dev.raw_split(lay, d_a, d_b, host=True, **dict(kw, cap=min(kw.get("cap", 1024), 1024))) == status, what + " (host form)"
        one = [tuple(r[0][:3]) + (2,) + tuple(r[0][4:6]) + (0,)]          # two samples, skip 2: nothing kept
        assert dev.raw_split(lay, d_a, d_b, one, 3, [2]) == INVALID
        # nothing was written by any refused call
        assert dev.read(False).tobytes() == np.full(dev.cap, CANARY[False], np.float32).tobytes()
        assert not dev.host_out.any()
        assert dev.ctx.to_host(np.zeros_like(lay.A), d_a).tobytes() == lay.A.tobytes()
        assert dev.raw_split(lay, d_a, d_b, r, 3, None, cap=st.plan_strided([int(r[0, 3] + r[0, 6]), n1], None, 3, False)[2]) == 0
    finally:
        dev.free(d_a, d_b)
    assert dev.raw([], 3, None) == 0 and dev.raw([], 0, None, host=True) == 0     # no clips: nothing to do
    assert dev.raw(ok, 3, [1, 2], cap=total) == 0                          # exactly the strided total


def test_kernel_times_name_the_strided_gathers(dev):
    case = TABLE.cases[4]
    lay, skips = st.split_case(TABLE, case, dev.src)
    d_a, d_b = dev.up(lay.A), dev.up(lay.B)
    dev.ctx.enable_timing(True)
    try:
        dev.ctx.kernel_times()                                            # (drop what earlier calls left)
        dev.export(TABLE.clips[case.idx], TABLE.skips(case), case.step, False)
        times = dev.ctx.kernel_times()
        assert {"clip_rms", "clip_pick", "clip_gather_strided"} <= set(times) and "clip_gather" not in times and times["clip_gather_strided"] > 0
        dev.export_split(lay.a(d_a), lay.b(d_b), lay.rows, skips, case.step, False)
        times = dev.ctx.kernel_times()
        assert {"clip_rms_split", "clip_pick", "clip_gather_strided_split"} <= set(times) and "clip_gather_split" not in times
    finally:
        dev.ctx.enable_timing(False)
        dev.free(d_a, d_b)
