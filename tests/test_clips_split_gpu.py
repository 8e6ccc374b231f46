"""The split-source Recorder on the GPU (fvad_clips_export_split_device / fvad_clips_export_split, csrc/clip_source_device.h):
every clip of clip_cases.py's table cut at every seam of clip_split_cases.py, its two pieces in two separately allocated device
buffers with their own lane counts, strides and lane order, NaN (f32) or a sentinel (PCM16) everywhere around the pieces.

The yardstick is fvad_clips_export_device on the unsplit lanes, computed once per format pair: a split clip's samples, pick, both
RMS values and offsets must be its bits.  Both are also held against the float64 model as test_clips_gpu.py does (RMS within one
f32 ulp)."""
import ctypes as C

import numpy as np
import pytest

import clip_cases as cc
import clip_split_cases as sc

pytestmark = pytest.mark.gpu

INVALID, OUT_OF_RANGE, TOO_SMALL = -100, -6, -106
STRIDE = cc.N_SAMPLES + 5
CANARY = {False: np.frombuffer(np.uint32(0x7FC0BEEF).tobytes(), np.float32)[0], True: np.int16(0x5A5A)}
SLACK = 64


class Device:
    """one source format on the device: the split table's A and B, the unsplit lanes, a canary-filled output"""

    def __init__(self, fv, ctx, pcm16):
        self.fv, self.ctx, self.pcm16 = fv, ctx, pcm16
        self.t = t = sc.SplitTable(pcm16)
        self.total = max(sc.plan_rows(t.rows, False)[1], sc.plan_rows(t.rows, True)[1])
        self.cap = self.total + SLACK
        host = np.full((cc.N_LANES, STRIDE), cc.SENTINEL if pcm16 else np.nan, t.src.dtype)
        host[:, :cc.N_SAMPLES] = t.src
        self.bufs = []
        self.d_src = self._up(host)
        self.d_a, self.d_b = self._up(t.A), self._up(t.B)
        self.d_out = ctx.device_alloc(self.cap * 4)
        self.bufs.append(self.d_out)
        self.host_out = np.zeros(1024, np.float32)

    def _up(self, arr):
        d = self.ctx.device_alloc(arr.nbytes)
        self.bufs.append(d)
        self.ctx.to_device(d, np.ascontiguousarray(arr))
        return d

    def close(self):
        for d in self.bufs:
            self.ctx.device_free(d)

    def fill(self, out_pcm16):
        self.ctx.to_device(self.d_out, np.full(self.cap, CANARY[out_pcm16], np.int16 if out_pcm16 else np.float32))

    def read(self, out_pcm16):
        return self.ctx.to_host(np.zeros(self.cap, np.int16 if out_pcm16 else np.float32), self.d_out)

    def _cut(self, res, lens, out_pcm16):
        out = self.read(out_pcm16)
        touched = np.zeros(self.cap, bool)
        res["samples"] = []
        for n, o in zip(lens, res["offsets"].astype(np.int64)):
            res["samples"].append(out[o:o + n].copy())
            touched[o:o + n] = True
        assert out[~touched].tobytes() == np.full(int((~touched).sum()), CANARY[out_pcm16], out.dtype).tobytes(), "a canary outside the clips' samples changed"
        return res

    def export_unsplit(self, out_pcm16):
        self.fill(out_pcm16)
        clips = self.t.clips
        res = self.ctx.clips_export(self.d_src, self.pcm16, cc.N_LANES, STRIDE, cc.N_SAMPLES, clips, out_pcm16=out_pcm16,
                                    d_out=self.d_out, out_capacity=self.cap)
        return self._cut(res, (clips[:, 3] - clips[:, 2]).astype(np.int64), out_pcm16)

    def export(self, rows, out_pcm16, a=None, b=None):
        """fvad_clips_export_split_device into the canary-filled buffer -> the result with `samples` cut from the output"""
        self.fill(out_pcm16)
        rows = np.asarray(rows, np.uint64).reshape(-1, sc.FIELDS)
        res = self.ctx.clips_export_split(a or self.t.a(self.d_a), b or self.t.b(self.d_b), self.pcm16, rows, out_pcm16=out_pcm16,
                                          d_out=self.d_out, out_capacity=self.cap)
        return self._cut(res, (rows[:, 3] + rows[:, 6]).astype(np.int64), out_pcm16)

    def raw(self, rows, out_pcm16=False, a=None, b=None, src_format=None, d_out="own", cap=None, out_format=None, host=False):
        """the C call itself -> status"""
        fv = self.fv
        rows = np.ascontiguousarray(np.asarray(rows, np.uint64).reshape(-1, sc.FIELDS))
        a, b = a or self.t.a(self.d_a), b or self.t.b(self.d_b)
        fn = fv.lib().fvad_clips_export_split if host else fv.lib().fvad_clips_export_split_device
        return fn(self.ctx.h, fv.vp(a[0]), a[1], a[2], a[3], fv.vp(b[0]), b[1], b[2], b[3],
                  int(self.pcm16) if src_format is None else src_format,
                  rows.ctypes.data_as(C.POINTER(C.c_uint64)) if len(rows) else None, len(rows),
                  int(out_pcm16) if out_format is None else out_format,
                  fv.vp((self.host_out.ctypes.data if host else self.d_out) if d_out == "own" else d_out),
                  self.cap if cap is None else cap, None, None, None, None)


@pytest.fixture(scope="module", params=[False, True], ids=["from-f32", "from-pcm16"])
def dev(request, fv, gpu_ctx):
    d = Device(fv, gpu_ctx, request.param)
    yield d
    d.close()


@pytest.fixture(scope="module")
def unsplit():
    """fvad_clips_export_device on the unsplit lanes and the float64 model, once per format pair"""
    cache = {}

    def get(dev, out_pcm16):
        key = (dev.pcm16, out_pcm16)
        if key not in cache:
            cache[key] = (dev.export_unsplit(out_pcm16), cc.model_export(dev.t.src, dev.t.clips, out_pcm16))
        return cache[key]
    return get


def assert_same_bits(got, want, what):
    for f in ("best_channel", "best_rms", "runner_up_rms", "offsets"):
        assert np.asarray(got[f]).tobytes() == np.asarray(want[f]).tobytes(), (what, f)
    assert got["total"] == want["total"], what
    for i, (g, w) in enumerate(zip(got["samples"], want["samples"])):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, "samples of row", i)


@pytest.mark.parametrize("out_pcm16", [False, True], ids=["to-f32", "to-pcm16"])
def test_every_seam_gives_the_unsplit_bits(dev, unsplit, out_pcm16):
    t = dev.t
    device, model = unsplit(dev, out_pcm16)
    cc.compare(device, model, "the unsplit export against the model")
    got = dev.export(t.rows, out_pcm16)
    what = f"pcm16 {dev.pcm16} -> {out_pcm16}"
    assert_same_bits(got, sc.expected_rows(device, t.base, t.rows, out_pcm16), what)
    cc.compare(got, sc.expected_rows(model, t.base, t.rows, out_pcm16), what)
    assert np.array_equal(got["offsets"], dev.fv.clips_plan([(0, 1, 0, int(r[3] + r[6])) for r in t.rows], out_pcm16)[0])
    by = 2 if dev.pcm16 else 4
    assert len(t.offsets_mod16()) == (16 // by) ** 2 and len(t.rows) > 400


def test_the_carry_moves_every_bit_pattern(fv, gpu_ctx):
    # equal formats, one mono clip per lane, as the harness carries a tail from one held buffer to the other: random 32-bit
    # patterns (NaNs of every payload, both infinities, denormals) plus -0 and the smallest denormals at the seam, and the same
    # for 16-bit patterns; out_offsets are the lanes' new bases
    rng = np.random.default_rng(3)
    T = sc.T
    for pcm16 in (False, True):
        word = np.uint16 if pcm16 else np.uint32
        dt = np.int16 if pcm16 else np.float32
        na, nb, lanes = 2 * T + 77, 3 * T + 5, 5
        A = rng.integers(0, np.iinfo(word).max, (lanes, na), dtype=word, endpoint=True)
        B = rng.integers(0, np.iinfo(word).max, (lanes + 2, nb), dtype=word, endpoint=True)
        if not pcm16:
            A[:, -3:] = [0x80000000, 0x00000001, 0x7FA00001]          # -0, the smallest denormal, a signalling NaN with a payload
            B[:, :3] = [0xFFC12345, 0x80000001, 0x007FFFFF]            # a negative quiet NaN, denormals
            assert np.isnan(A.view(np.float32)).sum() > 50
        rows = []
        for l, (from_a, len_a, len_b) in enumerate([(0, na, nb), (5, na - 5, 0), (0, 0, nb - 1), (T + 3, T + 74, 9), (na - 1, 1, 2 * T)]):
            rows.append((1, l, from_a, len_a, l + 2, 0 if l != 2 else 1, len_b))
        d_a, d_b = gpu_ctx.device_alloc(A.nbytes), gpu_ctx.device_alloc(B.nbytes)
        total = sc.plan_rows(rows, pcm16)[1]
        d_out = gpu_ctx.device_alloc(total * A.itemsize)
        try:
            gpu_ctx.to_device(d_a, A.view(dt))
            gpu_ctx.to_device(d_b, B.view(dt))
            res = gpu_ctx.clips_export_split((d_a, lanes, na, na), (d_b, lanes + 2, nb, nb), pcm16, rows, out_pcm16=pcm16, d_out=d_out)
            out = gpu_ctx.to_host(np.zeros(total, dt), d_out).view(word)
        finally:
            for d in (d_a, d_b, d_out):
                gpu_ctx.device_free(d)
        assert np.array_equal(res["offsets"], sc.plan_rows(rows, pcm16)[0]) and not res["best_channel"].any()
        for (_, la, fa, n1, lb, fb, n2), o in zip(rows, res["offsets"].astype(np.int64)):
            want = np.concatenate([A[la, fa:fa + n1], B[lb, fb:fb + n2]])
            assert out[o:o + n1 + n2].tobytes() == want.tobytes()


@pytest.mark.parametrize("out_pcm16", [False, True], ids=["to-f32", "to-pcm16"])
def test_a_row_is_the_same_bits_whatever_else_is_in_the_call(dev, out_pcm16):
    rng = np.random.default_rng(11)
    t = dev.t
    mid = [r for r in range(len(t.rows)) if 0 < t.sigma[r] < int(t.rows[r][3] + t.rows[r][6])]
    picks = [next(r for r in mid if t.base[r] == t.names[name] and t.sigma[r] == s) for name, s in (("dup", sc.T + 1), ("tie-D", 3), ("last", 1500))]
    whole = dev.export(t.rows, out_pcm16)
    rev = dev.export(t.rows[::-1], out_pcm16)
    for r in picks:
        alone = dev.export(t.rows[r:r + 1], out_pcm16)
        others = t.rows[rng.integers(0, len(t.rows), 150)]
        among = dev.export(np.concatenate([others[:71], t.rows[r:r + 1], others[71:]]), out_pcm16)
        for res, k in ((among, 71), (whole, r), (rev, len(t.rows) - 1 - r)):
            for f in ("best_channel", "best_rms", "runner_up_rms"):
                assert res[f][k].tobytes() == alone[f][0].tobytes(), (r, f)
            assert res["samples"][k].tobytes() == alone["samples"][0].tobytes(), r
    again = dev.export(t.rows, out_pcm16)                              # two identical calls: identical bits
    assert_same_bits(again, whole, "a second call")


def test_host_export_equals_device_export(dev):
    t = dev.t
    for out_pcm16 in (False, True):
        d = dev.export(t.rows, out_pcm16)
        h = dev.ctx.clips_export_split(t.a(dev.d_a), t.b(dev.d_b), dev.pcm16, t.rows, out_pcm16=out_pcm16)
        assert all(h[f].tobytes() == d[f].tobytes() for f in ("best_channel", "best_rms", "runner_up_rms", "offsets"))
        touched = np.zeros(h["total"], bool)
        for r, o, s in zip(t.rows.astype(np.int64), h["offsets"].astype(np.int64), d["samples"]):
            n = r[3] + r[6]
            assert h["out"][o:o + n].tobytes() == s.tobytes()
            touched[o:o + n] = True
        assert not h["out"][~touched].any()                             # the padding between slots comes back as zeros


def test_no_held_buffer(dev, unsplit):
    # the first slice: d_a NULL, every a_len 0 -- the rows with sigma 0 as they are, and B alone
    t = dev.t
    first = np.flatnonzero(t.sigma == 0)
    got = dev.export(t.rows[first], False, a=(None, 0, 0, 0))
    assert_same_bits(got, sc.expected_rows(unsplit(dev, False)[0], t.base[first], t.rows[first], False), "d_a NULL")
    # and the mirror image: everything in A, d_b NULL
    last = np.flatnonzero(t.rows[:, 6] == 0)
    got = dev.export(t.rows[last], False, b=(None, 0, 0, 0))
    assert_same_bits(got, sc.expected_rows(unsplit(dev, False)[0], t.base[last], t.rows[last], False), "d_b NULL")


def test_errors_come_back_before_any_launch(dev):
    t = dev.t
    dev.fill(False)
    both = t.rows[(t.rows[:, 3] > 0) & (t.rows[:, 6] > 0)]
    ok = [tuple(int(v) for v in both[0]), tuple(int(v) for v in both[-1])]
    A, B = t.a(dev.d_a), t.b(dev.d_b)
    row = list(ok[0])

    def changed(**kw):
        r = list(row)
        for k, v in kw.items():
            r[("n_channels", "a_lane", "a_from", "a_len", "b_lane", "b_from", "b_len").index(k)] = v
        return [ok[1], tuple(r)]
    by = 2 if dev.pcm16 else 4
    for what, status, kw in (
            ("NULL output", INVALID, dict(rows=ok, d_out=0)),
            ("bad source format", INVALID, dict(rows=ok, src_format=2)),
            ("bad output format", INVALID, dict(rows=ok, out_format=-1)),
            ("NULL A that a row reads", INVALID, dict(rows=ok, a=(None,) + A[1:])),
            ("NULL B that a row reads", INVALID, dict(rows=ok, b=(None,) + B[1:])),
            ("misaligned A", INVALID, dict(rows=ok, a=(dev.d_a + 1,) + A[1:])),
            ("misaligned B", INVALID, dict(rows=ok, b=(dev.d_b + by // 2,) + B[1:])),
            ("misaligned output", INVALID, dict(rows=ok, d_out=dev.d_out + 4)),
            ("A's stride below its samples", INVALID, dict(rows=ok, a=(A[0], A[1], A[3] - 1, A[3]))),
            ("B's stride below its samples", INVALID, dict(rows=ok, b=(B[0], B[1], B[3] - 1, B[3]))),
            ("both lengths 0", INVALID, dict(rows=changed(a_len=0, b_len=0))),
            ("no channels", INVALID, dict(rows=changed(n_channels=0))),
            ("A's piece past its samples", OUT_OF_RANGE, dict(rows=changed(a_from=t.a_samples - row[3] + 1))),
            ("A's lanes past its lanes", OUT_OF_RANGE, dict(rows=changed(a_lane=sc.A_LANES - row[0] + 1))),
            ("B's piece past its samples", OUT_OF_RANGE, dict(rows=changed(b_from=t.b_samples - row[6] + 1))),
            ("B's lanes past its lanes", OUT_OF_RANGE, dict(rows=changed(b_lane=sc.B_LANES))),
            ("capacity below the total", TOO_SMALL, dict(rows=ok, cap=sc.plan_rows(ok, False)[1] - 1)),
            ("the output inside A", INVALID, dict(rows=ok, d_out=dev.d_a + 64)),
            ("the output inside B", INVALID, dict(rows=ok, d_out=dev.d_b + 4096))):
        assert dev.raw(**kw) == status, what
        assert "fvad_clips_export_split" in dev.fv.lib().fvad_last_error(dev.ctx.h).decode(), what
        if "d_out" not in kw or kw["d_out"] == 0:                       # (a host buffer has no alignment rule and is no device range)
            assert dev.raw(host=True, **dict(kw, cap=min(kw.get("cap", 1024), 1024))) == status, what + " (host form)"
    assert dev.raw([]) == 0 and dev.raw([], host=True) == 0              # no clips: nothing to do
    out = dev.read(False)
    assert out.tobytes() == np.full(dev.cap, CANARY[False], np.float32).tobytes()   # every canary untouched by the refused calls
    assert not dev.host_out.any()
    # the sources are as they were: the outputs aimed at them were refused
    assert dev.ctx.to_host(np.zeros_like(t.A), dev.d_a).tobytes() == t.A.tobytes()
    assert dev.ctx.to_host(np.zeros_like(t.B), dev.d_b).tobytes() == t.B.tobytes()
    assert dev.raw(ok, cap=sc.plan_rows(ok, False)[1]) == 0              # exactly the plan's total


def test_kernel_times_name_the_three_kernels(dev):
    dev.ctx.enable_timing(True)
    try:
        dev.ctx.kernel_times()                                            # (drop what earlier calls left)
        dev.export(dev.t.rows, False)
        times = dev.ctx.kernel_times()
    finally:
        dev.ctx.enable_timing(False)
    names = ("clip_rms_split", "clip_pick", "clip_gather_split")
    assert set(names) <= set(times) and all(times[k] > 0 for k in names) and "clip_rms" not in times and "clip_gather" not in times
