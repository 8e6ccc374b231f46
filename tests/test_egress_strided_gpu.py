"""The strided resampling egress on the GPU (fvad_egress_resample_strided_device, fvad_egress_resample_strided): the case
tables of egress_strided_cases.py -- the rows of egress_resample_cases.py `step` apart in their lanes with NaN on EVERY other lane
sample -- as f32 files against the float64 model within its computed bound, as PCM16 / PCM24 files byte for byte against the
conversion of those f32 values, and byte for byte against what fvad_egress_resample_device (the parent's kernel, the yardstick)
writes over a compacted copy of the lanes; the host form through a small ring; streams cut into rows; the invariances; the
refused calls; a row far into a long stream; and 1/1 with the tap 1.0 at step 3 against fvad_egress over every third sample."""
import ctypes as C

import numpy as np
import pytest

import egress_cases as ec
import egress_resample_cases as er
import egress_strided_cases as es
import ingest_resample_cases as rc

pytestmark = pytest.mark.gpu

INVALID, RANGE = -100, -6
SMALL_RING = "6000"   # bytes: the tables' largest rows cross it several times


class Device:
    """a case's strided table with its lanes on the device; the model, the all-f32 run and the expected bytes computed once"""

    def __init__(self, fv, ctx, case):
        self.fv, self.ctx = fv, ctx
        self.up, self.down, _, self.step = case
        self.taps = es.case_taps(case)
        self.base = er.case_table(self.up, self.down, self.taps.size)
        self.t = es.strided(self.base, self.step, seed=self.step)
        self.t32 = er.twin_f32(self.t)
        self.rows, self.out_bytes = self.t["rows"], self.t["out_bytes"]
        self.out_in = er.canaries(self.out_bytes)
        self.model = er.model(self.t, self.taps, self.up, self.down)   # computed once, shared, never changed
        self.d_lanes = ctx.device_alloc(self.t["lanes"].nbytes)
        ctx.to_device(self.d_lanes, self.t["lanes"])
        self.d_out = ctx.device_alloc(max(self.out_bytes, self.t32["out_bytes"]))
        self.out32 = self.want = None

    def close(self):
        self.ctx.device_free(self.d_lanes)
        self.ctx.device_free(self.d_out)

    def geom(self, t=None):
        t = self.t if t is None else t
        return dict(d_lanes=self.d_lanes, n_lanes=t["n_lanes"], lane_stride=t["lane_stride"], n_samples=t["n_samples"])

    def call(self, rows, **kw):
        self.ctx.egress_resample_strided(rows, self.up, self.down, self.taps, self.step, **kw)

    def run32(self):
        """the all-f32 table through the device form -> its bytes"""
        n = self.t32["out_bytes"]
        self.ctx.to_device(self.d_out, er.canaries(n))
        self.call(self.t32["rows"], out=self.d_out, out_bytes=n, **self.geom())
        return self.ctx.to_host(np.zeros(n, np.uint8), self.d_out)

    def expected(self):
        """the table's bytes: the conversion of what the library wrote as f32 files (held against the model before it is used)"""
        if self.want is None:
            self.out32 = self.run32()
            er.compare_f32(self.out32, self.t32, self.model, self.up, self.taps.size, "fvad_egress_resample_strided_device, f32 files")
            self.want = er.bytes_from_f32(self.t, self.t32, self.out32)
        return self.want

    def fill(self):
        self.ctx.to_device(self.d_out, self.out_in)

    def read(self):
        return self.ctx.to_host(np.zeros_like(self.out_in), self.d_out)

    def device_form(self, rows):
        self.call(rows, out=self.d_out, out_bytes=self.out_bytes, **self.geom())

    def host_form(self, rows, out=None):
        out = self.out_in.copy() if out is None else out
        self.call(rows, out=[out] * len(rows), **self.geom())
        return out

    def status(self, rows, host=False, out="own", out_bytes=None, src_format=0, d_lanes="own", up=None, taps="own", n_samples=None, stride=None, host_buf=None,
               step=None):
        """the C call itself -> status"""
        fv = self.fv
        snk = np.ascontiguousarray(np.asarray(self.rows[:1] if rows is None else rows, np.uint64).reshape(-1, 10))
        ptr = snk.ctypes.data_as(C.POINTER(C.c_uint64)) if rows is not None else None   # (None: a NULL table of one row)
        tp = fv.fptr(self.taps) if isinstance(taps, str) else taps
        head = (self.ctx.h, fv.vp(self.d_lanes if isinstance(d_lanes, str) else d_lanes), src_format, self.t["n_lanes"],
                self.t["lane_stride"] if stride is None else stride, self.t["n_samples"] if n_samples is None else n_samples, ptr, len(snk),
                self.up if up is None else up, self.down, tp, self.taps.size, self.step if step is None else step)
        if host:
            ptrs = (fv.vp * max(len(snk), 1))(*([host_buf.ctypes.data] * len(snk)))
            return fv.lib().fvad_egress_resample_strided(*head, ptrs if isinstance(out, str) else out)
        return fv.lib().fvad_egress_resample_strided_device(*head, fv.vp(self.d_out if isinstance(out, str) else out),
                                                            self.out_bytes if out_bytes is None else out_bytes)


@pytest.fixture(scope="module", params=es.CASES, ids=es.case_id)
def dev(request, fv, gpu_ctx):
    d = Device(fv, gpu_ctx, request.param)
    yield d
    d.close()


def test_case_table_matches_the_model(dev):
    # every row as an f32 file: within gamma(up, n_taps) * B + one ulp of the float64 model, no NaN (no off-stride sample and
    # nothing around a row reached a sum), every byte between the rows still the canary.  Then the table itself -- PCM16, PCM24
    # and f32 files, odd byte offsets, rows that touch: byte for byte the conversion of those f32 values.
    want = dev.expected()
    dev.fill()
    dev.device_form(dev.rows)
    ec.compare(dev.read(), want, "fvad_egress_resample_strided_device")


def test_bytes_equal_the_parents_over_compacted_lanes(dev):
    # the yardstick is fvad_egress_resample_device, the parent's kernel, over the lanes it would be given for the same rows
    ctx, c = dev.ctx, es.compacted(dev.t)
    d_l = ctx.device_alloc(c["lanes"].nbytes)
    try:
        ctx.to_device(d_l, c["lanes"])
        dev.fill()
        ctx.egress_resample(c["rows"], dev.up, dev.down, dev.taps, d_lanes=d_l, n_lanes=c["n_lanes"], lane_stride=c["lane_stride"], n_samples=c["n_samples"],
                            out=dev.d_out, out_bytes=dev.out_bytes)
        parent = dev.read()
    finally:
        ctx.device_free(d_l)
    assert np.any(parent != dev.out_in)
    dev.fill()
    dev.device_form(dev.rows)
    ec.compare(dev.read(), parent, "fvad_egress_resample_strided_device against fvad_egress_resample_device over compacted lanes")
    if dev.step == 1:   # the same lanes: the parent's host form as well
        out = dev.out_in.copy()
        ctx.egress_resample(dev.rows, dev.up, dev.down, dev.taps, out=[out] * len(dev.rows), **dev.geom())
        ec.compare(dev.host_form(dev.rows), out, "step 1 against fvad_egress_resample over the same lanes")
        ec.compare(out, parent, "fvad_egress_resample, host form")


@pytest.mark.parametrize("ring", [SMALL_RING, None], ids=["small-ring", "default-ring"])
def test_host_form_equals_device_form_however_the_ring_cuts(dev, ring):
    want = dev.expected()
    with dev.ctx.options(ingest_ring_bytes=ring):
        ec.compare(dev.host_form(dev.rows), want, f"fvad_egress_resample_strided, ring {ring}")


def test_streams_cut_into_rows_give_the_one_row_bytes(dev):
    # every big stream again, cut at outputs that are no multiple of 4; each piece is given exactly its fvad_resample_window, at
    # a src_offset of its own in a fresh lane buffer that is NaN everywhere else, off the stride included
    want = dev.expected()
    ctx, fv, step = dev.ctx, dev.fv, dev.step
    for i in dev.t["big"]:
        row = dev.rows[i]
        at, n_out, Cn, fmt = (int(v) for v in row[:4])
        nb = n_out * Cn * er.SAMPLE_BYTES[fmt]
        cuts = [1, 7, n_out // 3 | 1, (n_out // 3 | 1) + 1, n_out // 2 + 2, n_out - 3]
        pieces = er.slices(row, cuts, dev.up, dev.down, dev.taps.size)
        x = dev.t["data"][i]
        cur, placed = 0, []
        for k, (p, lo, hi) in enumerate(pieces):
            assert (lo, hi) == fv.resample_window(dev.up, dev.down, dev.taps.size, int(row[8]), p[9], p[1])
            src = cur + 1 + (k - (cur + 1)) % 4
            placed.append((p[0] - at + 5, p[1], p[2], p[3], 1, src) + p[6:])
            cur = src + ((hi - lo - 1) * step + 1 if hi > lo else 0)
        n_samples = cur + 1
        lanes = np.full((Cn + 2, n_samples + 2), np.nan, np.float32)
        for (p, lo, hi), q in zip(pieces, placed):
            if hi > lo:
                lanes[1:1 + Cn, q[5]:q[5] + (hi - lo - 1) * step + 1:step] = x[lo:hi].T
        d_l, d_o = ctx.device_alloc(lanes.nbytes), ctx.device_alloc(nb + 8)
        try:
            ctx.to_device(d_l, lanes)
            ctx.to_device(d_o, er.canaries(nb + 8))
            dev.call(placed[::-1], d_lanes=d_l, n_lanes=Cn + 2, lane_stride=n_samples + 2, n_samples=n_samples, out=d_o, out_bytes=nb + 8)
            got = ctx.to_host(np.zeros(nb + 8, np.uint8), d_o)
        finally:
            ctx.device_free(d_l)
            ctx.device_free(d_o)
        ec.compare(got, np.concatenate([er.canaries(5), want[at:at + nb], er.canaries(3)]), f"row {i} in {len(pieces)} pieces")


def test_order_and_reruns_change_nothing(dev):
    want = dev.expected()
    dev.fill()
    dev.device_form(dev.rows[::-1])
    ec.compare(dev.read(), want, "the rows reversed")
    dev.device_form(dev.rows)                          # a second run over the bytes the first one wrote
    ec.compare(dev.read(), want, "a second run")
    dev.fill()
    for row in dev.rows:
        dev.device_form(row[None])
    ec.compare(dev.read(), want, "one row per call")
    out = dev.out_in.copy()
    with dev.ctx.options(ingest_ring_bytes=SMALL_RING):
        dev.host_form(dev.rows[::2], out)
        dev.host_form(dev.rows[1::2][::-1], out)
    ec.compare(out, want, "two host calls")


def test_refused_calls_leave_the_canaries_alone(dev):
    dev.fill()
    host_buf = dev.out_in.copy()
    good = dev.rows[dev.t["big"][0]].copy()
    last = int(good[5]) + (int(good[7]) - 1) * dev.step   # the row's last strided lane sample

    def edit(col, value):
        r = good.copy()
        r[col] = value
        return r

    for host in (False, True):
        kw = dict(host=host, host_buf=host_buf)
        assert dev.status(good, d_lanes=None, **kw) == INVALID
        assert dev.status(good, out=None, **kw) == INVALID
        assert dev.status(None, **kw) == INVALID
        assert dev.status(good, src_format=1, **kw) == INVALID and dev.status(good, src_format=2, **kw) == INVALID   # PCM16 lanes are refused
        assert dev.status(good, up=0, **kw) == INVALID and dev.status(good, up=641, **kw) == INVALID
        assert dev.status(good, step=0, **kw) == INVALID and dev.status(good, step=17, **kw) == INVALID            # the step's rules
        assert dev.status(good, taps=None, **kw) == INVALID
        assert dev.status(edit(3, 3), **kw) == INVALID
        assert dev.status(edit(2, 0), **kw) == INVALID and dev.status(edit(2, 65), **kw) == INVALID
        assert dev.status(edit(9, 1), **kw) == INVALID                                          # one output past the stream's last
        assert dev.status(edit(7, int(good[7]) - 1), **kw) == INVALID                           # the window's last frame is not given
        assert dev.status(np.stack([good, good]), **kw) == INVALID                              # overlapping bytes
        assert dev.status(good, d_lanes=dev.d_lanes + 2, **kw) == INVALID                       # lanes not aligned to their samples
        assert dev.status(good, stride=dev.t["n_samples"] - 1, **kw) == INVALID
        assert dev.status(edit(4, dev.t["n_lanes"]), **kw) == RANGE
        assert dev.status(good, n_samples=last, **kw) == RANGE                                  # the strided range rule: the last sample at n_samples
        assert dev.status(edit(0, (1 << 64) - 1), **kw) == RANGE                                # byte_offset + bytes wraps (the host form: the address)
    assert dev.status(good, out_bytes=int(good[0]) + int(good[1]) * int(good[2]) * er.SAMPLE_BYTES[int(good[3])] - 1) == RANGE
    fv = dev.fv
    rows = np.ascontiguousarray(np.stack([good, edit(0, int(good[0]) + 1)]))
    head = (dev.ctx.h, fv.vp(dev.d_lanes), 0, dev.t["n_lanes"], dev.t["lane_stride"], dev.t["n_samples"], rows.ctypes.data_as(C.POINTER(C.c_uint64)))
    tail = (dev.up, dev.down, fv.fptr(dev.taps), dev.taps.size, dev.step)
    assert fv.lib().fvad_egress_resample_strided(*head, 1, *tail, (fv.vp * 1)(None)) == INVALID       # a row with outputs and no bytes
    assert fv.lib().fvad_egress_resample_strided(*head, 2, *tail, (fv.vp * 2)(host_buf.ctypes.data + 1, host_buf.ctypes.data)) == INVALID   # the same bytes through two bases
    empty = np.zeros((0, 10), np.uint64)
    assert dev.status(empty) == 0 and dev.status(empty, host=True, host_buf=host_buf) == 0    # nothing to do
    ec.compare(dev.read(), dev.out_in, "the device canaries after the refused calls")
    ec.compare(host_buf, dev.out_in, "the host canaries after the refused calls")
    with pytest.raises(fv.FvadError):   # the binding's own bounds check of a host buffer
        dev.call(good[None], out=[host_buf[:int(good[0])]], **dev.geom())
    # the last strided sample at n_samples - 1 is accepted and the bytes are the table's
    dev.call(good[None], out=dev.d_out, out_bytes=dev.out_bytes, **dict(dev.geom(), n_samples=last + 1))
    at, nb = int(good[0]), int(good[1]) * int(good[2]) * er.SAMPLE_BYTES[int(good[3])]
    want = dev.out_in.copy()
    want[at:at + nb] = dev.expected()[at:at + nb]
    ec.compare(dev.read(), want, "the range rule's boundary")


def test_a_row_without_outputs_touches_nothing(dev):
    dev.fill()
    row = np.array([[dev.out_bytes, 0, 2, er.PCM16, 1, 3, 0, 0, 100, 0]], np.uint64)
    dev.device_form(row)
    ec.compare(dev.read(), dev.out_in, "a row without outputs, device form")
    row[0, 0] = dev.out_bytes + 12345   # the host form: no buffer at all, whatever byte_offset says
    dev.call(row, out=[None], **dev.geom())
    ec.compare(dev.read(), dev.out_in, "a row without outputs, host form")


def test_kernel_times_name_egress_strided(dev):
    ctx = dev.ctx
    was = ctx.timing
    ctx.enable_timing(True)
    try:
        ctx.kernel_times()
        dev.device_form(dev.rows)
        times = ctx.kernel_times()
    finally:
        ctx.enable_timing(was)
    assert list(times) == ["egress_strided"] and times["egress_strided"] > 0, times


# ------------------------------------------------------------------ one-off cases
def _run(ctx, rows, up, down, taps, step, lanes, out_bytes):
    """rows over `lanes` [n_lanes][n_samples] through the device form -> the bytes (canaries first)"""
    d_l, d_o = ctx.device_alloc(lanes.nbytes), ctx.device_alloc(out_bytes)
    try:
        ctx.to_device(d_l, lanes)
        ctx.to_device(d_o, er.canaries(out_bytes))
        ctx.egress_resample_strided(rows, up, down, taps, step, d_lanes=d_l, n_lanes=lanes.shape[0], lane_stride=lanes.shape[1], n_samples=lanes.shape[1],
                                    out=d_o, out_bytes=out_bytes)
        return ctx.to_host(np.zeros(out_bytes, np.uint8), d_o)
    finally:
        ctx.device_free(d_l)
        ctx.device_free(d_o)


def test_a_row_far_into_a_long_stream(gpu_ctx):
    # stream_frames = 2^36 strided samples, 300 outputs from 2^33 + 5, step 3: out_from * down is past 2^40 and (lo - frame_base)
    # * step is the only product with the step.  The lanes hold only the window's span, the last strided sample the lane's last.
    up, down, step = 147, 160, 3
    taps = rc.case_taps(up, down, 16, "design")
    sf, a, n = 1 << 36, (1 << 33) + 5, 300
    assert a * down > 1 << 40 and sf * up < 1 << 62
    lo, hi = rc.window(up, down, taps.size, sf, a, n)
    x = er.lane_data(np.random.default_rng(9), hi - lo, 2)
    span = (hi - lo - 1) * step + 1
    lanes = np.full((3, 3 + span), np.nan, np.float32)
    lanes[1:3, 3:3 + span:step] = x.T
    rows = [(45, n, 2, er.F32, 1, 3, lo, hi - lo, sf, a), (45 + n * 8, n, 2, er.PCM16, 1, 3, lo, hi - lo, sf, a)]
    out = _run(gpu_ctx, rows, up, down, taps, step, lanes, 45 + n * 12 + 3)
    y, B = rc.resample_model(x.astype(np.float64), taps, up, down, a, n, frame_base=lo, file_frames=sf)
    got = er.row_f32(out, rows[0])
    assert not np.isnan(got).any()
    rc.compare(got, y, B, up, taps.size, "outputs from 2^33 + 5")
    want = np.concatenate([er.canaries(45), out[45:45 + n * 8], ec.encode(np.ascontiguousarray(got.T).reshape(-1).view(np.uint32), er.PCM16, False).reshape(-1),
                           er.canaries(3)])
    ec.compare(out, want, "the PCM16 row and the canaries")


def test_identity_at_step_3_gives_fvad_egress_bytes_of_every_third_sample(gpu_ctx):
    # a 16 kHz recording of the network's samples: 1/1 with the tap 1.0 at step 3, phase 2, over random lanes equals fvad_egress
    # over lanes[:, 2::3], but for the -0.0 sample
    ctx = gpu_ctx
    rng = np.random.default_rng(4)
    n = 9001
    lanes = rng.uniform(-1.2, 1.2, (3, 3 * n)).astype(np.float32)
    lanes[1, 2 + 3 * 100] = -0.0
    third = np.ascontiguousarray(lanes[:, 2::3])
    rows, sinks, at = [], [], 44
    for fmt in (er.F32, er.PCM16, er.PCM24):
        sinks.append((at, n, 2, fmt, 1, 0))
        rows.append((at, n, 2, fmt, 1, 2, 0, n, n, 0))
        at += n * 2 * er.SAMPLE_BYTES[fmt] + 1
    got = _run(ctx, rows, 1, 1, [1.0], 3, lanes, at + 2)
    d_l, d_o = ctx.device_alloc(third.nbytes), ctx.device_alloc(at + 2)
    try:
        ctx.to_device(d_l, third)
        ctx.to_device(d_o, er.canaries(at + 2))
        ctx.egress(sinks, d_lanes=d_l, n_lanes=3, lane_stride=n, n_samples=n, out=d_o, out_bytes=at + 2)
        want = ctx.to_host(np.zeros(at + 2, np.uint8), d_o)
    finally:
        ctx.device_free(d_l)
        ctx.device_free(d_o)
    k = 44 + (100 * 2 + 0) * 4   # the -0.0 sample of the f32 file: fvad_egress moves its bits, fma(1, -0, +0) is +0
    assert want[k:k + 4].tolist() == [0, 0, 0, 0x80] and got[k:k + 4].tolist() == [0, 0, 0, 0]
    want[k + 3] = 0
    ec.compare(got, want, "1/1 with the tap 1.0 at step 3 against fvad_egress over every third sample")
