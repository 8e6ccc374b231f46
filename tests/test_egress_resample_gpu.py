"""The resampling egress on the GPU (fvad_egress_resample_device, fvad_egress_resample): the case tables of
egress_resample_cases.py -- as f32 files against the float64 model within its computed bound, as PCM16 / PCM24 files byte for
byte against the conversion of the f32 values the library itself wrote --, with NaN around everything the rows may read and
canaries around everything they write; the host form through a ring so small that rows are cut several times; streams cut into
rows; a row eleven hours into a stream; the invariances; the refused calls; the identity ratio against fvad_egress; and the round
trip of a 44.1 kHz file through the resampling ingest and back."""
import ctypes as C

import numpy as np
import pytest

import egress_cases as ec
import egress_resample_cases as er
import ingest_resample_cases as rc

pytestmark = pytest.mark.gpu

INVALID, RANGE = -100, -6
SMALL_RING = "6000"   # bytes: the tables' largest rows (about 38 KB) cross it in seven pieces


class Device:
    """a ratio's case table with its lanes on the device; the model, the all-f32 run and the expected bytes computed once"""

    def __init__(self, fv, ctx, ratio):
        self.fv, self.ctx = fv, ctx
        self.up, self.down, half, kind = ratio
        self.taps = rc.case_taps(self.up, self.down, half, kind)
        self.t = er.case_table(self.up, self.down, self.taps.size)
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

    def geom(self):
        return dict(d_lanes=self.d_lanes, n_lanes=self.t["n_lanes"], lane_stride=self.t["lane_stride"], n_samples=self.t["n_samples"])

    def run32(self):
        """the all-f32 table through the device form -> its bytes"""
        n = self.t32["out_bytes"]
        self.ctx.to_device(self.d_out, er.canaries(n))
        self.ctx.egress_resample(self.t32["rows"], self.up, self.down, self.taps, out=self.d_out, out_bytes=n, **self.geom())
        return self.ctx.to_host(np.zeros(n, np.uint8), self.d_out)

    def expected(self):
        """the table's bytes: the conversion of what the library wrote as f32 files (held against the model before it is used)"""
        if self.want is None:
            self.out32 = self.run32()
            er.compare_f32(self.out32, self.t32, self.model, self.up, self.taps.size, "fvad_egress_resample_device, f32 files")
            self.want = er.bytes_from_f32(self.t, self.t32, self.out32)
        return self.want

    def fill(self):
        self.ctx.to_device(self.d_out, self.out_in)

    def read(self):
        return self.ctx.to_host(np.zeros_like(self.out_in), self.d_out)

    def device_form(self, rows):
        self.ctx.egress_resample(rows, self.up, self.down, self.taps, out=self.d_out, out_bytes=self.out_bytes, **self.geom())

    def host_form(self, rows, out=None):
        out = self.out_in.copy() if out is None else out
        self.ctx.egress_resample(rows, self.up, self.down, self.taps, out=[out] * len(rows), **self.geom())
        return out

    def status(self, rows, host=False, out="own", out_bytes=None, src_format=0, d_lanes="own", up=None, taps="own", n_samples=None, stride=None, host_buf=None):
        """the C call itself -> status"""
        fv = self.fv
        snk = np.ascontiguousarray(np.asarray(self.rows[:1] if rows is None else rows, np.uint64).reshape(-1, 10))
        ptr = snk.ctypes.data_as(C.POINTER(C.c_uint64)) if rows is not None else None   # (None: a NULL table of one row)
        tp = fv.fptr(self.taps) if isinstance(taps, str) else taps
        head = (self.ctx.h, fv.vp(self.d_lanes if isinstance(d_lanes, str) else d_lanes), src_format, self.t["n_lanes"],
                self.t["lane_stride"] if stride is None else stride, self.t["n_samples"] if n_samples is None else n_samples, ptr, len(snk),
                self.up if up is None else up, self.down, tp, self.taps.size)
        if host:
            ptrs = (fv.vp * max(len(snk), 1))(*([host_buf.ctypes.data] * len(snk)))
            return fv.lib().fvad_egress_resample(*head, ptrs if isinstance(out, str) else out)
        return fv.lib().fvad_egress_resample_device(*head, fv.vp(self.d_out if isinstance(out, str) else out), self.out_bytes if out_bytes is None else out_bytes)


@pytest.fixture(scope="module", params=er.RATIOS, ids=er.ratio_id)
def dev(request, fv, gpu_ctx):
    d = Device(fv, gpu_ctx, request.param)
    yield d
    d.close()


def test_case_table_matches_the_model(dev):
    # every row as an f32 file: within gamma(up, n_taps) * B + one ulp of the float64 model, no NaN (nothing outside the given
    # frames was read), every byte between the rows still the canary.  Then the table itself -- PCM16, PCM24 and f32 files, odd
    # byte offsets, rows that touch: byte for byte the conversion of those f32 values.
    want = dev.expected()
    dev.fill()
    dev.device_form(dev.rows)
    ec.compare(dev.read(), want, "fvad_egress_resample_device")


@pytest.mark.parametrize("ring", [SMALL_RING, None], ids=["small-ring", "default-ring"])
def test_host_form_equals_device_form_however_the_ring_cuts(dev, ring):
    want = dev.expected()
    with dev.ctx.options(ingest_ring_bytes=ring):
        ec.compare(dev.host_form(dev.rows), want, f"fvad_egress_resample, ring {ring}")


def test_streams_cut_into_rows_give_the_one_row_bytes(dev):
    # every big stream again, cut at outputs that are no multiple of 4; each piece is given exactly its fvad_resample_window, at
    # a src_offset of its own in a fresh lane buffer that is NaN everywhere else
    want = dev.expected()
    ctx, fv = dev.ctx, dev.fv
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
            cur = src + (hi - lo)
        n_samples = cur + 1
        lanes = np.full((Cn + 2, n_samples + 2), np.nan, np.float32)
        for (p, lo, hi), q in zip(pieces, placed):
            lanes[1:1 + Cn, q[5]:q[5] + hi - lo] = x[lo:hi].T
        d_l, d_o = ctx.device_alloc(lanes.nbytes), ctx.device_alloc(nb + 8)
        try:
            ctx.to_device(d_l, lanes)
            ctx.to_device(d_o, er.canaries(nb + 8))
            ctx.egress_resample(placed[::-1], dev.up, dev.down, dev.taps, d_lanes=d_l, n_lanes=Cn + 2, lane_stride=n_samples + 2, n_samples=n_samples,
                                out=d_o, out_bytes=nb + 8)
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
        assert dev.status(good, taps=None, **kw) == INVALID
        assert dev.status(edit(3, 3), **kw) == INVALID
        assert dev.status(edit(2, 0), **kw) == INVALID and dev.status(edit(2, 65), **kw) == INVALID
        assert dev.status(edit(9, 1), **kw) == INVALID                                          # one output past the stream's last
        assert dev.status(edit(7, int(good[7]) - 1), **kw) == INVALID                           # the window's last frame is not given
        assert dev.status(np.stack([good, good]), **kw) == INVALID                              # overlapping bytes
        assert dev.status(good, d_lanes=dev.d_lanes + 2, **kw) == INVALID                       # lanes not aligned to their samples
        assert dev.status(good, stride=dev.t["n_samples"] - 1, **kw) == INVALID
        assert dev.status(edit(4, dev.t["n_lanes"]), **kw) == RANGE
        assert dev.status(good, n_samples=int(good[5]) + int(good[7]) - 1, **kw) == RANGE
        assert dev.status(edit(0, (1 << 64) - 1), **kw) == RANGE                                # byte_offset + bytes wraps (the host form: the address)
    assert dev.status(good, out_bytes=int(good[0]) + int(good[1]) * int(good[2]) * er.SAMPLE_BYTES[int(good[3])] - 1) == RANGE
    fv = dev.fv
    rows = np.ascontiguousarray(np.stack([good, edit(0, int(good[0]) + 1)]))
    head = (dev.ctx.h, fv.vp(dev.d_lanes), 0, dev.t["n_lanes"], dev.t["lane_stride"], dev.t["n_samples"], rows.ctypes.data_as(C.POINTER(C.c_uint64)))
    tail = (dev.up, dev.down, fv.fptr(dev.taps), dev.taps.size)
    assert fv.lib().fvad_egress_resample(*head, 1, *tail, (fv.vp * 1)(None)) == INVALID       # a row with outputs and no bytes
    assert fv.lib().fvad_egress_resample(*head, 2, *tail, (fv.vp * 2)(host_buf.ctypes.data + 1, host_buf.ctypes.data)) == INVALID   # the same bytes through two bases
    empty = np.zeros((0, 10), np.uint64)
    assert dev.status(empty) == 0 and dev.status(empty, host=True, host_buf=host_buf) == 0    # nothing to do
    ec.compare(dev.read(), dev.out_in, "the device canaries after the refused calls")
    ec.compare(host_buf, dev.out_in, "the host canaries after the refused calls")
    with pytest.raises(fv.FvadError):   # the binding's own bounds check of a host buffer
        dev.ctx.egress_resample(good[None], dev.up, dev.down, dev.taps, out=[host_buf[:int(good[0])]], **dev.geom())


def test_a_row_without_outputs_touches_nothing(dev):
    dev.fill()
    row = np.array([[dev.out_bytes, 0, 2, er.PCM16, 1, 3, 0, 0, 100, 0]], np.uint64)
    dev.device_form(row)
    ec.compare(dev.read(), dev.out_in, "a row without outputs, device form")
    row[0, 0] = dev.out_bytes + 12345   # the host form: no buffer at all, whatever byte_offset says
    dev.ctx.egress_resample(row, dev.up, dev.down, dev.taps, out=[None], **dev.geom())
    ec.compare(dev.read(), dev.out_in, "a row without outputs, host form")


def test_kernel_times_name_egress_resample(dev):
    ctx = dev.ctx
    was = ctx.timing
    ctx.enable_timing(True)
    try:
        ctx.kernel_times()
        dev.device_form(dev.rows)
        times = ctx.kernel_times()
    finally:
        ctx.enable_timing(was)
    assert list(times) == ["egress_resample"] and times["egress_resample"] > 0, times


# ------------------------------------------------------------------ one-off cases
def _run(ctx, rows, up, down, taps, lanes, out_bytes):
    """rows over `lanes` [n_lanes][n_samples] through the device form -> the bytes (canaries first)"""
    d_l, d_o = ctx.device_alloc(lanes.nbytes), ctx.device_alloc(out_bytes)
    try:
        ctx.to_device(d_l, lanes)
        ctx.to_device(d_o, er.canaries(out_bytes))
        ctx.egress_resample(rows, up, down, taps, d_lanes=d_l, n_lanes=lanes.shape[0], lane_stride=lanes.shape[1], n_samples=lanes.shape[1],
                            out=d_o, out_bytes=out_bytes)
        return ctx.to_host(np.zeros(out_bytes, np.uint8), d_o)
    finally:
        ctx.device_free(d_l)
        ctx.device_free(d_o)


def test_a_row_far_into_a_long_stream(gpu_ctx):
    # stream_frames = 2^36 (16 days), 300 outputs from 2^33 + 5: out_from * down is past 2^40, every 32-bit product would have
    # wrapped many times.  The lanes hold only the window.
    up, down = 147, 160
    taps = rc.case_taps(up, down, 16, "design")
    sf, a, n = 1 << 36, (1 << 33) + 5, 300
    assert a * down > 1 << 40 and sf * up < 1 << 62
    lo, hi = rc.window(up, down, taps.size, sf, a, n)
    x = er.lane_data(np.random.default_rng(9), hi - lo, 2)
    lanes = np.full((3, hi - lo + 7), np.nan, np.float32)
    lanes[1:3, 3:3 + hi - lo] = x.T
    rows = [(45, n, 2, er.F32, 1, 3, lo, hi - lo, sf, a), (45 + n * 8, n, 2, er.PCM16, 1, 3, lo, hi - lo, sf, a)]
    out = _run(gpu_ctx, rows, up, down, taps, lanes, 45 + n * 12 + 3)
    y, B = rc.resample_model(x.astype(np.float64), taps, up, down, a, n, frame_base=lo, file_frames=sf)
    got = er.row_f32(out, rows[0])
    assert not np.isnan(got).any()
    rc.compare(got, y, B, up, taps.size, "outputs from 2^33 + 5")
    want = np.concatenate([er.canaries(45), out[45:45 + n * 8], ec.encode(np.ascontiguousarray(got.T).reshape(-1).view(np.uint32), er.PCM16, False).reshape(-1),
                           er.canaries(3)])
    ec.compare(out, want, "the PCM16 row and the canaries")


def test_identity_ratio_and_tap_give_fvad_egress_bytes(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(4)
    n = 9001
    lanes = rng.uniform(-1.2, 1.2, (3, n + 6)).astype(np.float32)
    lanes[1, 100] = -0.0
    plain = [(44, n, 2, fmt, 1, 5) for fmt in (er.F32, er.PCM16, er.PCM24)]
    rows, sinks, at = [], [], 44
    for _, _, Cn, fmt, l0, src in plain:
        sinks.append((at, n, Cn, fmt, l0, src))
        rows.append((at, n, Cn, fmt, l0, src, 0, n, n, 0))
        at += n * Cn * er.SAMPLE_BYTES[fmt] + 1
    got = _run(ctx, rows, 1, 1, [1.0], lanes, at + 2)
    d_l, d_o = ctx.device_alloc(lanes.nbytes), ctx.device_alloc(at + 2)
    try:
        ctx.to_device(d_l, lanes)
        ctx.to_device(d_o, er.canaries(at + 2))
        ctx.egress(sinks, d_lanes=d_l, n_lanes=3, lane_stride=n + 6, n_samples=n + 6, out=d_o, out_bytes=at + 2)
        want = ctx.to_host(np.zeros(at + 2, np.uint8), d_o)
    finally:
        ctx.device_free(d_l)
        ctx.device_free(d_o)
    k = 44 + ((100 - 5) * 2 + 0) * 4   # the -0.0 sample of the f32 file: fvad_egress moves its bits, fma(1, -0, +0) is +0
    assert want[k:k + 4].tolist() == [0, 0, 0, 0x80] and got[k:k + 4].tolist() == [0, 0, 0, 0]
    want[k + 3] = 0
    ec.compare(got, want, "1/1 with the tap 1.0 against fvad_egress")


def test_ingest_resample_then_egress_resample_returns_the_file(fv, gpu_ctx):
    # A 44.1 kHz PCM16 file of 147 * 60 frames (a multiple of 147, so that ceil(ceil(N 160 / 147) 147 / 160) is N) holding a
    # 1 kHz tone of amplitude 0.5: up to 48 kHz with the default 160/147 design, down again with the default 147/160 design.
    # Both filters are centred, so there is no delay to correct.  The tolerance, derived from tools/resample_response.py's
    # figures (include/fvad.h): each design's pass-band ripple is at most 0.11 dB, so the tone's gain lies within
    # 10^(+-0.22 / 20) of 1; each design's stop band is -69.8 dB or better, which bounds what an image adds; and the file's
    # samples are rounded to PCM16 once on the way out (the input is exact).
    ctx = gpu_ctx
    A, N = 0.5, 147 * 60
    tol = A * (10 ** (0.22 / 20) - 1) + 2 * A * 10 ** (-69.8 / 20) + 0.5 / 32768
    s = np.rint(A * 32768 * np.sin(2 * np.pi * 1000 * np.arange(N) / 44100)).astype("<i2")
    raw = s.view(np.uint8)
    up_in = fv.resample_ratio(44100)
    up_out = fv.resample_ratio(48000, 44100)
    assert up_in == (160, 147) and up_out == (147, 160)
    M = fv.resample_out_frames(N, *up_in)
    assert M == 160 * 60 and fv.resample_out_frames(M, *up_out) == N
    d_l, d_o = ctx.device_alloc((M + 4) * 4), ctx.device_alloc(N * 2)
    try:
        ctx.ingest_resample([(0, N, 1, er.PCM16, 0, 1, M + 1, 0, N, 0, M)], *up_in, fv.resample_design(*up_in), d_lanes=d_l, n_lanes=1,
                            lane_stride=M + 4, n_samples=M + 4, raw=[raw])
        ctx.egress_resample([(0, N, 1, er.PCM16, 0, 1, 0, M, M, 0)], *up_out, fv.resample_design(*up_out), d_lanes=d_l, n_lanes=1,
                            lane_stride=M + 4, n_samples=M + 4, out=d_o, out_bytes=N * 2)
        back = ctx.to_host(np.zeros(N * 2, np.uint8), d_o).view("<i2")
    finally:
        ctx.device_free(d_l)
        ctx.device_free(d_o)
    assert back.size == N
    edge = 64   # 16 periods of the wider filter and more
    err = np.abs(back[edge:-edge].astype(np.float64) - s[edge:-edge]) / 32768
    print("round trip: max error", err.max(), "tolerance", tol)
    assert err.max() <= tol, (err.max(), tol)
