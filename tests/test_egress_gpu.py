"""The device-side egress on the GPU (fvad_egress_device, fvad_egress): the case table of egress_cases.py against the numpy model
in all four format pairs, byte for byte, with canaries around everything the sinks write; the host form through a ring so small
that sinks are cut several times; the invariances; the refused calls; and the round trip through the ingest -- a file's bytes
into lanes and out again are the file's bytes."""
import ctypes as C

import numpy as np
import pytest

import egress_cases as ec
import ingest_cases as ic

pytestmark = pytest.mark.gpu

INVALID, RANGE = -100, -6
SMALL_RING = "6000"   # bytes: the table's largest sink (32 KB) crosses it in six pieces


class Device:
    """a case table's lanes on the device and an output buffer of canaries"""

    def __init__(self, fv, ctx, src_pcm16):
        self.fv, self.ctx, self.src_pcm16 = fv, ctx, src_pcm16
        t = ec.case_table(src_pcm16)
        self.lanes, self.sinks, self.out_bytes = t["lanes"], t["sinks"], t["out_bytes"]
        self.n_lanes, self.stride, self.n_samples = t["n_lanes"], t["lane_stride"], t["n_samples"]
        self.out_in = ec.canaries(self.out_bytes)
        self.want = ec.egress_model(self.lanes, self.sinks, src_pcm16, self.out_in)   # computed once, shared, never changed
        self.d_lanes = ctx.device_alloc(self.lanes.nbytes)
        ctx.to_device(self.d_lanes, self.lanes)
        self.d_out = ctx.device_alloc(self.out_bytes)

    def close(self):
        self.ctx.device_free(self.d_lanes)
        self.ctx.device_free(self.d_out)

    def fill(self):
        self.ctx.to_device(self.d_out, self.out_in)

    def read(self):
        return self.ctx.to_host(np.zeros_like(self.out_in), self.d_out)

    def args(self):
        return dict(src_pcm16=self.src_pcm16, d_lanes=self.d_lanes, n_lanes=self.n_lanes, lane_stride=self.stride, n_samples=self.n_samples)

    def device_form(self, sinks):
        self.ctx.egress(sinks, out=self.d_out, out_bytes=self.out_bytes, **self.args())

    def host_form(self, sinks, out=None):
        """-> the host buffer, canaries before the call"""
        out = self.out_in.copy() if out is None else out
        self.ctx.egress(sinks, out=[out] * len(sinks), **self.args())
        return out

    def status(self, sinks, host=False, out="own", out_bytes=None, src_format=None, d_lanes="own", n_lanes=None, n_samples=None, stride=None, host_buf=None):
        """the C call itself -> status"""
        fv = self.fv
        snk = np.ascontiguousarray(np.asarray([(0, 1, 1, ec.PCM16, 1, 0)] if sinks is None else sinks, np.uint64).reshape(-1, 6))
        rows = snk.ctypes.data_as(C.POINTER(C.c_uint64)) if sinks is not None else None   # (None: a NULL table of one row)
        head = (self.ctx.h, fv.vp(self.d_lanes if d_lanes == "own" else d_lanes), int(self.src_pcm16) if src_format is None else src_format,
                self.n_lanes if n_lanes is None else n_lanes, self.stride if stride is None else stride,
                self.n_samples if n_samples is None else n_samples, rows, len(snk))
        if host:
            ptrs = (fv.vp * max(len(snk), 1))(*([host_buf.ctypes.data] * len(snk)))
            return fv.lib().fvad_egress(*head, ptrs if out == "own" else out)
        return fv.lib().fvad_egress_device(*head, fv.vp(self.d_out if out == "own" else out), self.out_bytes if out_bytes is None else out_bytes)


@pytest.fixture(scope="module", params=[False, True], ids=["from-f32", "from-pcm16"])
def dev(request, fv, gpu_ctx):
    d = Device(fv, gpu_ctx, request.param)
    yield d
    d.close()


def test_case_table_matches_the_model(dev):
    # f32 lanes to PCM16 / PCM24 / f32 files, PCM16 lanes to PCM16 files: every length around the tile, channel count, byte and
    # source alignment of the table; whatever no sink writes is still the canary (the model starts from them)
    dev.fill()
    dev.device_form(dev.sinks)
    ec.compare(dev.read(), dev.want, "fvad_egress_device")


@pytest.mark.parametrize("ring", [SMALL_RING, None], ids=["small-ring", "default-ring"])
def test_host_form_equals_device_form_however_the_ring_cuts(dev, ring):
    with dev.ctx.options(ingest_ring_bytes=ring):
        ec.compare(dev.host_form(dev.sinks), dev.want, f"fvad_egress, ring {ring}")


def test_order_batching_and_reruns_change_nothing(dev):
    dev.fill()
    dev.device_form(dev.sinks[::-1])
    ec.compare(dev.read(), dev.want, "the sinks reversed")
    dev.device_form(dev.sinks)                        # a second run over the bytes the first one wrote
    ec.compare(dev.read(), dev.want, "a second run")
    dev.fill()
    for row in dev.sinks:
        dev.device_form(row[None])
    ec.compare(dev.read(), dev.want, "one sink per call")
    out = dev.out_in.copy()
    with dev.ctx.options(ingest_ring_bytes=SMALL_RING):
        for row in dev.sinks[::-1]:
            dev.host_form(row[None], out)
    ec.compare(out, dev.want, "one sink per host call, reversed")
    # a file cut into sinks (time slices) at frames that are no multiple of anything
    k = dev.sinks[:, 1].argmax()
    o, n, Cn, fmt, l0, s0 = (int(x) for x in dev.sinks[k])
    fb = Cn * ec.SAMPLE_BYTES[fmt]
    cuts = [0, 1, 7, n // 3, n // 3 + 1, n - 2, n]
    pieces = [(o + a * fb, b - a, Cn, fmt, l0, s0 + a) for a, b in zip(cuts, cuts[1:])]
    dev.fill()
    dev.device_form(np.concatenate([np.asarray(pieces[::-1], np.uint64), np.delete(dev.sinks, k, axis=0)]))
    ec.compare(dev.read(), dev.want, "a sink cut into pieces")


def test_refused_calls_leave_the_canaries_alone(dev):
    dev.fill()
    host_buf = dev.out_in.copy()
    good = dev.sinks[dev.sinks[:, 1] > 0][0].copy()

    def edit(col, value):
        r = good.copy()
        r[col] = value
        return r

    other_format = ec.PCM24 if dev.src_pcm16 else 3   # PCM16 lanes -> PCM24 is a conversion; format 3 does not exist
    for host in (False, True):
        kw = dict(host=host, host_buf=host_buf)
        assert dev.status(good, d_lanes=None, **kw) == INVALID
        assert dev.status(good, out=None, **kw) == INVALID
        assert dev.status(None, **kw) == INVALID
        assert dev.status(good, src_format=2, **kw) == INVALID
        assert dev.status(edit(3, other_format), **kw) == INVALID
        assert dev.status(edit(2, 0), **kw) == INVALID and dev.status(edit(2, 65), **kw) == INVALID
        assert dev.status(np.stack([good, good]), **kw) == INVALID                               # overlapping bytes
        assert dev.status(good, d_lanes=dev.d_lanes + 1, **kw) == INVALID                        # lanes not aligned to their samples
        assert dev.status(good, stride=dev.n_samples - 1, **kw) == INVALID
        assert dev.status(edit(4, dev.n_lanes), **kw) == RANGE
        assert dev.status(good, n_samples=int(good[5]) + int(good[1]) - 1, stride=dev.stride, **kw) == RANGE
        assert dev.status(edit(0, (1 << 64) - 1), **kw) == RANGE                                 # byte_offset + bytes wraps (the host form: the address)
    assert dev.status(good, out_bytes=int(good[0]) + int(good[1]) * int(good[2]) * ec.SAMPLE_BYTES[int(good[3])] - 1) == RANGE
    if dev.src_pcm16:
        assert dev.status(edit(3, ec.F32)) == INVALID
    # a NULL buffer for a sink with frames; two host buffers that are one: the overlap is of absolute addresses
    fv = dev.fv
    rows = np.ascontiguousarray(np.stack([good, edit(0, int(good[0]) + 1)]))
    head = (dev.ctx.h, fv.vp(dev.d_lanes), int(dev.src_pcm16), dev.n_lanes, dev.stride, dev.n_samples, rows.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert fv.lib().fvad_egress(*head, 1, (fv.vp * 1)(None)) == INVALID
    assert fv.lib().fvad_egress(*head, 2, (fv.vp * 2)(host_buf.ctypes.data, host_buf.ctypes.data)) == INVALID
    assert fv.lib().fvad_egress(*head, 2, (fv.vp * 2)(host_buf.ctypes.data + 1, host_buf.ctypes.data)) == INVALID   # the same bytes through two bases
    empty = np.zeros((0, 6), np.uint64)
    assert dev.status(empty) == 0 and dev.status(empty, host=True, host_buf=host_buf) == 0   # nothing to do
    ec.compare(dev.read(), dev.out_in, "the device canaries after the refused calls")
    ec.compare(host_buf, dev.out_in, "the host canaries after the refused calls")
    with pytest.raises(fv.FvadError):   # the binding's own bounds check of a host buffer
        dev.ctx.egress(good[None], out=[host_buf[:int(good[0])]], **dev.args())
    with pytest.raises(ValueError):
        ro = host_buf.copy()
        ro.flags.writeable = False
        dev.ctx.egress(good[None], out=[ro], **dev.args())


def test_kernel_times_name_egress(dev):
    ctx = dev.ctx
    was = ctx.timing
    ctx.enable_timing(True)
    try:
        ctx.kernel_times()
        dev.device_form(dev.sinks)
        times = ctx.kernel_times()
    finally:
        ctx.enable_timing(was)
    assert list(times) == ["egress"] and times["egress"] > 0, times


def test_a_sink_without_frames_touches_nothing(dev):
    dev.fill()
    row = np.array([[dev.out_bytes, 0, 2, ec.PCM16, 1, 3]], np.uint64)
    dev.device_form(row)
    ec.compare(dev.read(), dev.out_in, "a sink without frames, device form")
    row[0, 0] = dev.out_bytes + 12345   # the host form: no buffer at all, whatever byte_offset says
    dev.ctx.egress(row, out=[None], **dev.args())
    ec.compare(dev.read(), dev.out_in, "a sink without frames, host form")
    real = dev.sinks[dev.sinks[:, 1] > 0][:1]
    out = dev.out_in.copy()
    dev.ctx.egress(np.concatenate([row, real]), out=[None, out], **dev.args())
    ec.compare(out, ec.egress_model(dev.lanes, real, dev.src_pcm16, dev.out_in), "an empty sink beside a real one")


# ------------------------------------------------------------------ the round trip through the ingest
@pytest.mark.parametrize("lanes_pcm16", [False, True], ids=["f32-lanes", "pcm16-lanes"])
def test_ingest_then_egress_gives_the_files_bytes_back(gpu_ctx, lanes_pcm16):
    # ingest_cases' raw bytes -- PCM16, PCM24 and f32 sources with their extremes, NaN payloads and -0 -- into lanes, and out
    # again through sinks of the same geometry: f32 lanes that hold s / 32768 (s / 8388608) give the PCM16 (PCM24) bytes, f32
    # sources their bits.  The raw buffer's padding is ic.PAD_BYTE, the output's canary too: the WHOLE buffer must come back.
    ctx = gpu_ctx
    assert ic.PAD_BYTE == ec.PAD_BYTE
    t = ic.case_table(lanes_pcm16)
    raw, src = t["raw"], t["sources"]
    lanes_in = ic.canaries(t["n_lanes"], t["lane_stride"], lanes_pcm16)
    geom = dict(d_lanes=ctx.device_alloc(lanes_in.nbytes), n_lanes=t["n_lanes"], lane_stride=t["lane_stride"], n_samples=t["n_samples"])
    d_out = ctx.device_alloc(raw.size)
    try:
        ctx.to_device(geom["d_lanes"], lanes_in)
        ctx.ingest(src, raw=[raw] * len(src), out_pcm16=lanes_pcm16, **geom)
        sinks = src[:, :6]   # byte_offset, n_frames, n_channels, format, first_lane, dst_offset -> src_offset
        ctx.to_device(d_out, ec.canaries(raw.size))
        ctx.egress(sinks, src_pcm16=lanes_pcm16, out=d_out, out_bytes=raw.size, **geom)
        ec.compare(ctx.to_host(np.zeros_like(raw), d_out), raw, "ingest, then egress (device form)")
        out = ec.canaries(raw.size)
        with ctx.options(ingest_ring_bytes=SMALL_RING):
            ctx.egress(sinks, src_pcm16=lanes_pcm16, out=[out] * len(sinks), **geom)
        ec.compare(out, raw, "ingest, then egress (host form, small ring)")
    finally:
        ctx.device_free(geom["d_lanes"])
        ctx.device_free(d_out)
