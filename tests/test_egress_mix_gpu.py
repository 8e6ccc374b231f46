"""The two-source egress on the GPU (fvad_egress_mix_device, fvad_egress_mix): the case table of egress_mix_cases.py against the
numpy model for every weight pair, byte for byte (a NaN of an f32 file for any NaN), with canaries around everything the sinks
write and NaN around everything they may read; the host form through a ring so small that sinks are cut several times; the
invariances; an absent source; the refused calls; and the pass-through against fvad_egress."""
import ctypes as C

import numpy as np
import pytest

import egress_cases as ec
import egress_mix_cases as mc

pytestmark = pytest.mark.gpu

INVALID, RANGE = -100, -6
SMALL_RING = "6000"   # bytes: the table's largest sink (32 KB) crosses it in six pieces
IDS = [f"{a}x{b}" for a, b in mc.WEIGHTS]


class Device:
    """a case table's two lane sets on the device and an output buffer of canaries"""

    def __init__(self, fv, ctx, w):
        self.fv, self.ctx, self.w = fv, ctx, w
        t = mc.case_table(*w)
        self.t, self.sinks, self.out_bytes = t, t["sinks"], t["out_bytes"]
        self.out_in = ec.canaries(self.out_bytes)
        self.want = mc.mix_model(t["orig"], t["den"], self.sinks, w[0], w[1], self.out_in)   # computed once, shared, never changed
        self.d_orig, self.d_den = ctx.device_alloc(t["orig"].nbytes), ctx.device_alloc(t["den"].nbytes)
        ctx.to_device(self.d_orig, t["orig"])
        ctx.to_device(self.d_den, t["den"])
        self.d_out = ctx.device_alloc(self.out_bytes)

    def close(self):
        for d in (self.d_orig, self.d_den, self.d_out):
            self.ctx.device_free(d)

    def fill(self):
        self.ctx.to_device(self.d_out, self.out_in)

    def read(self):
        return self.ctx.to_host(np.zeros_like(self.out_in), self.d_out)

    def args(self, **kw):
        t = self.t
        a = dict(w_orig=self.w[0], w_den=self.w[1], d_orig=self.d_orig, orig_stride=t["orig_stride"], orig_samples=t["orig_samples"],
                 d_den=self.d_den, den_stride=t["den_stride"], den_samples=t["den_samples"], n_lanes=t["n_lanes"])
        a.update(kw)
        return a

    def device_form(self, sinks, **kw):
        self.ctx.egress_mix(sinks, out=self.d_out, out_bytes=self.out_bytes, **self.args(**kw))

    def host_form(self, sinks, out=None, **kw):
        """-> the host buffer, canaries before the call"""
        out = self.out_in.copy() if out is None else out
        self.ctx.egress_mix(sinks, out=[out] * len(sinks), **self.args(**kw))
        return out

    def status(self, sinks, host=False, host_buf=None, out="own", out_bytes=None, null_rows=False, src_format=0, **kw):
        """the C call itself -> status"""
        fv, a = self.fv, self.args(**kw)
        snk = np.ascontiguousarray(np.asarray(sinks, np.uint64).reshape(-1, 8))
        rows = None if null_rows else snk.ctypes.data_as(C.POINTER(C.c_uint64))
        head = (self.ctx.h, fv.vp(a["d_orig"]), a["orig_stride"], a["orig_samples"], fv.vp(a["d_den"]), a["den_stride"], a["den_samples"],
                src_format, a["n_lanes"], a["w_orig"], a["w_den"], rows, len(snk))
        if host:
            ptrs = (fv.vp * max(len(snk), 1))(*([host_buf.ctypes.data] * len(snk)))
            return fv.lib().fvad_egress_mix(*head, ptrs if out == "own" else out)
        return fv.lib().fvad_egress_mix_device(*head, fv.vp(self.d_out if out == "own" else out), self.out_bytes if out_bytes is None else out_bytes)

    def check(self, got, what):
        mc.compare(got, self.want, self.sinks, what)


_devices = {}


@pytest.fixture(scope="module")
def devices(fv, gpu_ctx):
    """one Device per weight pair, made when first asked for"""
    def get(w):
        if w not in _devices:
            _devices[w] = Device(fv, gpu_ctx, w)
        return _devices[w]
    yield get
    for d in _devices.values():
        d.close()
    _devices.clear()


@pytest.fixture(params=mc.WEIGHTS, ids=IDS)
def dev(request, devices):
    return devices(request.param)


def test_case_table_matches_the_model(dev):
    # every file format, channel count, length around the tile, byte alignment, pair of source alignments and count of leading
    # zeros of the table; whatever no sink writes is still the canary, and no NaN from outside a sink's ranges came in
    dev.fill()
    dev.device_form(dev.sinks)
    dev.check(dev.read(), "fvad_egress_mix_device")


@pytest.mark.parametrize("ring", [SMALL_RING, None], ids=["small-ring", "default-ring"])
def test_host_form_equals_device_form_however_the_ring_cuts(dev, ring):
    with dev.ctx.options(ingest_ring_bytes=ring):
        dev.check(dev.host_form(dev.sinks), f"fvad_egress_mix, ring {ring}")


def test_order_batching_cuts_and_reruns_change_nothing(dev):
    dev.fill()
    dev.device_form(dev.sinks[::-1])
    dev.check(dev.read(), "the sinks reversed")
    dev.device_form(dev.sinks)                        # a second run over the bytes the first one wrote
    dev.check(dev.read(), "a second run")
    dev.fill()
    for row in dev.sinks:
        dev.device_form(row[None])
    dev.check(dev.read(), "one sink per call")
    out = dev.out_in.copy()
    with dev.ctx.options(ingest_ring_bytes=SMALL_RING):
        for row in dev.sinks[::-1]:
            dev.host_form(row[None], out)
    dev.check(out, "one sink per host call, reversed")
    # a file cut into sinks (time slices) by hand, at frames that are no multiple of anything and around the last leading zero:
    # the piece from frame a on has a zeros fewer (at most all of them) and starts the rest of a further into the original
    snk = dev.sinks.astype(object)
    k = max((i for i, r in enumerate(snk) if 0 < r[7] < r[1]), key=lambda i: snk[i][1])
    o, n, Cn, fmt, l0, s0, oo, z = (int(x) for x in snk[k])
    assert 1 < z < n - 2 and n > ec.tile_frames(Cn, fmt)
    fb = Cn * ec.SAMPLE_BYTES[fmt]
    cuts = sorted({0, 1, 7, z - 1, z, z + 1, n // 3, n // 3 + 1, n - 2, n})
    pieces = [(o + a * fb, b - a, Cn, fmt, l0, s0 + a, oo + a - min(z, a), z - min(z, a)) for a, b in zip(cuts, cuts[1:])]
    dev.fill()
    dev.device_form(np.concatenate([np.asarray(pieces[::-1], np.uint64), np.delete(dev.sinks, k, axis=0)]))
    dev.check(dev.read(), "a sink cut into pieces")


@pytest.mark.parametrize("w", [w for w in mc.WEIGHTS if 0.0 in w], ids=lambda w: f"{w[0]}x{w[1]}")
def test_a_source_whose_weight_is_zero_may_be_absent(devices, w):
    dev = devices(w)
    gone = dict(d_orig=None, orig_stride=0, orig_samples=0) if w[0] == 0 else dict(d_den=None, den_stride=0, den_samples=0)
    dev.fill()
    dev.device_form(dev.sinks, **gone)
    dev.check(dev.read(), "the device form without the unread lanes")
    with dev.ctx.options(ingest_ring_bytes=SMALL_RING):
        dev.check(dev.host_form(dev.sinks, **gone), "the host form without the unread lanes")
    # nor does a pointer that is not read need an alignment
    odd = dict(d_orig=dev.d_orig + 1) if w[0] == 0 else dict(d_den=dev.d_den + 3)
    dev.fill()
    assert dev.status(dev.sinks, **odd) == 0
    dev.check(dev.read(), "the device form with a misaligned pointer to the unread lanes")
    # the source that IS read may not be absent
    good = dev.sinks[dev.sinks[:, 1] > 0][0]
    need = dict(d_den=None) if w[0] == 0 else dict(d_orig=None)
    assert dev.status(good, **need) == INVALID and dev.status(good, host=True, host_buf=dev.out_in.copy(), **need) == INVALID


def test_refused_calls_leave_the_canaries_alone(dev):
    dev.fill()
    host_buf = dev.out_in.copy()
    good = dev.sinks[(dev.sinks[:, 1] > 0) & (dev.sinks[:, 7] < dev.sinks[:, 1])][0].copy()
    t, w = dev.t, dev.w

    def edit(col, value):
        r = good.copy()
        r[col] = value
        return r

    for host in (False, True):
        kw = dict(host=host, host_buf=host_buf)
        assert dev.status(good, out=None, **kw) == INVALID
        assert dev.status(good, null_rows=True, **kw) == INVALID
        assert dev.status(good, src_format=1, **kw) == INVALID and dev.status(good, src_format=2, **kw) == INVALID   # PCM16 lanes are refused
        assert dev.status(good, w_orig=0.0, w_den=0.0, **kw) == INVALID
        assert dev.status(good, w_orig=float("nan"), **kw) == INVALID and dev.status(good, w_den=float("inf"), **kw) == INVALID
        assert dev.status(edit(3, 3), **kw) == INVALID
        assert dev.status(edit(2, 0), **kw) == INVALID and dev.status(edit(2, 65), **kw) == INVALID
        assert dev.status(np.stack([good, good]), **kw) == INVALID                               # overlapping bytes
        assert dev.status(edit(4, t["n_lanes"]), **kw) == RANGE
        assert dev.status(edit(0, (1 << 64) - 1), **kw) == RANGE                                 # byte_offset + bytes wraps (the host form: the address)
        if w[0] != 0:
            assert dev.status(good, d_orig=None, **kw) == INVALID
            assert dev.status(good, d_orig=dev.d_orig + 2, **kw) == INVALID                      # lanes not aligned to their samples
            assert dev.status(good, orig_stride=t["orig_samples"] - 1, **kw) == INVALID
            assert dev.status(good, orig_samples=int(good[6]) + int(good[1]) - int(good[7]) - 1, **kw) == RANGE
        if w[1] != 0:
            assert dev.status(good, d_den=None, **kw) == INVALID
            assert dev.status(good, d_den=dev.d_den + 1, **kw) == INVALID
            assert dev.status(good, den_stride=t["den_samples"] - 1, **kw) == INVALID
            assert dev.status(good, den_samples=int(good[5]) + int(good[1]) - 1, **kw) == RANGE
    assert dev.status(good, out_bytes=int(good[0]) + int(good[1]) * int(good[2]) * ec.SAMPLE_BYTES[int(good[3])] - 1) == RANGE
    # a NULL buffer for a sink with frames; two host buffers that are one: the overlap is of absolute addresses
    fv = dev.fv
    rows = np.ascontiguousarray(np.stack([good, edit(0, int(good[0]) + 1)]))
    a = dev.args()
    head = (dev.ctx.h, fv.vp(a["d_orig"]), a["orig_stride"], a["orig_samples"], fv.vp(a["d_den"]), a["den_stride"], a["den_samples"], 0,
            a["n_lanes"], a["w_orig"], a["w_den"], rows.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert fv.lib().fvad_egress_mix(*head, 1, (fv.vp * 1)(None)) == INVALID
    assert fv.lib().fvad_egress_mix(*head, 2, (fv.vp * 2)(host_buf.ctypes.data, host_buf.ctypes.data)) == INVALID
    assert fv.lib().fvad_egress_mix(*head, 2, (fv.vp * 2)(host_buf.ctypes.data + 1, host_buf.ctypes.data)) == INVALID   # the same bytes through two bases
    empty = np.zeros((0, 8), np.uint64)
    assert dev.status(empty) == 0 and dev.status(empty, host=True, host_buf=host_buf) == 0   # nothing to do
    ec.compare(dev.read(), dev.out_in, "the device canaries after the refused calls")
    ec.compare(host_buf, dev.out_in, "the host canaries after the refused calls")
    with pytest.raises(fv.FvadError):   # the binding's own bounds check of a host buffer
        dev.ctx.egress_mix(good[None], out=[host_buf[:int(good[0])]], **dev.args())
    with pytest.raises(ValueError):
        ro = host_buf.copy()
        ro.flags.writeable = False
        dev.ctx.egress_mix(good[None], out=[ro], **dev.args())


def test_a_sink_without_frames_touches_nothing(dev):
    dev.fill()
    row = np.array([[dev.out_bytes, 0, 2, ec.PCM16, 1, 3, 5, 7]], np.uint64)
    dev.device_form(row)
    ec.compare(dev.read(), dev.out_in, "a sink without frames, device form")
    row[0, 0] = dev.out_bytes + 12345   # the host form: no buffer at all, whatever byte_offset says
    dev.ctx.egress_mix(row, out=[None], **dev.args())
    ec.compare(dev.read(), dev.out_in, "a sink without frames, host form")
    real = dev.sinks[dev.sinks[:, 1] > 0][:1]
    out = dev.out_in.copy()
    dev.ctx.egress_mix(np.concatenate([row, real]), out=[None, out], **dev.args())
    mc.compare(out, mc.mix_model(dev.t["orig"], dev.t["den"], real, dev.w[0], dev.w[1], dev.out_in), real, "an empty sink beside a real one")


def test_pass_through_writes_fvad_egress_bytes(devices):
    # w = (0, 1): the denoised lanes as fvad_egress writes them, byte for byte (the payload of a NaN apart, which only this
    # kernel's multiplication by 1 may touch)
    dev = devices((0.0, 1.0))
    t = dev.t
    d_plain = dev.ctx.device_alloc(dev.out_bytes)
    try:
        dev.ctx.to_device(d_plain, dev.out_in)
        dev.ctx.egress(mc.as_egress_rows(dev.sinks), d_lanes=dev.d_den, n_lanes=t["n_lanes"], lane_stride=t["den_stride"], n_samples=t["den_samples"],
                       out=d_plain, out_bytes=dev.out_bytes)
        plain = dev.ctx.to_host(np.zeros_like(dev.out_in), d_plain)
    finally:
        dev.ctx.device_free(d_plain)
    dev.fill()
    dev.device_form(dev.sinks)
    got = dev.read()
    mc.compare(got, plain, dev.sinks, "fvad_egress_mix(0, 1) against fvad_egress")
    # and without any NaN in the way: a sink whose lanes hold none
    clean = [r for r in dev.sinks if int(r[1]) > 0 and not np.isnan(t["den"][int(r[4]):int(r[4]) + int(r[2]), int(r[5]):int(r[5]) + int(r[1])]).any()]
    assert clean
    for r in clean:
        o, nb = int(r[0]), int(r[1]) * int(r[2]) * ec.SAMPLE_BYTES[int(r[3])]
        ec.compare(got[o:o + nb], plain[o:o + nb], "a sink without NaN, strictly")


def test_kernel_times_name_egress_mix(dev):
    ctx = dev.ctx
    was = ctx.timing
    ctx.enable_timing(True)
    try:
        ctx.kernel_times()
        dev.device_form(dev.sinks)
        times = ctx.kernel_times()
    finally:
        ctx.enable_timing(was)
    assert list(times) == ["egress_mix"] and times["egress_mix"] > 0, times
