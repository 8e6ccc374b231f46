"""The resampling ingest on the GPU (fvad_ingest_resample_device, fvad_ingest_resample): per ratio and per set of taps the case
table of ingest_resample_cases.py against the float64 model within the computed fma-chain bound, with NaN canaries around
everything the sources write; then, bit for bit against that first result: the files cut into slices, the host form through a
1 KB ring and the default one, other orders and calls, and the f32 twins of the PCM files.  Last the index-width case, the
identity ratio against fvad_ingest, and the refused calls."""
import ctypes as C

import numpy as np
import pytest

import ingest_cases as ic
import ingest_resample_cases as rc

pytestmark = pytest.mark.gpu

INVALID, RANGE = -100, -6
PARAMS = [(up, down, half, kind) for up, down, half in rc.CASES for kind in ("design", "random")]


class Device:
    """a case table's raw bytes on the device, canary-filled lanes, the model (computed once, never changed)"""

    def __init__(self, fv, ctx, up, down, half, kind):
        self.fv, self.ctx, self.up, self.down = fv, ctx, up, down
        self.taps = fv.resample_design(up, down, half) if kind == "design" else rc.case_taps(up, down, half, kind)
        if kind == "design":
            assert np.array_equal(self.taps, rc.case_taps(up, down, half, kind))
        self.n_taps = self.taps.size
        self.table = t = rc.case_table(up, down, self.n_taps, lambda ch, fmt: fv.ingest_resample_tile(up, down, self.n_taps, ch, fmt))
        self.raw, self.rows = t["raw"], t["rows"]
        self.n_lanes, self.stride, self.n_samples = t["n_lanes"], t["lane_stride"], t["n_samples"]
        self.lanes_in = ic.canaries(self.n_lanes, self.stride, False)
        self.want, self.lanes_want = rc.model_lanes(t, self.taps, up, down, self.lanes_in)
        self.d_raw = ctx.device_alloc(self.raw.size)
        ctx.to_device(self.d_raw, self.raw)
        self.d_lanes = ctx.device_alloc(self.lanes_in.nbytes)
        self.base = None   # the device form's lanes, once they have passed the model

    def close(self):
        self.ctx.device_free(self.d_raw)
        self.ctx.device_free(self.d_lanes)

    def fill(self):
        self.ctx.to_device(self.d_lanes, self.lanes_in)

    def read(self):
        return self.ctx.to_host(np.zeros_like(self.lanes_in), self.d_lanes)

    def args(self):
        return dict(d_lanes=self.d_lanes, n_lanes=self.n_lanes, lane_stride=self.stride, n_samples=self.n_samples)

    def device_form(self, rows, d_raw=None, raw_bytes=None):
        self.ctx.ingest_resample(rows, self.up, self.down, self.taps, raw=self.d_raw if d_raw is None else d_raw,
                                 raw_bytes=self.raw.size if raw_bytes is None else raw_bytes, **self.args())

    def host_form(self, rows):
        self.ctx.ingest_resample(rows, self.up, self.down, self.taps, raw=[self.raw] * len(rows), **self.args())

    def first(self):
        if self.base is None:
            self.fill()
            self.device_form(self.rows)
            got = self.read()
            rc.compare_lanes(got, self.table, self.want, self.lanes_want, self.up, self.n_taps, "fvad_ingest_resample_device")
            self.base = got
        return self.base

    def status(self, rows, host=False, raw="own", raw_bytes=None, up=None, down=None, taps="own", n_taps=None, d_lanes="own", n_lanes=None,
               n_samples=None, stride=None):
        """the C call itself -> status"""
        fv = self.fv
        src = np.ascontiguousarray(np.asarray([self.rows[0]] if rows is None else rows, np.uint64).reshape(-1, rc.FIELDS))
        rp = src.ctypes.data_as(C.POINTER(C.c_uint64)) if rows is not None else None
        tp = np.ascontiguousarray(self.taps if isinstance(taps, str) else taps, np.float32) if taps is not None else None
        tail = (self.up if up is None else up, self.down if down is None else down, None if tp is None else fv.fptr(tp),
                (0 if tp is None else tp.size) if n_taps is None else n_taps, fv.vp(self.d_lanes if isinstance(d_lanes, str) else d_lanes),
                self.n_lanes if n_lanes is None else n_lanes, self.stride if stride is None else stride, self.n_samples if n_samples is None else n_samples)
        if host:
            ptrs = (fv.vp * max(len(src), 1))(*([self.raw.ctypes.data] * len(src)))
            return fv.lib().fvad_ingest_resample(self.ctx.h, ptrs if isinstance(raw, str) else raw, rp, len(src), *tail)
        return fv.lib().fvad_ingest_resample_device(self.ctx.h, fv.vp(self.d_raw if isinstance(raw, str) else raw),
                                                    self.raw.size if raw_bytes is None else raw_bytes, rp, len(src), *tail)


@pytest.fixture(scope="module", params=PARAMS, ids=[f"{u}-{d}-half{h}-{k}" for u, d, h, k in PARAMS])
def dev(request, fv, gpu_ctx):
    d = Device(fv, gpu_ctx, *request.param)
    yield d
    d.close()


def test_case_table_within_the_bound_of_the_model(dev):
    # PCM16 / PCM24 / f32 files of 1, 2, 3 and 64 channels at odd and even byte offsets, outputs on both sides of one and two
    # tiles, from the file's first and up to its last output, files shorter than the filter, of 1 and of 0 frames, the 4
    # destination alignments with fills: every output within g B + ulp of the float64 model, zeros and canaries exact
    dev.first()


@pytest.mark.parametrize("pieces", [2, 7])
def test_slices_are_the_file(dev, pieces):
    base = dev.first()
    rng = np.random.default_rng(pieces)
    rows = []
    for row in dev.rows:
        o, n = int(row[9]), int(row[10])
        if n < 8:
            rows.append(tuple(int(v) for v in row))
            continue
        cuts = np.sort(rng.choice(np.arange(o + 1, o + n), pieces - 1, replace=False))
        rows += rc.slices(row, cuts, dev.up, dev.down, dev.n_taps)
    assert len(rows) > len(dev.rows)
    dev.fill()
    dev.device_form(rows[::-1])
    ic.compare(dev.read(), base, f"every file in {pieces} slices, each given exactly its window")


@pytest.mark.parametrize("ring", ["1024", None], ids=["1KB-ring", "default-ring"])
def test_host_form_equals_device_form_however_the_ring_cuts(dev, ring):
    base = dev.first()
    with dev.ctx.options(ingest_ring_bytes=ring):
        dev.fill()
        dev.host_form(dev.rows)
        ic.compare(dev.read(), base, f"fvad_ingest_resample, ring {ring}")


@pytest.mark.parametrize("dev", PARAMS[:1], indirect=True, ids=["{}-{}-half{}-{}".format(*PARAMS[0])])   # (the shortest filter)
def test_more_slices_than_a_batch_holds(dev):
    # a batch of fvad_ingest_resample takes 2048 sources at most: the rows cut at seeded outputs into more slices than that,
    # each given exactly its window, through the default ring -- the pump flushes for the count and not for the bytes
    base = dev.first()
    rng = np.random.default_rng(2048)
    big = [i for i, row in enumerate(dev.rows) if int(row[10]) >= 8]
    inner = np.concatenate([np.stack([np.full(int(dev.rows[i][10]) - 1, i), int(dev.rows[i][9]) + np.arange(1, int(dev.rows[i][10]))], axis=1) for i in big])
    chosen = inner[rng.choice(len(inner), 2200, replace=False)]
    rows = []
    for i, row in enumerate(dev.rows):
        rows += rc.slices(row, sorted(chosen[chosen[:, 0] == i, 1].tolist()), dev.up, dev.down, dev.n_taps)
    assert len(rows) == len(dev.rows) + 2200 > 2048
    dev.fill()
    dev.host_form(rows)
    ic.compare(dev.read(), base, f"fvad_ingest_resample, {len(rows)} slices")


def test_order_company_and_reruns_change_nothing(dev):
    base = dev.first()
    dev.fill()
    dev.device_form(dev.rows[::-1])
    ic.compare(dev.read(), base, "the sources reversed")
    dev.device_form(dev.rows)                      # a second run over the lanes the first one wrote
    ic.compare(dev.read(), base, "a second run")
    dev.fill()
    for row in dev.rows:
        dev.device_form(row[None])
    ic.compare(dev.read(), base, "one source per call")


def test_pcm_files_equal_their_f32_twins(dev):
    base = dev.first()
    tw = rc.twin_f32(dev.table)
    d_raw = dev.ctx.device_alloc(tw["raw"].size)
    try:
        dev.ctx.to_device(d_raw, tw["raw"])
        dev.fill()
        dev.device_form(tw["rows"], d_raw=d_raw, raw_bytes=tw["raw"].size)
        ic.compare(dev.read(), base, "f32 files holding s / 32768 and s / 8388608")
    finally:
        dev.ctx.device_free(d_raw)


def test_refused_calls_leave_the_lanes_alone(dev):
    dev.fill()
    # a stereo file's row that ends at the file's last output: its window ends at the file's last frame
    good = dev.rows[(dev.rows[:, 10] > 8) & (dev.rows[:, 2] == 2) & (dev.rows[:, 9] > 0)][0].copy()
    assert int(good[9]) + int(good[10]) == rc.out_frames(int(good[8]), dev.up, dev.down)

    def edit(col, value):
        r = good.copy()
        r[col] = value
        return r

    for host in (False, True):
        assert dev.status(good, host=host, d_lanes=None) == INVALID
        assert dev.status(good, host=host, raw=None) == INVALID
        assert dev.status(None, host=host) == INVALID
        assert dev.status(good, host=host, taps=None) == INVALID
        assert dev.status(good, host=host, n_taps=dev.n_taps - 1) == INVALID
        assert dev.status(good, host=host, up=0) == INVALID and dev.status(good, host=host, up=641) == INVALID
        assert dev.status(good, host=host, down=0) == INVALID
        bad = dev.taps.copy()
        bad[0] = np.nan
        assert dev.status(good, host=host, taps=bad) == INVALID
        assert dev.status(edit(3, 3), host=host) == INVALID
        assert dev.status(edit(2, 0), host=host) == INVALID and dev.status(edit(2, 65), host=host) == INVALID
        assert dev.status(edit(6, int(good[5]) + int(good[10]) - 1), host=host) == INVALID
        assert dev.status(edit(9, rc.out_frames(int(good[8]), dev.up, dev.down) - int(good[10]) + 1), host=host) == INVALID   # one output past the file
        assert dev.status(edit(1, int(good[1]) - 1), host=host) == INVALID            # the window's last frame not given
        assert dev.status(edit(1, int(good[1]) + 1), host=host) == INVALID            # a frame past the file given
        assert dev.status(np.stack([good, good]), host=host) == INVALID              # overlapping destinations
        assert dev.status(good, host=host, d_lanes=dev.d_lanes + 1) == INVALID       # lanes not aligned to their samples
        assert dev.status(good, host=host, stride=dev.n_samples - 1) == INVALID
        assert dev.status(edit(4, dev.n_lanes), host=host) == RANGE
        assert dev.status(good, host=host, n_samples=int(good[6]) - 1, stride=dev.stride) == RANGE
    assert dev.status(good, raw_bytes=int(good[0]) + int(good[1]) * int(good[2]) * ic.SAMPLE_BYTES[int(good[3])] - 1) == RANGE
    empty = np.zeros((0, rc.FIELDS), np.uint64)
    assert dev.status(empty) == 0 and dev.status(empty, host=True) == 0           # nothing to do
    assert dev.status(empty, up=0) == INVALID                                     # ... but the ratio still counts
    ic.compare(dev.read(), dev.lanes_in, "the canaries after the refused calls")


def test_kernel_times_name_ingest_resample(dev):
    ctx = dev.ctx
    was = ctx.timing
    ctx.enable_timing(True)
    try:
        ctx.kernel_times()
        dev.device_form(dev.rows)
        times = ctx.kernel_times()
    finally:
        ctx.enable_timing(was)
    assert list(times) == ["ingest_resample"] and times["ingest_resample"] > 0, times


# ---------------------------------------------------------------- single cases
def _one_call(fv, ctx, raw, rows, up, down, taps, n_lanes, n_samples):
    lanes = ic.canaries(n_lanes, n_samples, False)
    d_raw, d_lanes = ctx.device_alloc(max(raw.size, 1)), ctx.device_alloc(lanes.nbytes)
    try:
        ctx.to_device(d_raw, raw)
        ctx.to_device(d_lanes, lanes)
        ctx.ingest_resample(rows, up, down, taps, raw=d_raw, raw_bytes=raw.size, d_lanes=d_lanes, n_lanes=n_lanes, lane_stride=n_samples, n_samples=n_samples)
        return ctx.to_host(np.zeros_like(lanes), d_lanes)
    finally:
        ctx.device_free(d_raw)
        ctx.device_free(d_lanes)


def test_index_arithmetic_is_64_bit(fv, gpu_ctx):
    # outputs whose o * down is past 2^32 (10.1 minutes into a 44.1 kHz file), over a window of 300 frames: the same frames
    # presented as a file position below 2^32 with the same o mod up -- the same phases against the same samples, so the same
    # bits -- and the float64 model at the large position
    up, down = 160, 147
    taps = fv.resample_design(up, down)
    n_out, shift = 280, 29_000_000 // up * up          # outputs moved back by a multiple of up: frames by shift / up * down
    o_big = 29_217_469 + 3
    o_small = o_big - shift
    assert o_big * down > 1 << 32 and (o_small + n_out) * down < 1 << 32 and o_big % up == o_small % up
    ff_big = 40_000_000
    lo, hi = rc.window(up, down, taps.size, ff_big, o_big, n_out)
    assert 280 < hi - lo <= 300
    moved = shift // up * down
    assert rc.window(up, down, taps.size, ff_big - moved, o_small, n_out) == (lo - moved, hi - moved)
    raw = np.concatenate([np.full(3, ic.PAD_BYTE, np.uint8), rc.file_bytes(np.random.default_rng(8), rc.PCM16, (hi - lo) * 2)])
    n_samples = n_out + 13
    rows = lambda base, ff, o: [(3, hi - lo, 2, rc.PCM16, 1, 5, n_out + 9, base, ff, o, n_out)]
    big = _one_call(fv, gpu_ctx, raw, rows(lo, ff_big, o_big), up, down, taps, 4, n_samples)
    small = _one_call(fv, gpu_ctx, raw, rows(lo - moved, ff_big - moved, o_small), up, down, taps, 4, n_samples)
    ic.compare(big, small, "the window at o * down > 2^32 against the same window below 2^32")
    x = rc.decode_f64(raw, 3, hi - lo, 2, rc.PCM16)
    y, B = rc.resample_model(x, taps, up, down, o_big, n_out, frame_base=lo, file_frames=ff_big)
    rc.compare(big[1:3, 5:5 + n_out], y, B, up, taps.size, "the window at o * down > 2^32")
    assert np.all(np.abs(y).max(axis=1) > 0.1)
    want = ic.canaries(4, n_samples, False)
    ic.bits(want)[1:3, 5:n_out + 9] = 0
    got = big.copy()
    ic.bits(got)[1:3, 5:5 + n_out] = 0
    ic.compare(got, want, "canaries and fill around the window")


def test_ratio_one_with_the_single_tap_is_fvad_ingest(fv, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(4)
    n, n_samples = 9001, 9030
    parts, rows, rrows, at = [], [], [], 0
    for i, (fmt, ch) in enumerate(((rc.PCM16, 2), (rc.PCM24, 1), (rc.F32, 3))):
        parts.append(np.full(1 + i, ic.PAD_BYTE, np.uint8))
        at += 1 + i
        data = rc.file_bytes(rng, fmt, n * ch)
        parts.append(data)
        lane = 1 + sum(r[2] for r in rows)
        rows.append((at, n, ch, fmt, lane, 3 + i, n + 20))
        rrows.append((at, n, ch, fmt, lane, 3 + i, n + 20, 0, n, 0, n))
        at += data.size
    raw = np.concatenate(parts)
    got = _one_call(fv, ctx, raw, rrows, 1, 1, np.ones(1, np.float32), 8, n_samples)
    lanes = ic.canaries(8, n_samples, False)
    d_raw, d_lanes = ctx.device_alloc(raw.size), ctx.device_alloc(lanes.nbytes)
    try:
        ctx.to_device(d_raw, raw)
        ctx.to_device(d_lanes, lanes)
        ctx.ingest(rows, raw=d_raw, raw_bytes=raw.size, d_lanes=d_lanes, n_lanes=8, lane_stride=n_samples, n_samples=n_samples)
        want = ctx.to_host(np.zeros_like(lanes), d_lanes)
    finally:
        ctx.device_free(d_raw)
        ctx.device_free(d_lanes)
    written = ic.bits(want) != ic.CANARY_F32
    assert written.sum() == 2 * (n + 17) + (n + 16) + 3 * (n + 15) and np.array_equal(written, ic.bits(got) != ic.CANARY_F32)
    assert np.array_equal(got[written], want[written])   # as values: fma(1, x, +0) is x, and +0 for x = -0
