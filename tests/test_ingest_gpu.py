"""The device-side ingest on the GPU (fvad_ingest_device, fvad_ingest): the case table of ingest_cases.py against the numpy
model in all four format pairs, bit for bit, with canaries around everything the sources write; the host form through a ring so
small that sources are cut several times; the invariances; the refused calls; the engine fed from ingested lanes; and the
harness with ingest="device" against ingest="host"."""
import ctypes as C
import filecmp
import json
import os
import shutil
import struct

import numpy as np
import pytest

import ingest_cases as ic
from test_harness import write_wav
from test_vad_parts_gpu import GRID
from test_vad_score_gpu import assert_bits, write_plan

pytestmark = pytest.mark.gpu

INVALID, RANGE = -100, -6
SMALL_RING = "6000"   # bytes: the table's largest source (32 KB) crosses it in six pieces


def good_row():
    return (0, 1, 1, ic.PCM16, 1, 0, 1)


class Device:
    """a case table's raw bytes on the device and canary-filled lanes"""

    def __init__(self, fv, ctx, out_pcm16):
        self.fv, self.ctx, self.out_pcm16 = fv, ctx, out_pcm16
        t = ic.case_table(out_pcm16)
        self.raw, self.sources = t["raw"], t["sources"]
        self.n_lanes, self.stride, self.n_samples = t["n_lanes"], t["lane_stride"], t["n_samples"]
        self.lanes_in = ic.canaries(self.n_lanes, self.stride, out_pcm16)
        self.want = ic.ingest_model(self.raw, self.sources, out_pcm16, self.lanes_in)   # computed once, shared, never changed
        self.d_raw = ctx.device_alloc(self.raw.size)
        ctx.to_device(self.d_raw, self.raw)
        self.d_lanes = ctx.device_alloc(self.lanes_in.nbytes)

    def close(self):
        self.ctx.device_free(self.d_raw)
        self.ctx.device_free(self.d_lanes)

    def fill(self):
        self.ctx.to_device(self.d_lanes, self.lanes_in)

    def read(self):
        return self.ctx.to_host(np.zeros_like(self.lanes_in), self.d_lanes)

    def args(self):
        return dict(out_pcm16=self.out_pcm16, d_lanes=self.d_lanes, n_lanes=self.n_lanes, lane_stride=self.stride, n_samples=self.n_samples)

    def device_form(self, sources):
        self.ctx.ingest(sources, raw=self.d_raw, raw_bytes=self.raw.size, **self.args())

    def host_form(self, sources):
        self.ctx.ingest(sources, raw=[self.raw] * len(sources), **self.args())

    def status(self, sources, host=False, raw="own", raw_bytes=None, out_format=None, d_lanes="own", n_lanes=None, n_samples=None, stride=None):
        """the C call itself -> status"""
        fv = self.fv
        src = np.ascontiguousarray(np.asarray([good_row()] if sources is None else sources, np.uint64).reshape(-1, 7))
        rows = src.ctypes.data_as(C.POINTER(C.c_uint64)) if sources is not None else None   # (None: a NULL table of one row)
        tail = (int(self.out_pcm16) if out_format is None else out_format, fv.vp(self.d_lanes if d_lanes == "own" else d_lanes),
                self.n_lanes if n_lanes is None else n_lanes, self.stride if stride is None else stride,
                self.n_samples if n_samples is None else n_samples)
        if host:
            ptrs = (fv.vp * max(len(src), 1))(*([self.raw.ctypes.data] * len(src)))
            return fv.lib().fvad_ingest(self.ctx.h, ptrs if raw == "own" else raw, rows, len(src), *tail)
        return fv.lib().fvad_ingest_device(self.ctx.h, fv.vp(self.d_raw if raw == "own" else raw),
                                           self.raw.size if raw_bytes is None else raw_bytes, rows, len(src), *tail)


@pytest.fixture(scope="module", params=[False, True], ids=["to-f32", "to-pcm16"])
def dev(request, fv, gpu_ctx):
    d = Device(fv, gpu_ctx, request.param)
    yield d
    d.close()


def test_case_table_matches_the_model(dev):
    # PCM16 / PCM24 / f32 sources into f32 lanes, PCM16 into PCM16 lanes: every length around the tile, channel count, byte and
    # destination alignment and fill of the table; whatever no source writes is still the canary (the model starts from them)
    dev.fill()
    dev.device_form(dev.sources)
    ic.compare(dev.read(), dev.want, "fvad_ingest_device")


@pytest.mark.parametrize("ring", [SMALL_RING, None], ids=["small-ring", "default-ring"])
def test_host_form_equals_device_form_however_the_ring_cuts(dev, ring):
    with dev.ctx.options(ingest_ring_bytes=ring):
        dev.fill()
        dev.host_form(dev.sources)
        ic.compare(dev.read(), dev.want, f"fvad_ingest, ring {ring}")


def test_more_pieces_than_a_batch_holds(dev):
    # a batch of fvad_ingest takes 4096 sources at most: the table's sources cut at seeded frame boundaries into more rows than
    # that, so that the pump flushes for the count and not for the bytes.  A piece is a source of its own on its source's lanes,
    # its bytes and destination moved on by the frames in front of it; only the last piece of a source keeps the fill.
    rng = np.random.default_rng(4096)
    src = dev.sources.astype(np.int64)
    inner = np.concatenate([np.stack([np.full(n - 1, i), np.arange(1, n)], axis=1) for i, n in enumerate(src[:, 1]) if n > 1])
    chosen = inner[rng.choice(len(inner), 4300, replace=False)]
    rows = []
    for i, (byte_offset, n, ch, fmt, first_lane, dst, fill_to) in enumerate(src.tolist()):
        edges = [0] + sorted(chosen[chosen[:, 0] == i, 1].tolist()) + [n]
        for a, b in zip(edges[:-1], edges[1:]):
            rows.append((byte_offset + a * ch * ic.SAMPLE_BYTES[fmt], b - a, ch, fmt, first_lane, dst + a, fill_to if b == n else dst + b))
    assert len(rows) == len(src) + 4300 > 4096
    dev.fill()
    dev.host_form(np.array(rows, np.uint64))
    ic.compare(dev.read(), dev.want, f"fvad_ingest, {len(rows)} pieces")


def test_order_batching_and_reruns_change_nothing(dev):
    dev.fill()
    dev.device_form(dev.sources[::-1])
    ic.compare(dev.read(), dev.want, "the sources reversed")
    dev.device_form(dev.sources)                      # a second run over the lanes the first one wrote
    ic.compare(dev.read(), dev.want, "a second run")
    dev.fill()
    for row in dev.sources:
        dev.device_form(row[None])
    ic.compare(dev.read(), dev.want, "one source per call")
    dev.fill()
    with dev.ctx.options(ingest_ring_bytes=SMALL_RING):
        for row in dev.sources[::-1]:
            dev.host_form(row[None])
    ic.compare(dev.read(), dev.want, "one source per host call, reversed")


def test_refused_calls_leave_the_lanes_alone(dev):
    dev.fill()
    good = dev.sources[dev.sources[:, 1] > 0][0].copy()

    def edit(col, value):
        r = good.copy()
        r[col] = value
        return r

    other_format = 2 if dev.out_pcm16 else 3   # PCM24 -> PCM16 is a conversion; format 3 does not exist
    for host in (False, True):
        assert dev.status(good, host=host, d_lanes=None) == INVALID
        assert dev.status(good, host=host, raw=None) == INVALID
        assert dev.status(None, host=host) == INVALID
        assert dev.status(good, host=host, out_format=2) == INVALID
        assert dev.status(edit(3, other_format), host=host) == INVALID
        assert dev.status(edit(2, 0), host=host) == INVALID and dev.status(edit(2, 65), host=host) == INVALID
        assert dev.status(edit(6, int(good[5]) + int(good[1]) - 1), host=host) == INVALID
        assert dev.status(np.stack([good, good]), host=host) == INVALID                         # overlapping destinations
        assert dev.status(good, host=host, d_lanes=dev.d_lanes + 1) == INVALID                  # lanes not aligned to their samples
        assert dev.status(good, host=host, stride=dev.n_samples - 1) == INVALID
        assert dev.status(edit(4, dev.n_lanes), host=host) == RANGE
        assert dev.status(good, host=host, n_samples=int(good[6]) - 1, stride=dev.stride) == RANGE
    assert dev.status(good, raw_bytes=int(good[0]) + int(good[1]) * int(good[2]) * ic.SAMPLE_BYTES[int(good[3])] - 1) == RANGE
    if dev.out_pcm16:
        assert dev.status(edit(3, ic.F32)) == INVALID
    assert dev.status(np.zeros((0, 7), np.uint64)) == 0 and dev.status(np.zeros((0, 7), np.uint64), host=True) == 0   # nothing to do
    ic.compare(dev.read(), dev.lanes_in, "the canaries after the refused calls")


def test_kernel_times_name_ingest(dev):
    ctx = dev.ctx
    was = ctx.timing
    ctx.enable_timing(True)
    try:
        ctx.kernel_times()
        dev.device_form(dev.sources)
        times = ctx.kernel_times()
    finally:
        ctx.enable_timing(was)
    assert list(times) == ["ingest"] and times["ingest"] > 0, times


def test_a_source_without_frames_reads_no_byte(dev):
    # a slice behind a file's end: no frames, a byte_offset past the buffer, only zeros -- through the binding's host form, whose
    # own bounds check applies to sources that read
    dev.fill()
    row = np.array([[dev.raw.size + 12345, 0, 2, ic.PCM16, 1, 3, 3 + 11]], np.uint64)
    dev.ctx.ingest(row, raw=[dev.raw], **dev.args())
    want = dev.lanes_in.copy()
    ic.bits(want)[1:3, 3:14] = 0
    ic.compare(dev.read(), want, "a fill-only source")
    with pytest.raises(dev.fv.FvadError):   # one frame at that offset is refused by the binding
        row[0, 1], row[0, 6] = 1, 3 + 12
        dev.ctx.ingest(row, raw=[dev.raw], **dev.args())
    ic.compare(dev.read(), want, "after the refused source")


# ------------------------------------------------------------------ feeding the engine
def test_the_engine_takes_ingested_lanes(fv, gpu_ctx):
    ctx = gpu_ctx
    n, nch = 3 * 24000, 2
    pcm = np.random.default_rng(9).integers(-12000, 12000, (nch, n)).astype(np.int16)
    raw = np.ascontiguousarray(pcm.T).view(np.uint8).reshape(-1)
    src = [(0, n, nch, ic.PCM16, 0, 0, n)]
    held = []

    def dalloc(nbytes):
        held.append(ctx.device_alloc(nbytes))
        return held[-1]

    try:
        d_old, d_new, d_old16, d_new16 = dalloc(nch * n * 4), dalloc(nch * n * 4), dalloc(nch * n * 2), dalloc(nch * n * 2)
        ctx.to_device(d_old, pcm.astype(np.float32) * np.float32(1.0 / 32768.0))      # the old way: converted on the host
        ctx.to_device(d_old16, pcm)
        ctx.ingest(src, raw=[raw], d_lanes=d_new, n_lanes=nch, lane_stride=n, n_samples=n)
        ctx.ingest(src, raw=[raw], out_pcm16=True, d_lanes=d_new16, n_lanes=nch, lane_stride=n, n_samples=n)
        d_den, d_den16 = dalloc(nch * n * 4), dalloc(nch * n * 2)
        out = []
        for d_pcm, i16 in ((d_old, False), (d_new, False), (d_old16, True), (d_new16, True)):
            d_band, d_rms = dalloc(nch * (n // 1024) * 4), dalloc(nch * 3 * 4)
            if i16:
                ctx._ck(fv.lib().fvad_engine_enqueue_device_i16(ctx.h, fv.vp(d_pcm), nch, n, n, fv.vp(d_den16), fv.vp(d_band), fv.vp(d_rms), None),
                        "fvad_engine_enqueue_device_i16")
            else:
                ctx.enqueue_device(d_pcm, nch, n, n, d_den, d_band, d_rms)
            out.append((ctx.to_host(np.empty((nch, n // 1024), np.float32), d_band), ctx.to_host(np.empty((nch, 3), np.float32), d_rms)))
        for a, b in ((0, 1), (2, 3)):
            assert_bits(out[a][0], out[b][0])
            assert_bits(out[a][1], out[b][1])
        assert np.all(out[1][1] > 0)
    finally:
        for d in held:
            ctx.device_free(d)


# ------------------------------------------------------------------ the harness
# unequal lengths with a partial last chunk; the two stereo files differ by more than a slice and its halo, so that in the
# sliced runs the short one has ended (a source without frames, only zeros) while its group goes on
STREAMS = [(1, "pcm16", 33.9), (2, "f32", 61.1), (2, "pcm16", 20.2)]


def _same_grid(a, b):
    assert_bits(a["stats"], b["stats"])
    assert a["configs"] == b["configs"] and a["slices"] == b["slices"]
    assert json.dumps(a["rows"], sort_keys=True) == json.dumps(b["rows"], sort_keys=True)


def test_run_grid_device_ingest_equals_host_ingest(pkg, gpu_ctx, tmp_path):
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, STREAMS)
    with gpu_ctx.options(reproducible="1", ingest_ring_bytes="1048576"):   # (every file crosses the ring in pieces)
        for kw in ({}, {"slice_chunks": 16}, {"slice_chunks": 16, "overlap": True}):
            host = sim.run_grid(plan, GRID, ctx=gpu_ctx, out=None, vad_on="device", score_on="device", **kw)
            dev = sim.run_grid(plan, GRID, ctx=gpu_ctx, out=None, vad_on="device", score_on="device", ingest="device", **kw)
            _same_grid(dev, host)
            assert float(host["stats"][:, :, 1].sum()) > 0            # (true positives: the machines found the speech)
    with pytest.raises(ValueError):
        sim.run_grid(plan, GRID, ctx=gpu_ctx, out=None, ingest="gpu")


def test_run_clips_device_ingest_writes_the_same_files(pkg, gpu_ctx, tmp_path):
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, STREAMS)
    with gpu_ctx.options(reproducible="1"):
        text_h, res_h = sim.run_clips(plan, str(tmp_path / "host"), ctx=gpu_ctx)
        text_d, res_d = sim.run_clips(plan, str(tmp_path / "device"), ctx=gpu_ctx, ingest="device")
    assert text_h == text_d
    for h, d in zip(res_h, res_d):
        assert len(h["segments"]) >= 1                                # a segment per instance
        assert h["segments"] == d["segments"] and h["audit"] == d["audit"] and h["clips"] == d["clips"]
    names = sorted(os.listdir(tmp_path / "host"))
    assert names == sorted(os.listdir(tmp_path / "device")) and len(names) > 3
    match, mismatch, errors = filecmp.cmpfiles(tmp_path / "host", tmp_path / "device", names, shallow=False)
    assert match == names and not mismatch and not errors


def write_pcm24(path, q, sample_rate=48000):
    """q [n_channels][n_frames] int32 in [-2^23, 2^23) -> a 24-bit PCM WAV file"""
    nch, n = q.shape
    data = np.ascontiguousarray(q.T).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    fmt = struct.pack("<HHIIHH", 1, nch, sample_rate, sample_rate * nch * 3, nch * 3, 24)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)


def test_a_24_bit_file_runs_with_device_ingest_only(pkg, fv, gpu_ctx, tmp_path):
    sim, synth = pkg.simulator, pkg.synth
    for d in ("p24", "f32"):
        (tmp_path / d).mkdir()
    plan24 = write_plan(pkg, tmp_path / "p24", STREAMS)
    shutil.copytree(tmp_path / "p24", tmp_path / "f32", dirs_exist_ok=True)
    planf = str(tmp_path / "f32" / "plan.json")
    # the stereo f32 stream (write_plan's stream 1) quantised to 24 bits: once as PCM24, once as the f32 file holding s / 2^23
    pcm, _ = synth.make_stream(STREAMS[1][2], seed=501, n_channels=2)
    q = np.clip(np.rint(pcm.astype(np.float64) * 8388608.0), -8388608, 8388607).astype(np.int32)
    write_pcm24(str(tmp_path / "p24" / "s1.wav"), q)
    write_wav(str(tmp_path / "f32" / "s1.wav"), q.astype(np.float32) * np.float32(1.0 / 8388608.0), fmt="f32")
    assert fv.wav_probe(str(tmp_path / "p24" / "s1.wav"))["format"] == fv.INGEST_PCM24
    with gpu_ctx.options(reproducible="1"):
        for kw in ({}, {"slice_chunks": 16}):
            want = sim.run_grid(planf, GRID, ctx=gpu_ctx, out=None, vad_on="device", score_on="device", **kw)
            got = sim.run_grid(plan24, GRID, ctx=gpu_ctx, out=None, vad_on="device", score_on="device", ingest="device", **kw)
            _same_grid(got, want)
            with pytest.raises(fv.FvadError, match="--ingest device"):
                sim.run_grid(plan24, GRID, ctx=gpu_ctx, out=None, vad_on="device", score_on="device", **kw)
