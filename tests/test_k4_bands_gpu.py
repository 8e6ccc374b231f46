"""K4 on the GPU against float64, one kernel at a time: fvad_engine_band_sums_device (vadfft1024_bands_kernel, vadfft_bands_kernel<R>,
rfft_generic_bands_kernel) on inputs made to break FFT kernels, and the single-band engine kernels on the engine's own denoised
audio.  Reference, metric and tolerance: k4_cases.py (GPU_FACTOR x the oracle's measured distance; nothing here is derived
from GPU output).  Every test prints its worst distance before it asserts (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import k4_cases as k4

pytestmark = pytest.mark.gpu

CANARY = 0x7FC0BEEF     # a NaN no kernel produces


def band_tol(F):
    return k4.GPU_FACTOR * k4.ORACLE_BAND_UNITS[F]


def bin_tol(F):
    return k4.GPU_FACTOR * k4.ORACLE_BIN_UNITS[F]


class DeviceBands:
    """lanes of whole frames on the device, every float around them NaN, and a band-sum buffer full of canaries"""

    def __init__(self, ctx, lanes, n_samples, F, n_bands, lane_stride=None, band_stride=None, offset=0):
        lanes = np.asarray(lanes, np.float32)
        self.ctx, self.F, self.L, self.n_samples, self.offset = ctx, F, lanes.shape[0], n_samples, offset
        self.n_frames = n_samples // F
        self.lane_stride = n_samples if lane_stride is None else lane_stride
        self.band_stride = max(self.n_frames, 1) if band_stride is None else band_stride
        self.n_bands = n_bands
        # only the whole frames are real: the tail of n_samples past them, the gaps between lanes and the floats in front of an
        # offset base stay NaN -- a kernel that read any of them into a frame would show it
        host = np.full(offset + self.L * self.lane_stride + 8, np.nan, np.float32)
        used = self.n_frames * F
        for l in range(self.L):
            host[offset + l * self.lane_stride:offset + l * self.lane_stride + used] = lanes[l, :used]
        self.d_den = ctx.device_alloc(host.nbytes)
        self.d_out = ctx.device_alloc(max(n_bands, 1) * self.L * self.band_stride * 4)
        ctx.to_device(self.d_den, host)
        self.reset()

    def reset(self):
        self.ctx.to_device(self.d_out, np.full(max(self.n_bands, 1) * self.L * self.band_stride, CANARY, np.uint32))

    @property
    def base(self):
        return self.d_den + 4 * self.offset

    def raw(self, fv, bins, n_bands=None, n_lanes=None, lane_stride=None, band_stride=None, base=None, fft_size=None):
        """the C call's status, nothing raised"""
        b = np.ascontiguousarray(np.asarray(bins, np.int32).reshape(-1, 2))
        return fv.lib().fvad_engine_band_sums_device(
            self.ctx.h, fv.vp(self.base if base is None else base), self.L if n_lanes is None else n_lanes,
            self.lane_stride if lane_stride is None else lane_stride, self.n_samples, self.F if fft_size is None else fft_size,
            b.ctypes.data_as(C.POINTER(C.c_int32)), b.shape[0] if n_bands is None else n_bands, fv.vp(self.d_out),
            self.band_stride if band_stride is None else band_stride)

    def run(self, bands):
        assert len(bands) == self.n_bands
        self.ctx.band_sums_device(self.base, self.L, self.lane_stride, self.n_samples, bands, self.d_out, self.band_stride,
                                  fft_size=self.F)
        return self.out()

    def out(self):
        """[n_bands][L][band_stride] as uint32 bits"""
        return self.ctx.to_host(np.empty((max(self.n_bands, 1), self.L, self.band_stride), np.uint32), self.d_out)

    def close(self):
        self.ctx.device_free(self.d_den)
        self.ctx.device_free(self.d_out)


def check_rows(out, n_frames, ref, bands, F, what):
    """out: DeviceBands.out() bits; ref: float64 bins of the frames, [L * n_frames][NB] lane-major.  Exactly [0, n_frames) of
    every (band, lane) row is written and lies within tolerance; every canary behind it survives.  Returns the f32 rows."""
    got = np.ascontiguousarray(out[:, :, :n_frames]).view(np.float32)
    assert (out[:, :, n_frames:] == CANARY).all(), f"{what}: a canary behind the {n_frames} frames of a row was overwritten"
    assert not (out[:, :, :n_frames] == CANARY).any(), f"{what}: a frame's band sum was not written"
    worst, (j, f) = k4.band_units(got.reshape(len(bands), -1), ref, bands)
    print(f"\n    {what}: worst {worst:.3g} units (tolerance {band_tol(F):.3g}) at band {bands[j]}, lane {f // max(n_frames, 1)}, "
          f"frame {f % max(n_frames, 1)}")
    assert worst <= band_tol(F), (what, worst, bands[j], f)
    return got


def assert_duplicates_identical(got, bands):
    """rows of the same band are the same bits"""
    first, n_dup = {}, 0
    for j, b in enumerate(bands):
        if b in first:
            n_dup += 1
            assert np.array_equal(got[j].view(np.uint32), got[first[b]].view(np.uint32)), (b, first[b], j)
        else:
            first[b] = j
    return n_dup


def lanes_from_table(frames, n_lanes, per_lane):
    """lane l holds frames (l + i) mod n of the table, i < per_lane: no two neighbouring lanes alike.  (lanes [L][per_lane * F],
    idx [L][per_lane])"""
    idx = (np.arange(n_lanes)[:, None] + 5 * np.arange(per_lane)[None, :]) % frames.shape[0]
    return frames[idx].reshape(n_lanes, -1), idx


MIXED_1024 = k4.PRUNED_EDGES + k4.PRUNED_NEIGHBOURS + [(11, 43), (0, 0), (0, 512), (512, 512), (16, 16), (11, 43), (1, 48)]


def geometry_bands(F):
    return MIXED_1024 if F == 1024 else k4.edge_bands(F) + [k4.edge_bands(F)[1]]


# ------------------------------------------------------------------ a. every size x the frame table x the band set

@pytest.mark.parametrize("F", k4.SIZES)
def test_frame_table_against_float64(gpu_ctx, F):
    # one-hot tones under single-bin bands: every bin of every kernel by itself (bins 16 and 32 of the pruned kernel -- its
    # k1 == 0 lanes --, bins 0 and F/2 everywhere); at 1024 points the set holds both launch classes; more than 256 bands
    # up to 2048 points: the launch split too
    frames, labels = k4.frame_table(F)
    bands = k4.band_set(F)
    n = frames.shape[0]
    d = DeviceBands(gpu_ctx, frames.reshape(1, -1), n * F, F, len(bands), band_stride=n + 3)
    try:
        got = check_rows(d.run(bands), n, k4.ref_bins(frames, F), bands, F, f"{F} points, {n} frames x {len(bands)} bands")
    finally:
        d.close()
    assert assert_duplicates_identical(got, bands) >= 4
    silent = labels.index("silence")
    assert (got[:, 0, silent].view(np.uint32) == 0).all()       # +0.0, every band


# ------------------------------------------------------------------ b. geometry

@pytest.mark.parametrize("F", [1024, 2048, 1000])
def test_partial_groups_tails_strides_and_canaries(gpu_ctx, F):
    frames, _ = k4.sweep_frames(F)
    bins = k4.ref_bins(frames, F)
    bands = geometry_bands(F)
    # 0, 1, 2, 3 frames in the last group of four; exactly one frame; n_samples no multiple of F (the tail is ignored);
    # lane_stride > n_samples; band_stride > n_frames
    for m, extra in ((4, 0), (5, 2), (6, F - 2), (7, 0), (1, 0), (8, F // 2), (9, 0)):
        lanes, idx = lanes_from_table(frames, 3, m + 1)
        n_samples = m * F + extra
        d = DeviceBands(gpu_ctx, lanes, n_samples, F, len(bands), lane_stride=n_samples + 6, band_stride=m + 3)
        try:
            check_rows(d.run(bands), m, bins[idx[:, :m].reshape(-1)], bands, F, f"{F} points, 3 lanes of {m} frames + {extra}")
        finally:
            d.close()
    # just under one frame: OK, nothing written
    lanes, _ = lanes_from_table(frames, 3, 1)
    d = DeviceBands(gpu_ctx, lanes, F - 2, F, len(bands), lane_stride=F + 6, band_stride=3)
    try:
        assert (d.run(bands) == CANARY).all()
    finally:
        d.close()


@pytest.mark.parametrize("F", [1024, 512, 1000])
def test_unaligned_base_and_plain_loads_give_the_aligned_bits(gpu_ctx, F):
    frames, _ = k4.sweep_frames(F)
    bins = k4.ref_bins(frames, F)
    bands = geometry_bands(F)
    m = 7
    lanes, idx = lanes_from_table(frames, 3, m)
    runs = {}
    for name, offset, plain in (("aligned", 0, None), ("8-byte base", 2, None), ("plain loads", 0, 1), ("plain, 8-byte base", 2, 1)):
        # offset 0, lane_stride m F + 4: every lane 16-byte aligned (LDS-DMA staging); offset 2, lane_stride m F + 2: lanes 0
        # and 2 sit 8 bytes off (plain loads), lane 1 is aligned again
        d = DeviceBands(gpu_ctx, lanes, m * F, F, len(bands), lane_stride=m * F + (2 if offset else 4), band_stride=m + 1, offset=offset)
        try:
            assert (d.base % 16 == 8) == bool(offset)
            with gpu_ctx.options(k4_plain_loads=plain):
                runs[name] = check_rows(d.run(bands), m, bins[idx.reshape(-1)], bands, F, f"{F} points, {name}")
        finally:
            d.close()
    for name, got in runs.items():
        assert np.array_equal(got.view(np.uint32), runs["aligned"].view(np.uint32)), (F, name)


@pytest.mark.parametrize("n_lanes", [1, 3, 512, 700])
def test_lane_counts_at_1024(gpu_ctx, n_lanes):
    # 21 frames a lane: six groups of four, the last with one frame.  From 2 * n_cu lanes on, a job has one workgroup
    # (per_job clamps to 1): its four persistent wavefronts walk all six groups, two of them twice around
    F, m = 1024, 21
    frames, _ = k4.sweep_frames(F)
    lanes, idx = lanes_from_table(frames, n_lanes, m)
    d = DeviceBands(gpu_ctx, lanes, m * F, F, len(MIXED_1024), band_stride=m + 2)
    try:
        got = check_rows(d.run(MIXED_1024), m, k4.ref_bins(frames, F)[idx.reshape(-1)], MIXED_1024, F, f"1024 points, {n_lanes} lanes")
    finally:
        d.close()
    assert assert_duplicates_identical(got, MIXED_1024) >= 3


def test_lane_count_generic(gpu_ctx):
    F, m, n_lanes = 1000, 3, 300
    frames, _ = k4.sweep_frames(F)
    bands = geometry_bands(F)
    lanes, idx = lanes_from_table(frames, n_lanes, m)
    d = DeviceBands(gpu_ctx, lanes, m * F + 10, F, len(bands), lane_stride=m * F + 12, band_stride=m + 2)
    try:
        check_rows(d.run(bands), m, k4.ref_bins(frames, F)[idx.reshape(-1)], bands, F, f"{F} points, {n_lanes} lanes")
    finally:
        d.close()


# ------------------------------------------------------------------ c. band counts: fewer and more bands than lanes, the launch split

@pytest.mark.parametrize("F,pruned_only", [(1024, True), (1024, False), (2048, False), (1000, False)])
def test_band_count_sweep(gpu_ctx, F, pruned_only):
    frames, _ = k4.sweep_frames(F)
    n = frames.shape[0]
    bins = k4.ref_bins(frames, F)
    lanes = np.stack([frames.reshape(-1), frames[::-1].reshape(-1)])
    ref = np.concatenate([bins, bins[::-1]])
    for count in k4.BAND_COUNTS:
        bands = k4.cycled_bands(F, count, pruned_only=pruned_only)
        d = DeviceBands(gpu_ctx, lanes, n * F, F, count, band_stride=n + 1)
        try:
            got = check_rows(d.run(bands), n, ref, bands, F, f"{F} points{', pruned only' if pruned_only else ''}, {count} bands")
        finally:
            d.close()
        n_dup = assert_duplicates_identical(got, bands)
        assert n_dup > 0 or count < 64


# ------------------------------------------------------------------ d. the single-band engine kernels on the engine's own audio

ENGINE_CASES = [(1024, b) for b in ((11, 43), (5, 30), (1, 47), (0, 43), (11, 48))] + \
               [(F, b) for F in (512, 2048, 960, 254, 4096) for b in ("speech", (0, F // 2))]


@pytest.mark.parametrize("F,band", ENGINE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_engine_band_sums_and_tap_against_float64_of_the_denoised_samples(gpu_ctx, pkg, F, band):
    # 1024 points: 11..43 is vadfft1024_band_kernel<11, 43>, 5..30 and 1..47 its run-time form <0, 0>, 0..43 and 11..48
    # vadfft_jobs_kernel<8>; the tap is vadfft_jobs_kernel's everywhere; other sizes: vadfft_jobs_kernel<R> or rfft_generic_kernel
    lo, hi = k4.speech_band(F) if band == "speech" else band
    lanes = []
    for i, n_ch in enumerate((7, 3, 1)):        # ragged: a lane's last group of four frames is partial
        pcm, _ = pkg.synth.make_stream(n_ch * 0.5 + 0.1, seed=60 + i)
        lanes.append(pcm[0][: n_ch * 24000].copy())
    outs = gpu_ctx.engine_run(lanes, want_denoised=True, want_bins=True, fft_size=F, min_bin=lo, max_bin=hi)
    for x, o in zip(lanes, outs):
        nf = len(x) // F
        assert o["n_fft_frames"] == nf and o["denoised"].shape == (len(x),)
        frames = o["denoised"][:nf * F].reshape(nf, F)
        bins = k4.ref_bins(frames, F)
        wb, (fb, kb) = k4.bin_units(o["fft_bins"], bins)
        ws, (_, fs) = k4.band_units(o["band_sum"][None, :], bins, [(lo, hi)])
        print(f"\n    engine {F} points, band {lo}..{hi}, {nf} frames: tap {wb:.3g} units (tolerance {bin_tol(F):.3g}) at frame {fb} "
              f"bin {kb}; band sum {ws:.3g} units (tolerance {band_tol(F):.3g}) at frame {fs}")
        assert wb <= bin_tol(F), (F, wb, fb, kb)
        assert ws <= band_tol(F), (F, lo, hi, ws, fs)
        # the multi-band pass over the same samples: the engine's bits
        d = DeviceBands(gpu_ctx, o["denoised"][None, :], len(x), F, 2, band_stride=nf + 1)
        try:
            multi = check_rows(d.run([(lo, hi), (lo, hi)]), nf, bins, [(lo, hi), (lo, hi)], F, f"band_sums_device {F} points {lo}..{hi}")
        finally:
            d.close()
        assert np.array_equal(multi[0, 0].view(np.uint32), o["band_sum"].view(np.uint32)), (F, lo, hi)
        assert np.array_equal(multi[1, 0].view(np.uint32), o["band_sum"].view(np.uint32)), (F, lo, hi)


# ------------------------------------------------------------------ e. argument rules

@pytest.mark.parametrize("F", [1024, 1000])
def test_argument_rules(fv, gpu_ctx, F):
    frames, _ = k4.sweep_frames(F)
    m, h = 5, F // 2
    lanes, _ = lanes_from_table(frames, 2, m)
    d = DeviceBands(gpu_ctx, lanes, m * F, F, 2, lane_stride=m * F + 2, band_stride=m + 1, offset=2)
    ok = [(1, 20), (0, h)]
    try:
        assert d.raw(fv, ok, n_bands=0) == fv.FVAD_OK
        assert d.raw(fv, ok, n_lanes=0) == fv.FVAD_OK
        assert d.raw(fv, ok, lane_stride=m * F + 3) == fv.FVAD_ERR_INVALID_ARGUMENT       # odd lane stride
        assert d.raw(fv, ok, base=d.base + 4) == fv.FVAD_ERR_INVALID_ARGUMENT             # 4-byte aligned base
        assert d.raw(fv, ok, band_stride=m - 1) == fv.FVAD_ERR_INVALID_ARGUMENT
        assert d.raw(fv, [(1, 20), (10, h + 1)]) == fv.FVAD_ERR_OUT_OF_RANGE
        assert d.raw(fv, [(-1, 20), (0, h)]) == fv.FVAD_ERR_OUT_OF_RANGE
        assert d.raw(fv, [(1, 20), (21, 20)]) == fv.FVAD_ERR_OUT_OF_RANGE
        gpu_ctx.synchronize()
        assert (d.out() == CANARY).all()        # none of them wrote anything
        assert d.raw(fv, ok) == fv.FVAD_OK
        assert not (d.out()[:, :, :m] == CANARY).any()
    finally:
        d.close()
