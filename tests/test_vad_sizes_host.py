"""Sweeps over the FFT size on the host (fvad_vad_batch_create_sweep_sized, fvad_vad_batch_run_sized): machines of several frame
lengths in one batch, bit for bit what one fvad_vad_batch_create_sweep batch per size gives; the size-major band table; the
part rules in samples; the argument checks; simulator.expand_grid_sized and the sliced check over sizes.  No GPU needed."""
import ctypes as C
import json
import math

import numpy as np
import pytest

from test_vad_sweep_host import CHUNK, CONFIGS, FS

SIZES = [512, 1000, 1024, 2048]
N_CHUNKS = 64   # (32 s: every size's frames end on the last sample)


def synth_sized(n_streams, nch, n_chunks, bands, seed):
    """band sums [n_bands][lanes][stride] for bands [(F, lo, hi)] (stride: the frames of the smallest size) and chunk RMS
    [lanes][n_chunks]: bursts every band sees, a noise floor of its own, quiet channels for the channel ratio"""
    rng = np.random.default_rng(seed)
    lanes = n_streams * nch
    f_min = min(F for F, _, _ in bands)
    stride = n_chunks * CHUNK // f_min
    band = np.zeros((len(bands), lanes, stride), np.float32)
    rms = np.empty((lanes, n_chunks), np.float32)
    dur = n_chunks * CHUNK / FS
    for s in range(n_streams):
        ons = []
        x = rng.uniform(0, 2)
        while x < dur:
            d = rng.uniform(0.3, 3.0)
            ons.append((x, x + d))
            x += d + rng.uniform(0.5, 5.0)
        starts, ends = np.array([a for a, _ in ons]), np.array([b for _, b in ons])

        def inside(t):   # t inside a burst (the bursts do not overlap)
            k = np.searchsorted(starts, t, side="right") - 1
            return (k >= 0) & (t < ends[np.maximum(k, 0)])
        for c in range(nch):
            lane = s * nch + c
            gain = 1.0 if c == 0 else rng.uniform(0.3, 1.0)
            for j, (F, lo, hi) in enumerate(bands):
                nf = n_chunks * CHUNK // F
                on = inside(np.arange(nf) * F / FS)
                w = (hi - lo + 1) * F / 1024.0
                band[j, lane, :nf] = 1e-3 * w * rng.uniform(0.5, 2.0, nf) + on * w * rng.uniform(0.02, 0.2, nf) * gain
            on_c = inside((np.arange(n_chunks) + 0.5) * CHUNK / FS).astype(float)
            rms[lane] = (0.01 + 0.1 * gain * on_c) * rng.uniform(0.8, 1.2, n_chunks)
    return band, rms


def mixed_configs():
    """configs interleaving the sizes; configs 0 and 1 share their Hz edges at two sizes"""
    cfgs, sizes = [], []
    for i in range(8):
        cfgs.append(dict(CONFIGS[i % len(CONFIGS)]))
        sizes.append(SIZES[i % len(SIZES)])
    cfgs[1] = dict(cfgs[0])
    return cfgs, sizes


def results(sw, S, NC):
    return ([sw.segments(c) for c in range(NC)], [[sw.audit(s, c) for c in range(NC)] for s in range(S)],
            [[sw.lazy_stats(s, c) for c in range(NC)] for s in range(S)])


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist() if isinstance(x, (list, tuple)) else x


def seg_bits(segs):
    return [[[(a, b, np.float32(r).view(np.uint32).item(), np.float32(m).view(np.uint32).item()) for a, b, r, m in st] for st in c]
            for c in segs]


def per_size_reference(fv, cfgs, sizes, band, rms, bands_sized, S, nch, n_frames_of):
    """config c's results from a create_sweep batch at its size, fed the sized batch's band blocks of that size"""
    out = {}
    for F in sorted(set(sizes)):
        idx = [c for c in range(len(cfgs)) if sizes[c] == F]
        ref = fv.VadSweep(S, [cfgs[c] for c in idx], n_channels=nch, fft_size=F)
        try:
            rbins, _ = ref.bands()
            blocks = []
            for lo, hi in rbins:
                j = bands_sized.index((F, lo, hi))
                blocks.append(band[j, :, :n_frames_of(F)])
            ref.run(np.ascontiguousarray(np.stack(blocks)), rms, n_threads=4)
            segs, aud, lazy = results(ref, S, len(idx))
            for k, c in enumerate(idx):
                out[c] = (segs[k], [aud[s][k] for s in range(S)], [lazy[s][k] for s in range(S)])
        finally:
            ref.close()
    return out


@pytest.mark.parametrize("F", [1024, 1000])
def test_one_size_equals_create_sweep(fv, F):
    cfgs = [dict(c) for c in CONFIGS]
    S, nch = 3, 2
    a = fv.VadSweepSized(S, cfgs, [F] * len(cfgs), n_channels=nch)
    b = fv.VadSweep(S, cfgs, n_channels=nch, fft_size=F)
    try:
        bins_b, band_of_b = b.bands()
        bands_a, band_of_a = a.bands()
        assert bands_a == [(F, lo, hi) for lo, hi in bins_b] and band_of_a == band_of_b
        assert a.frame_sizes() == ([F], [0] * len(bins_b))
        band, rms = synth_sized(S, nch, N_CHUNKS, bands_a, 3)
        nf = N_CHUNKS * CHUNK // F
        band = np.ascontiguousarray(band[:, :, :nf])
        a.run(band, rms, [nf], n_threads=4)
        b.run(band, rms, n_threads=4)
        ra, rb = results(a, S, len(cfgs)), results(b, S, len(cfgs))
        assert seg_bits(ra[0]) == seg_bits(rb[0])
        assert [[bits(x) for x in row] for row in ra[1]] == [[bits(x) for x in row] for row in rb[1]]
        assert ra[2] == rb[2]
        # the host scorer's statistics, as uint32
        rng = np.random.default_rng(1)
        refs = [[(float(x), float(x) + 1.5) for x in np.sort(rng.uniform(0, 18, 4))] for _ in range(S)]
        for sw in (a, b):
            sw.set_references(refs, {"ignore_shorter_than_sec": 0.5, "extrude_start": 1.0, "extrude_end": 1.0, "fill_gaps": 0.5})
            sw.score(4)
        for c in range(len(cfgs)):
            assert np.array_equal(a.config_stats(c).view(np.uint32), b.config_stats(c).view(np.uint32))
        # the old run call takes a one-size sized batch
        assert fv.lib().fvad_vad_batch_run(a.h, fv.fptr(band), nf, nf, fv.fptr(rms), N_CHUNKS, N_CHUNKS, CHUNK, 2) == 0
        assert seg_bits(results(a, S, len(cfgs))[0]) == seg_bits(rb[0])
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("F", [512, 1024, 960])
def test_create_sweep_batch_on_the_sized_surface(fv, F):
    """a create_sweep batch reports its one size and its band blocks, follows a retain, and takes run_sized in parts from
    first_sample, bit for bit its own run in one call"""
    cfgs = [dict(CONFIGS[0]), dict(CONFIGS[1]), dict(CONFIGS[3])]   # two distinct bands: configs 0 and 2 share the default one
    S, nch, n_chunks = 1, 2, 40
    one = fv.VadSweep(S, cfgs, n_channels=nch, fft_size=F)
    parts = fv.VadSweep(S, cfgs, n_channels=nch, fft_size=F)
    try:
        bins, band_of = parts.bands()
        assert len(bins) == 2 and band_of == [0, 1, 0]
        assert parts.sizes == [F] and parts.size_of_band == [0, 0]
        assert parts.frame_sizes() == ([F], [0, 0])
        assert parts.size_blocks() == [(F, 0, bins)]
        band, rms = synth_sized(S, nch, n_chunks, [(F, lo, hi) for lo, hi in bins], 17)
        nf = n_chunks * CHUNK // F
        assert band.shape[2] == nf
        one.run(band, rms, n_threads=2)
        for c0 in range(0, n_chunks, 16):   # (16 chunks are a whole number of frames at each size)
            c1 = min(c0 + 16, n_chunks)
            f0, f1 = c0 * CHUNK // F, min(c1 * CHUNK // F, nf)
            assert f0 * F == c0 * CHUNK
            parts.run_sized(np.ascontiguousarray(band[:, :, f0:f1]), np.ascontiguousarray(rms[:, c0:c1]), [f1 - f0],
                            first_sample=c0 * CHUNK, n_threads=2)
        ra, rb = results(parts, S, len(cfgs)), results(one, S, len(cfgs))
        assert seg_bits(ra[0]) == seg_bits(rb[0])
        assert [[bits(x) for x in row] for row in ra[1]] == [[bits(x) for x in row] for row in rb[1]]
        assert ra[2] == rb[2]
        assert any(len(st) for c in ra[0] for st in c)   # (the configs do decide something)
        # one band of one mono stream cut out of a wider array: numpy keeps the old strides on the axes of length 1
        mono = fv.VadSweep(1, [cfgs[0]], fft_size=F)
        ref1 = fv.VadSweep(1, [cfgs[0]], fft_size=F)
        try:
            cut = np.ascontiguousarray(band[:1, 1:2, :nf - 3])
            mono.run_sized(cut, np.ascontiguousarray(rms[1:2]), nf - 3)
            ref1.run(cut.copy(), np.ascontiguousarray(rms[1:2]))
            assert seg_bits(results(mono, 1, 1)[0]) == seg_bits(results(ref1, 1, 1)[0]) and results(mono, 1, 1)[1:] == results(ref1, 1, 1)[1:]
        finally:
            mono.close()
            ref1.close()
        # a retain that drops config 1 drops its band
        parts.retain(None, [0, 2])
        assert parts.bands() == ([bins[0]], [0, 0])
        assert parts.sizes == [F] and parts.size_of_band == [0]
        assert parts.size_blocks() == [(F, 0, [bins[0]])]
    finally:
        one.close()
        parts.close()


def test_mixed_sizes_equal_per_size_batches(fv):
    cfgs, sizes = mixed_configs()
    S, nch = 2, 2
    sw = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    try:
        bands, band_of = sw.bands()
        band, rms = synth_sized(S, nch, N_CHUNKS, bands, 7)
        nfs = [N_CHUNKS * CHUNK // F for F in sw.sizes]
        sw.run(band, rms, nfs, n_threads=4)
        got = results(sw, S, len(cfgs))
        want = per_size_reference(fv, cfgs, sizes, band, rms, bands, S, nch, lambda F: N_CHUNKS * CHUNK // F)
        for c in range(len(cfgs)):
            assert seg_bits([got[0][c]]) == seg_bits([want[c][0]]), c
            assert [bits(got[1][s][c]) for s in range(S)] == [bits(x) for x in want[c][1]], c
            assert [got[2][s][c] for s in range(S)] == want[c][2], c
        assert any(len(st) for c in range(len(cfgs)) for st in got[0][c])   # (the configs do decide something)
    finally:
        sw.close()


def test_parts_equal_one_call_and_part_rules(fv):
    cfgs, sizes = mixed_configs()
    S, nch = 2, 1
    one = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    parts = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    try:
        bands, _ = one.bands()
        band, rms = synth_sized(S, nch, N_CHUNKS, bands, 11)
        one.run(band, rms, [N_CHUNKS * CHUNK // F for F in one.sizes], n_threads=4)
        # parts on the lcm grid of chunk and every size: 24000 * lcm(slice_align) samples
        align = math.lcm(*[math.lcm(CHUNK, F) // CHUNK for F in sizes])
        assert align == 32   # (512: 8 chunks, 1000: 1, 1024: 16, 2048: 32)
        bounds = [0, 32, N_CHUNKS]
        for c0, c1 in zip(bounds[:-1], bounds[1:]):
            s0 = c0 * CHUNK
            nf = [(c1 * CHUNK) // F - s0 // F for F in parts.sizes]
            w = max(nf)
            part = np.ascontiguousarray(np.stack([band[j, :, s0 // bands[j][0]:s0 // bands[j][0] + w] for j in range(len(bands))]))
            assert part.shape[2] == w
            parts.run(part, np.ascontiguousarray(rms[:, c0:c1]), nf, first_sample=s0, n_threads=4)
        assert seg_bits(results(parts, S, len(cfgs))[0]) == seg_bits(results(one, S, len(cfgs))[0])
        assert results(parts, S, len(cfgs))[1:] == results(one, S, len(cfgs))[1:]
        lib = fv.lib()
        nf = (fv.sz * 4)(0, 0, 0, 0)
        z = np.zeros((len(bands), S * nch, 1), np.float32)
        r = np.zeros((S * nch, 1), np.float32)
        # a start on a chunk but not on a frame of every size (512 does not divide 24000)
        assert lib.fvad_vad_batch_run_sized(parts.h, fv.fptr(z), 1, nf, fv.fptr(r), 1, 1, CHUNK, CHUNK, 1) == fv.FVAD_ERR_INVALID_ARGUMENT
        # a start on the grid but not where the last part ended
        assert lib.fvad_vad_batch_run_sized(parts.h, fv.fptr(z), 1, nf, fv.fptr(r), 1, 1, CHUNK, 32 * CHUNK, 1) == fv.FVAD_ERR_INVALID_ARGUMENT
        # a start off the chunk grid
        assert lib.fvad_vad_batch_run_sized(parts.h, fv.fptr(z), 1, nf, fv.fptr(r), 1, 1, CHUNK, 1024000, 1) == fv.FVAD_ERR_INVALID_ARGUMENT
        # where the last part ended: accepted
        assert lib.fvad_vad_batch_run_sized(parts.h, fv.fptr(z), 1, nf, fv.fptr(r), 1, 0, CHUNK, N_CHUNKS * CHUNK, 1) == 0
        # a part after which the sizes end apart is the last
        nf1 = (fv.sz * 4)(1, 0, 0, 0)
        assert lib.fvad_vad_batch_run_sized(parts.h, fv.fptr(z), 1, nf1, fv.fptr(r), 1, 1, CHUNK, N_CHUNKS * CHUNK, 1) == 0
        for s0 in (N_CHUNKS * CHUNK, (N_CHUNKS + 32) * CHUNK):
            assert lib.fvad_vad_batch_run_sized(parts.h, fv.fptr(z), 1, nf, fv.fptr(r), 1, 0, CHUNK, s0, 1) == fv.FVAD_ERR_INVALID_ARGUMENT
    finally:
        one.close()
        parts.close()


def test_band_order_and_bins(fv):
    from test_vad_sweep_host import freq_to_bin   # (at 1024 points)
    cfgs = [{"speech_min_freq": 300.0, "speech_max_freq": 3400.0}, {}, {"speech_min_freq": 300.0, "speech_max_freq": 3400.0},
            {}, {"speech_min_freq": 1000.0, "speech_max_freq": 4000.0}]
    sizes = [2048, 512, 512, 2048, 1024]
    sw = fv.VadSweepSized(1, cfgs, sizes)
    try:
        bands, band_of = sw.bands()
        assert sw.sizes == [2048, 512, 1024]

        def fb(f, F):   # FFT.freqToBin in f32 at size F
            x = float(np.float32(f) / np.float32(np.float32(FS) / np.float32(F)))
            return int(math.floor(x + 0.5))
        want = [(2048, fb(300, 2048), fb(3400, 2048)), (2048, fb(500, 2048), fb(2000, 2048)),
                (512, fb(500, 512), fb(2000, 512)), (512, fb(300, 512), fb(3400, 512)),
                (1024, freq_to_bin(1000.0), freq_to_bin(4000.0))]
        assert bands == want
        assert band_of == [0, 2, 3, 1, 4]
        assert sw.frame_sizes() == ([2048, 512, 1024], [0, 0, 1, 1, 2])
        # the same Hz edges at two sizes are two bands
        assert bands[1][1:] != bands[2][1:]
    finally:
        sw.close()


def _create_sized(fv, cfgs, sizes, n_channels=1, n_streams=1):
    arr = (fv.VadConfig * len(cfgs))()
    for i, ov in enumerate(cfgs):
        fv.lib().fvad_vad_config_default(C.byref(arr[i]))
        for k, v in ov.items():
            setattr(arr[i], k, v)
    h = fv.vp()
    rc = fv.lib().fvad_vad_batch_create_sweep_sized(arr, (fv.sz * len(sizes))(*sizes), len(cfgs), FS, n_channels, n_streams, C.byref(h))
    if rc == 0:
        fv.lib().fvad_vad_batch_destroy(h)
    return rc


def _create_single(fv, cfg, F):
    c = fv.VadConfig()
    fv.lib().fvad_vad_config_default(C.byref(c))
    for k, v in cfg.items():
        setattr(c, k, v)
    h = fv.vp()
    rc = fv.lib().fvad_vad_create(C.byref(c), FS, 1, F, C.byref(h))
    if rc == 0:
        fv.lib().fvad_vad_destroy(h)
    return rc


def test_each_config_checked_at_its_own_size(fv):
    # a channel-ratio window of 0.2 s: 18 frames at 512 points, 0 at 16384 (48000 / 16384 * 0.2 = 0.58)
    cfg = {"channel_vol_ratio_avg_sec": 0.2}
    assert _create_single(fv, cfg, 512) == 0
    want = _create_single(fv, cfg, 16384)
    assert want != 0
    assert _create_sized(fv, [cfg, {}], [512, 1024]) == 0
    assert _create_sized(fv, [{}, cfg], [512, 16384]) == want
    # a band above Nyquist is the same at every size; a band whose bins cross at one size only
    assert _create_sized(fv, [{"speech_max_freq": 30000.0}], [1024]) == fv.FVAD_ERR_OUT_OF_RANGE
    assert _create_sized(fv, [{"speech_min_freq": -1.0}], [2048]) == fv.FVAD_ERR_NEGATIVE_FREQUENCY


def test_size_and_call_checks(fv):
    for bad in (0, 1, 2, 3, 1023, 16386, 32768):
        assert _create_sized(fv, [{}, {}], [1024, bad]) == fv.FVAD_ERR_INVALID_ARGUMENT, bad
    for good in (4, 16384, 1000):
        assert _create_sized(fv, [{"speech_min_freq": 0.0, "speech_max_freq": 0.0, "channel_vol_ratio_avg_sec": 1000.0}], [good]) == 0
    cfgs, sizes = mixed_configs()
    sw = fv.VadSweepSized(2, cfgs, sizes)
    lib = fv.lib()
    try:
        band = np.zeros((len(sw.bands()[0]), 2, 375), np.float32)
        r = np.zeros((2, 16), np.float32)
        nf = (fv.sz * 2)(0, 0)
        # the single-size run calls refuse several sizes
        assert lib.fvad_vad_batch_run(sw.h, fv.fptr(band), 375, 375, fv.fptr(r), 16, 16, CHUNK, 1) == fv.FVAD_ERR_INVALID_ARGUMENT
        assert lib.fvad_vad_batch_run_part(sw.h, fv.fptr(band), 375, 375, fv.fptr(r), 16, 16, CHUNK, 0, 1) == fv.FVAD_ERR_INVALID_ARGUMENT
        import torch
        if not torch.cuda.is_available():
            assert lib.fvad_vad_batch_run_device(None, sw.h, None, 1, nf, fv.fptr(r), 1, nf, CHUNK) == fv.FVAD_ERR_NO_DEVICE
            nf8 = (fv.sz * 8)()
            assert lib.fvad_vad_batch_run_device_sized(None, sw.h, None, 1, nf8, fv.fptr(r), 1, nf, CHUNK) == fv.FVAD_ERR_NO_DEVICE
            assert lib.fvad_vad_batch_run_device_part_sized(None, sw.h, None, 1, nf8, fv.fptr(r), 1, nf, CHUNK, 0) == fv.FVAD_ERR_NO_DEVICE
        # band_stride below a size's frame count
        nf4 = (fv.sz * 4)(375, 0, 0, 0)
        assert lib.fvad_vad_batch_run_sized(sw.h, fv.fptr(band), 374, nf4, fv.fptr(r), 16, 16, CHUNK, 0, 1) == fv.FVAD_ERR_INVALID_ARGUMENT
        # a frame without its chunk's ratio (16 chunks hold 750 frames of 512)
        nf4 = (fv.sz * 4)(751, 0, 0, 0)
        big = np.zeros((band.shape[0], 2, 751), np.float32)
        assert lib.fvad_vad_batch_run_sized(sw.h, fv.fptr(big), 751, nf4, fv.fptr(r), 16, 16, CHUNK, 0, 1) == fv.FVAD_ERR_INVALID_ARGUMENT
    finally:
        sw.close()
    # the new run call takes a create_sweep batch, bit for bit its own run
    a = fv.VadSweep(1, CONFIGS[:3])
    b = fv.VadSweep(1, CONFIGS[:3])
    try:
        bins, _ = a.bands()
        band, rms = synth_sized(1, 1, 16, [(1024, lo, hi) for lo, hi in bins], 2)
        a.run(band, rms)
        assert lib.fvad_vad_batch_run_sized(b.h, fv.fptr(band), band.shape[2], (fv.sz * 1)(band.shape[2]), fv.fptr(rms), 16, 16, CHUNK, 0, 1) == 0
        assert seg_bits(results(a, 1, 3)[0]) == seg_bits(results(b, 1, 3)[0]) and results(a, 1, 3)[1:] == results(b, 1, 3)[1:]
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ the grid
@pytest.fixture(scope="module")
def sim(pkg):
    return pkg.simulator


def test_expand_grid_sized_order_and_counts(sim):
    grid = {"base": {"speech_threshold_factor": 3}, "axes": {"max_speech_gap_sec": [1, 2], "speech_min_freq": [300, 400, 500]}}
    base = sim.expand_grid(grid)
    assert sim.expand_grid_sized(grid, 1024) == ([1024] * 6, base)
    sizes, cfgs = sim.expand_grid_sized(dict(grid, fft_size=[2048, 512]), 1024)
    assert sizes == [2048] * 6 + [512] * 6 and cfgs == base + base
    sizes, cfgs = sim.expand_grid_sized({"fft_size": [1000]}, 1024)
    assert sizes == [1000] and cfgs == [{}]
    # the product counts against GRID_MAX_CONFIGS
    n = sim.GRID_MAX_CONFIGS // 2
    g = {"axes": {"speech_threshold_factor": list(range(n))}, "fft_size": [512, 1024]}
    assert len(sim.expand_grid_sized(g, 1024)[1]) == 2 * n
    with pytest.raises(ValueError, match="GRID_MAX_CONFIGS"):
        sim.expand_grid_sized(dict(g, fft_size=[512, 1024, 2048]), 1024)


BAD_SIZED = [({"fft_size": []}, "non-empty"), ({"fft_size": 1024}, "non-empty"), ({"fft_size": [1024, 1023]}, "even"),
             ({"fft_size": [2]}, "even"), ({"fft_size": [16386]}, "even"), ({"fft_size": [1024.0]}, "even"),
             ({"fft_size": [True]}, "even"), ({"fft_size": [512, 1024, 512]}, "twice"),
             ({"fft_size": [512], "base": {"fft_size": 1024}}, "valid fields"),
             ({"fft_size": [512], "axes": {"fft_size": [1024]}}, "valid fields")]


@pytest.mark.parametrize("grid,words", BAD_SIZED)
def test_sized_grid_errors_before_any_gpu_work(sim, tmp_path, grid, words):
    with pytest.raises(ValueError, match=words):
        sim.expand_grid_sized(grid, 1024)
    (tmp_path / "grid.json").write_text(json.dumps(grid))
    with pytest.raises(ValueError, match=words):   # (the plan does not exist: the grid is refused first)
        sim.run_grid(str(tmp_path / "missing-plan.json"), str(tmp_path / "grid.json"), out=None)
    # fft_size inside base or axes keeps expand_grid's message
    with pytest.raises(ValueError) as e:
        sim.expand_grid({"axes": {"fft_size": [512]}})
    assert "fft_size" in str(e.value) and "valid fields" in str(e.value)


def test_sliced_check_over_sizes(sim, fv, tmp_path):
    assert math.lcm(sim.slice_align(512), sim.slice_align(2048)) == 32
    for n in (16, 8, 48, 0, -32, True):
        with pytest.raises(ValueError, match=r"\[512, 2048\]"):
            sim.check_slice_chunks_sized(n, [2048, 512])
    for n in (32, 64):
        sim.check_slice_chunks_sized(n, [2048, 512])
    sim.check_slice_chunks_sized(16, [1024])
    with pytest.raises(ValueError):
        sim.check_slice_chunks_sized(8, [1024])
    # run_grid refuses the slice before any GPU work (no device here: reaching it would raise FVAD_ERR_NO_DEVICE instead)
    pcm = np.zeros((1, 3 * CHUNK), np.float32)
    fv.wav_write(str(tmp_path / "a.wav"), pcm)
    (tmp_path / "a.txt").write_text("0.5\t1.0\tspeech\n")
    plan = {"instances": [{"name": "a", "audio_path": "a.wav", "ref_path": "a.txt"}], "config": {"vad_config": {"fft_size": 1024}}}
    (tmp_path / "plan.json").write_text(json.dumps(plan))
    with pytest.raises(ValueError, match=r"slice_chunks.*\[512, 2048\]"):
        sim.run_grid(str(tmp_path / "plan.json"), {"axes": {"speech_threshold_factor": [3.0]}, "fft_size": [512, 2048]},
                     slice_chunks=16, out=None)
