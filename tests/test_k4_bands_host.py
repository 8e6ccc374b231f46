"""K4's yardstick, checked on the CPU: the float64 reference of k4_cases against the analytic Hann spectrum, the oracle's band
edges, the input builders' conditions, and the oracle's own distance from the reference over the whole case table -- the
constants from which the GPU tolerance of test_k4_bands_gpu.py derives."""
import numpy as np
import pytest

import k4_cases as k4
import orc


@pytest.mark.parametrize("F", [32, 254, 1000, 1024, 6250])
def test_ref_bins_match_the_analytic_hann_spectrum_of_integer_bin_tones(F):
    # A sin(2 pi k n / F + phi) under the periodic Hann window 1/2 - 1/2 cos(2 pi n / F): |X| = A F / 4 at k and A F / 8 at
    # k - 1 and k + 1, nothing elsewhere; norm = 1 / sum(w) = 2 / F turns that into A / 2 and A / 4.  (2 <= k <= F/2 - 2: the
    # images at -k and F - k stay clear of the three bins.)  The f32 window and the f32 samples differ from the ideal ones by
    # 2^-24 relative each: 1e-6 of A holds with room.
    h = F // 2
    for i, k in enumerate(sorted({2, 3, 7, h // 3, h // 2, h - 3, h - 2})):
        if not 2 <= k <= h - 2:
            continue
        A = k4.TONE_AMPS[i % len(k4.TONE_AMPS)]
        bins = k4.ref_bins(k4.one_hot_tone(F, k, i), F)
        want = np.zeros(h + 1)
        want[k - 1], want[k], want[k + 1] = A / 4, A / 2, A / 4
        assert np.abs(bins - want).max() <= 1e-6 * A, (F, k, A, np.abs(bins - want).max())
        assert abs(k4.ref_band(bins, k - 1, k + 1) - A) <= 3e-6 * A


def test_ref_bins_dc_and_nyquist_and_norm():
    for F in (4, 6, 1024, 16384):
        w, norm = k4.window_and_norm(F)
        assert abs(float(norm) * F / 2 - 1.0) < 1e-6        # sum(w) = F / 2
        dc = k4.ref_bins(np.full(F, 0.5, np.float32), F)
        assert abs(dc[0] - 0.5) < 1e-6 and abs(dc[1] - 0.25) < 1e-6 and (F < 8 or dc[2:].max() < 1e-6)
        ny = k4.ref_bins((0.5 * (1.0 - 2.0 * (np.arange(F) % 2))).astype(np.float32), F)
        assert abs(ny[F // 2] - 0.5) < 1e-6 and abs(ny[F // 2 - 1] - 0.25) < 1e-6


def test_oracle_bands_at_the_default_config():
    assert k4.speech_band(1024) == (11, 43)                 # VADMachine.zig:146-151 at 48 kHz
    assert k4.speech_band(512) == (5, 21) and k4.speech_band(2048) == (21, 85)
    assert (11, 43) in k4.band_set(1024)
    for b in k4.PRUNED_EDGES + k4.PRUNED_NEIGHBOURS:
        assert b in k4.band_set(1024)


@pytest.mark.parametrize("F", k4.SIZES)
def test_input_builders_meet_their_conditions(F):
    frames, labels = k4.frame_table(F)
    h = F // 2
    assert frames.dtype == np.float32 and frames.shape == (len(labels), F)
    # deterministic
    assert np.array_equal(frames, k4.frame_table(F)[0])
    # amplitudes at or above 1e-9 (silence apart), below f32 trouble
    peak = np.abs(frames).max(axis=1)
    assert labels.count("silence") == 1 and peak[labels.index("silence")] == 0.0
    assert all(p >= 0.99e-9 for p, l in zip(peak, labels) if l != "silence") and peak.max() <= 1.0
    # |X|^2 of every significant bin inside normal f32
    assert k4.significant_bins_normal(frames, F) == []
    # only the silence frame has an all-zero spectrum
    bins = k4.ref_bins(frames, F)
    assert [l for l, b in zip(labels, bins) if not b.any()] == ["silence"]
    # the tones walk the bins the issue names, and every walked bin has its single-bin band
    tb = k4.tone_bins(F)
    if F <= 1024:
        assert tb == list(range(h + 1))
    else:
        assert set(range(50)) <= set(tb) and {h - 2, h - 1, h} <= set(tb) and len([k for k in tb if 50 <= k < h - 2]) >= 8
    bands = k4.band_set(F)
    assert all((k, k) in bands for k in tb) and {(0, 0), (0, h), (h, h)} <= set(bands)
    assert len(bands) > len(set(bands))                     # duplicates
    assert all(0 <= lo <= hi <= h for lo, hi in bands)
    # each tone is loudest in its own bin
    for k in tb:
        assert int(np.argmax(bins[labels.index(f"tone {k}")])) == k
    for count in k4.BAND_COUNTS:
        cb = k4.cycled_bands(F, count)
        assert len(cb) == count and all(0 <= lo <= hi <= h for lo, hi in cb)
    if F == 1024:
        for count in k4.BAND_COUNTS:
            cb = k4.cycled_bands(F, count, pruned_only=True)
            assert len(cb) == count and all(1 <= lo <= hi <= 47 for lo, hi in cb)
            mixed = k4.cycled_bands(F, count)
            assert count < 8 or (any(lo >= 1 and hi <= 47 for lo, hi in mixed) and any(lo < 1 or hi > 47 for lo, hi in mixed))
        assert len(set(k4.cycled_bands(F, 600))) < 600 and len(set(k4.cycled_bands(F, 600))) > 40


def test_metric_refuses_what_it_must():
    F = 1024
    frames, _ = k4.sweep_frames(F)
    bins = k4.ref_bins(frames, F)
    bands = [(11, 43), (16, 16), (0, 512)]
    exact = np.stack([k4.ref_band(bins, lo, hi) for lo, hi in bands]).astype(np.float32)
    assert k4.band_units(exact, bins, bands)[0] <= 1.0      # the reference rounded to f32: half an ulp of the sum
    off = np.stack([k4.ref_band(bins, lo, hi - 1) for lo, hi in bands]).astype(np.float32)      # hi taken as exclusive
    assert k4.band_units(off, bins, bands)[0] > 1e3
    silent = [i for i, b in enumerate(bins) if not b.any()]
    neg = exact.copy()
    neg[:, silent] = -0.0
    assert k4.band_units(neg, bins, bands)[0] == np.inf     # silence is +0.0 exactly
    nan = exact.copy()
    nan[1, 0] = np.nan
    assert k4.band_units(nan, bins, bands)[0] == np.inf
    assert k4.bin_units(bins.astype(np.float32), bins)[0] <= 1.0
    shifted = np.roll(bins, 1, axis=1).astype(np.float32)
    assert k4.bin_units(shifted, bins)[0] > 1e3


@pytest.mark.parametrize("F", k4.SIZES)
def test_oracle_stays_inside_the_recorded_constants(F, capsys):
    # the whole table, no case left out: every frame of frame_table(F), every bin, every band of band_set(F)
    frames, labels = k4.frame_table(F)
    bands = k4.band_set(F)
    bins = k4.ref_bins(frames, F)
    ob = k4.oracle_bins(frames, F)
    wb, (fb, kb) = k4.bin_units(ob, bins)
    ws, (js, fs) = k4.band_units(k4.oracle_bands(ob, bands), bins, bands)
    with capsys.disabled():
        print(f"\n    {F}: bins {wb:.3g} ({labels[fb]}, bin {kb}); bands {ws:.3g} ({labels[fs]}, band {bands[js]}); "
              f"{len(labels)} frames, {len(bands)} bands")
    assert wb <= k4.ORACLE_BIN_UNITS[F], (F, wb, labels[fb], kb)
    assert ws <= k4.ORACLE_BAND_UNITS[F], (F, ws, labels[fs], bands[js])
    # the constants are measurements, not allowances: the oracle reaches at least a third of each
    assert wb >= k4.ORACLE_BIN_UNITS[F] / 3 and ws >= k4.ORACLE_BAND_UNITS[F] / 3
    # far below what an indexing or twiddle mistake costs, GPU factor included
    assert k4.GPU_FACTOR * max(k4.ORACLE_BIN_UNITS[F], k4.ORACLE_BAND_UNITS[F]) < 1e3
