"""Parameter sweeps on the host (fvad_vad_batch_create_sweep): one VAD machine per (stream, config), each on its own speech
band, bit for bit what one fvad_vad_batch per config gives; the band table; the configs' argument checks.  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

FS, FFT, CHUNK = 48000, 1024, 24000


def synth_inputs(n_streams, n_channels, n_chunks, bands, seed):
    """band sums [n_bands][lanes][n_frames] and chunk RMS [lanes][n_chunks]: a noise floor with speech-like bursts (0.3 .. 4 s
    on, 0.5 .. 6 s off) that every band sees with its own gain, a few quiet channels so that the channel ratio moves too"""
    rng = np.random.default_rng(seed)
    n_frames = n_chunks * CHUNK // FFT
    lanes = n_streams * n_channels
    t = np.arange(n_frames) * FFT / FS
    band = np.empty((len(bands), lanes, n_frames), np.float32)
    rms = np.empty((lanes, n_chunks), np.float32)
    for s in range(n_streams):
        on = np.zeros(n_frames, bool)
        x = rng.uniform(0, 3)
        while x < t[-1]:
            d = rng.uniform(0.3, 4.0)
            on |= (t >= x) & (t < x + d)
            x += d + rng.uniform(0.5, 6.0)
        for c in range(n_channels):
            lane = s * n_channels + c
            gain = 1.0 if c == 0 else rng.uniform(0.3, 1.0)
            for j, (lo, hi) in enumerate(bands):
                floor = 1e-3 * (hi - lo + 1) * rng.uniform(0.5, 2.0, n_frames)
                burst = on * (hi - lo + 1) * rng.uniform(0.02, 0.2, n_frames) * gain
                band[j, lane] = floor + burst
            tc = (np.arange(n_chunks) + 0.5) * CHUNK / FS
            rms[lane] = (0.01 + 0.1 * gain * np.interp(tc, t, on.astype(float))) * rng.uniform(0.8, 1.2, n_chunks)
    return band, rms


def freq_to_bin(f):  # FFT.freqToBin: roundf (half away from zero) of f / (48000 / 1024) in f32
    x = float(np.float32(f) / np.float32(np.float32(FS) / np.float32(FFT)))
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


CONFIGS = [
    {},  # the defaults: 500-2000 Hz, 180 s long-term average from 0.005
    {"speech_min_freq": 300.0, "speech_max_freq": 3400.0, "long_term_speech_avg_sec": 8.0, "has_initial_long_term_avg": 0,
     "speech_threshold_factor": 4.0},
    {"speech_min_freq": 492.1875, "speech_max_freq": 1500.0, "long_term_speech_avg_sec": 12.0, "initial_long_term_avg": 0.02,
     "short_term_speech_avg_sec": 0.5, "speech_threshold_factor": 3.0},
    {"long_term_speech_avg_sec": 6.0, "has_initial_long_term_avg": 0, "short_term_speech_avg_sec": 0.1, "speech_threshold_factor": 2.5,
     "channel_vol_ratio_avg_sec": 1.0, "channel_vol_ratio_threshold": 0.3},
    {"speech_min_freq": 300.0, "speech_max_freq": 3400.0, "long_term_speech_avg_sec": 20.0, "initial_long_term_avg": 0.3, "speech_threshold_factor": 5.0,
     "min_consecutive_sec_to_open": 0.0, "max_speech_gap_sec": 0.5, "min_vad_duration_sec": 0.2},
    {"speech_min_freq": 1000.0, "speech_max_freq": 4000.0, "long_term_speech_avg_sec": 10.0, "has_initial_long_term_avg": 0,
     "speech_threshold_factor": 3.0, "max_speech_gap_sec": 1.0, "min_vad_duration_sec": 0.4},
    {"speech_min_freq": 1000.0, "speech_max_freq": 4000.0, "long_term_speech_avg_sec": 30.0, "initial_long_term_avg": 0.5,
     "speech_threshold_factor": 6.0, "channel_vol_ratio_threshold": 0.2},
    {"long_term_speech_avg_sec": 4.0, "initial_long_term_avg": 0.5, "short_term_speech_avg_sec": 0.3, "speech_threshold_factor": 2.0,
     "min_consecutive_sec_to_open": 0.5, "max_speech_gap_sec": 3.0, "min_vad_duration_sec": 1.0},
    {"speech_min_freq": 300.0, "speech_max_freq": 3400.0, "long_term_speech_avg_sec": 5.0, "has_initial_long_term_avg": 0,
     "short_term_speech_avg_sec": 0.05, "speech_threshold_factor": 1.5, "channel_vol_ratio_avg_sec": 0.1,
     "min_consecutive_sec_to_open": 0.0, "max_speech_gap_sec": 0.0, "min_vad_duration_sec": 0.0},
    {"speech_min_freq": 492.1875, "speech_max_freq": 1500.0, "long_term_speech_avg_sec": 15.0, "speech_threshold_factor": 8.0,
     "channel_vol_ratio_avg_sec": 2.0, "channel_vol_ratio_threshold": 0.6},
    {"speech_min_freq": 0.0, "speech_max_freq": 24000.0, "long_term_speech_avg_sec": 9.0, "has_initial_long_term_avg": 0,
     "speech_threshold_factor": 2.0},
    {"long_term_speech_avg_sec": 3.0, "initial_long_term_avg": 1.0, "speech_threshold_factor": 3.5, "min_vad_duration_sec": 0.3},
]


def config_bins(cfg):
    return freq_to_bin(cfg.get("speech_min_freq", 500.0)), freq_to_bin(cfg.get("speech_max_freq", 2000.0))


def test_sweep_batch_equals_one_batch_per_config(fv):
    n_streams, nch, n_chunks = 3, 2, 200
    sw = fv.VadSweep(n_streams, CONFIGS, n_channels=nch)
    bins, band_of = sw.bands()
    assert len(bins) >= 3
    band, rms = synth_inputs(n_streams, nch, n_chunks, bins, seed=5)
    sw.run(band, rms, n_threads=4)
    for c, cfg in enumerate(CONFIGS):
        one = fv.VadBatch(n_streams, n_channels=nch, overrides=cfg)
        want = one.run(np.ascontiguousarray(band[band_of[c]]), rms, n_threads=2)
        got = sw.segments(c)
        assert got == want, f"config {c}"
        assert all(len(w) > 0 for w in want), f"config {c} closes no segment in some stream"
        for s in range(n_streams):
            assert sw.audit(s, c) == one.audit(s), (c, s)
        one.close()
    # the plain accessors are config 0's
    offs = (fv.sz * (n_streams + 1))()
    n = fv.lib().fvad_vad_batch_total_segments(sw.h)
    arr = (fv.SpeechSegment * max(n, 1))()
    assert fv.lib().fvad_vad_batch_segments(sw.h, arr, max(n, 1), offs) == 0
    assert n == sum(len(x) for x in sw.segments(0))
    a = fv.VadAudit()
    assert fv.lib().fvad_vad_batch_audit(sw.h, 1, C.byref(a)) == 0
    assert (a.min_rel_threshold_margin, a.min_abs_ratio_margin, a.n_frames) == sw.audit(1, 0)
    sw.close()


def test_sweep_in_parts_equals_one_run(fv):
    n_streams, nch, n_chunks = 2, 2, 96
    cfgs = CONFIGS[1:6]
    whole = fv.VadSweep(n_streams, cfgs, n_channels=nch)
    bins, _ = whole.bands()
    band, rms = synth_inputs(n_streams, nch, n_chunks, bins, seed=11)
    whole.run(band, rms)
    parts = fv.VadSweep(n_streams, cfgs, n_channels=nch)
    # a part ends on a chunk boundary: 375 frames = 16 chunks; band blocks keep their [n_bands][lanes] layout (stride = full length)
    nf = band.shape[2]
    for f0 in range(0, nf, 750):
        f1 = min(nf, f0 + 750)
        c0 = f0 * FFT // CHUNK
        bp = band[:, :, f0:]
        st = fv.lib().fvad_vad_batch_run_part(parts.h, bp.ctypes.data_as(fv.c_float_p), nf, f1 - f0,
                                             rms[:, c0:].ctypes.data_as(fv.c_float_p), n_chunks, n_chunks - c0, CHUNK, f0, 2)
        assert st == 0
    for c in range(len(cfgs)):
        assert parts.segments(c) == whole.segments(c)
        for s in range(n_streams):
            assert parts.audit(s, c) == whole.audit(s, c)


def test_bands_dedup_order_and_rounding(fv):
    cfgs = [{"speech_min_freq": 1000.0, "speech_max_freq": 4000.0}, {}, {"speech_min_freq": 492.1875, "speech_max_freq": 2000.0},
            {"speech_min_freq": 1000.0, "speech_max_freq": 4000.0, "speech_threshold_factor": 3.0}, {"speech_threshold_factor": 4.0},
            {"speech_min_freq": 491.0, "speech_max_freq": 2000.0}, {"speech_min_freq": 23.4375, "speech_max_freq": 24000.0}]
    sw = fv.VadSweep(1, cfgs)
    bins, band_of = sw.bands()
    # 492.1875 Hz is bin 10.5: FFT.freqToBin's @round goes away from zero (11), round-half-even would say 10
    want_bins, want_of = [], []
    for c in cfgs:
        b = config_bins(c)
        if b not in want_bins:
            want_bins.append(b)
        want_of.append(want_bins.index(b))
    assert bins == want_bins and band_of == want_of
    assert bins == [(21, 85), (11, 43), (10, 43), (1, 512)] and band_of == [0, 1, 1, 0, 1, 2, 3]
    # a plain batch has one config, the band of its config
    plain = fv.VadBatch(1)
    assert fv.lib().fvad_vad_batch_n_configs(plain.h) == 1
    n = fv.sz()
    b2 = (C.c_int32 * 2)()
    assert fv.lib().fvad_vad_batch_bands(plain.h, b2, 1, C.byref(n), None) == 0 and n.value == 1 and list(b2) == [11, 43]
    # too small a buffer
    assert fv.lib().fvad_vad_batch_bands(sw.h, b2, 1, C.byref(n), None) == fv.FVAD_ERR_BUFFER_TOO_SMALL and n.value == 4


def _create(fv, cfgs):
    arr = (fv.VadConfig * len(cfgs))()
    for i, ov in enumerate(cfgs):
        fv.lib().fvad_vad_config_default(C.byref(arr[i]))
        for k, v in ov.items():
            setattr(arr[i], k, v)
    h = C.c_void_p()
    st = fv.lib().fvad_vad_batch_create_sweep(arr, len(cfgs), FS, 1, FFT, 1, C.byref(h))
    if st == 0:
        fv.lib().fvad_vad_batch_destroy(h)
    return st, arr


def test_config_errors_have_the_status_codes_of_the_single_machine(fv):
    bad = [({"speech_max_freq": 24001.0}, fv.FVAD_ERR_OUT_OF_RANGE),          # above Nyquist (fvad_pipeline_create)
           ({"speech_min_freq": 30000.0}, fv.FVAD_ERR_OUT_OF_RANGE),
           ({"speech_min_freq": -1.0}, fv.FVAD_ERR_NEGATIVE_FREQUENCY),        # negative edge
           ({"speech_min_freq": 3000.0, "speech_max_freq": 1000.0}, fv.FVAD_ERR_INVALID_ARGUMENT),  # max < min
           ({"channel_vol_ratio_avg_sec": 0.01}, fv.FVAD_ERR_INVALID_ARGUMENT)]  # ratio ring of length 0
    for ov, code in bad:
        st, arr = _create(fv, [{}, {"speech_threshold_factor": 3.0}, ov])
        assert st == code, (ov, st)
    # the ring check is fvad_vad_create's, with its code
    cfg = fv.VadConfig()
    fv.lib().fvad_vad_config_default(C.byref(cfg))
    cfg.channel_vol_ratio_avg_sec = 0.01
    h = C.c_void_p()
    assert fv.lib().fvad_vad_create(C.byref(cfg), FS, 1, FFT, C.byref(h)) == _create(fv, [{"channel_vol_ratio_avg_sec": 0.01}])[0]
    # no configs / no streams
    arr = (fv.VadConfig * 1)()
    fv.lib().fvad_vad_config_default(C.byref(arr[0]))
    assert fv.lib().fvad_vad_batch_create_sweep(arr, 0, FS, 1, FFT, 1, C.byref(h)) == fv.FVAD_ERR_INVALID_ARGUMENT
    assert fv.lib().fvad_vad_batch_create_sweep(arr, 1, FS, 1, FFT, 0, C.byref(h)) == fv.FVAD_ERR_INVALID_ARGUMENT
    # accessors past the configs
    sw = fv.VadSweep(2, [{}, {"speech_threshold_factor": 3.0}])
    a = fv.VadAudit()
    assert fv.lib().fvad_vad_batch_config_audit(sw.h, 0, 2, C.byref(a)) == fv.FVAD_ERR_INVALID_ARGUMENT
    assert fv.lib().fvad_vad_batch_config_audit(sw.h, 2, 0, C.byref(a)) == fv.FVAD_ERR_INVALID_ARGUMENT
    offs = (fv.sz * 3)()
    assert fv.lib().fvad_vad_batch_config_segments(sw.h, 2, None, 0, offs) == fv.FVAD_ERR_INVALID_ARGUMENT


def test_gpu_entry_points_without_a_device(fv):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    bins = (C.c_int32 * 2)(11, 43)
    assert fv.lib().fvad_engine_band_sums_device(None, None, 1, 1024, 1024, 1024, bins, 1, None, 1) == fv.FVAD_ERR_NO_DEVICE
    sw = fv.VadSweep(1, [{}, {"speech_threshold_factor": 3.0}])
    nf = (fv.sz * 1)(0)
    rms = np.zeros((1, 1), np.float32)
    assert fv.lib().fvad_vad_batch_run_device(None, sw.h, None, 1, nf, fv.fptr(rms), 1, nf, CHUNK) == fv.FVAD_ERR_NO_DEVICE
