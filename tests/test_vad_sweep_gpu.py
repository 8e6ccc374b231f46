"""Parameter sweeps on the GPU: the multi-band K4 pass (fvad_engine_band_sums_device) against single-band engine calls, the VAD
machine kernel (fvad_vad_batch_run_device) against the host machines bit for bit, and simulator.run_sweep against run_plan."""
import ctypes as C
import json

import numpy as np
import pytest

from test_harness import write_wav
from test_vad_sweep_host import CHUNK, CONFIGS, FS, synth_inputs

pytestmark = pytest.mark.gpu


def engine_bands(fv, ctx, d_pcm, n_lanes, n_samples, d_den, fft_size, band):
    """band sums of one band from a plain engine call (fvad_engine_enqueue_device), [n_lanes][n_frames]"""
    n_den = n_samples // CHUNK * CHUNK
    nf = n_den // fft_size
    d_band = ctx.device_alloc(n_lanes * nf * 4)
    try:
        opts = fv.EngineOpts()
        fv.lib().fvad_engine_opts_default(C.byref(opts))
        opts.min_bin, opts.max_bin, opts.fft_size = band[0], band[1], fft_size
        ctx._ck(fv.lib().fvad_engine_enqueue_device(ctx.h, fv.vp(d_pcm), n_lanes, n_samples, n_samples, fv.vp(d_den), fv.vp(d_band),
                                                    None, C.byref(opts)), "enqueue")
        return ctx.to_host(np.empty((n_lanes, nf), np.float32), d_band)
    finally:
        ctx.device_free(d_band)


@pytest.mark.parametrize("fft_size,bands", [(1024, [(11, 43), (5, 40), (30, 100), (0, 512), (11, 43)]),
                                            (2048, [(22, 86), (5, 40), (100, 300)]),
                                            (1000, [(10, 40), (1, 47)])])
def test_band_sums_device_equal_single_band_engine_calls(fv, pkg, gpu_ctx, fft_size, bands):
    ctx = gpu_ctx
    n_lanes, n_samples = 3, 12 * CHUNK
    pcm = np.stack([pkg.synth.make_stream(n_samples / FS, seed=300 + l)[0][0] for l in range(n_lanes)])
    n_frames = n_samples // fft_size
    d_pcm = ctx.device_alloc(pcm.nbytes)
    d_den = ctx.device_alloc(pcm.nbytes)
    d_den2 = ctx.device_alloc(pcm.nbytes + 64)
    stride = n_frames + 5
    d_multi = ctx.device_alloc(len(bands) * n_lanes * stride * 4)
    try:
        ctx.to_device(d_pcm, np.ascontiguousarray(pcm))
        want = [engine_bands(fv, ctx, d_pcm, n_lanes, n_samples, d_den, fft_size, b) for b in bands]  # d_den: the denoised audio
        ctx.band_sums_device(d_den, n_lanes, n_samples, n_samples, bands, d_multi, stride, fft_size=fft_size)
        got = ctx.to_host(np.empty((len(bands), n_lanes, stride), np.float32), d_multi)
        for j, b in enumerate(bands):
            assert np.array_equal(got[j, :, :n_frames], want[j]), (fft_size, b)
        # the same frames at addresses that are 8- but not 16-byte aligned (lane l at float 2 + l * (n_samples + 2))
        den = ctx.to_host(np.empty((n_lanes, n_samples), np.float32), d_den)
        shifted = np.zeros(2 + n_lanes * (n_samples + 2) + 14, np.float32)
        for l in range(n_lanes):
            shifted[2 + l * (n_samples + 2):2 + l * (n_samples + 2) + n_samples] = den[l]
        ctx.to_device(d_den2, shifted[:(pcm.nbytes + 64) // 4])
        ctx.band_sums_device(d_den2 + 8, n_lanes, n_samples + 2, n_samples, bands, d_multi, stride, fft_size=fft_size)
        got2 = ctx.to_host(np.empty((len(bands), n_lanes, stride), np.float32), d_multi)
        assert np.array_equal(got2[:, :, :n_frames], got[:, :, :n_frames])
        # argument checks
        bad = (C.c_int32 * 2)(10, fft_size // 2 + 1)
        assert fv.lib().fvad_engine_band_sums_device(ctx.h, fv.vp(d_den), n_lanes, n_samples, n_samples, fft_size, bad, 1,
                                                     fv.vp(d_multi), stride) == fv.FVAD_ERR_OUT_OF_RANGE
        bad = (C.c_int32 * 2)(40, 39)
        assert fv.lib().fvad_engine_band_sums_device(ctx.h, fv.vp(d_den), n_lanes, n_samples, n_samples, fft_size, bad, 1,
                                                     fv.vp(d_multi), stride) == fv.FVAD_ERR_OUT_OF_RANGE
    finally:
        for a in (d_pcm, d_den, d_den2, d_multi):
            ctx.device_free(a)


def sweep_configs(n, seed):
    """n configs that vary every field; config 1 opens and closes on almost every burst"""
    rng = np.random.default_rng(seed)
    band_choices = [(500.0, 2000.0), (300.0, 3400.0), (1000.0, 4000.0), (200.0, 1200.0)]
    out = [{}, {"long_term_speech_avg_sec": 5.0, "has_initial_long_term_avg": 0, "short_term_speech_avg_sec": 0.05,
                "speech_threshold_factor": 1.5, "channel_vol_ratio_avg_sec": 0.1, "min_consecutive_sec_to_open": 0.0,
                "max_speech_gap_sec": 0.0, "min_vad_duration_sec": 0.0}]
    out += [dict(c) for c in CONFIGS[1:]]
    while len(out) < n:
        lo, hi = band_choices[rng.integers(len(band_choices))]
        c = {"speech_min_freq": lo, "speech_max_freq": hi, "long_term_speech_avg_sec": float(rng.choice([2.0, 6.0, 15.0, 30.0, 180.0])),
             "short_term_speech_avg_sec": float(rng.uniform(0.05, 0.6)), "speech_threshold_factor": float(rng.uniform(1.5, 8.0)),
             "channel_vol_ratio_avg_sec": float(rng.uniform(0.1, 2.0)), "channel_vol_ratio_threshold": float(rng.uniform(0.2, 0.6)),
             "min_consecutive_sec_to_open": float(rng.uniform(0.0, 0.5)), "max_speech_gap_sec": float(rng.uniform(0.0, 3.0)),
             "min_vad_duration_sec": float(rng.uniform(0.0, 1.0))}
        if rng.uniform() < 0.4:
            c["has_initial_long_term_avg"] = 0
        else:
            c["initial_long_term_avg"] = float(rng.uniform(0.05, 1.0))
        out.append(c)
    return out[:n]


def run_both(fv, ctx, cfgs, n_chunks, nch, seed):
    """device sweep over ragged streams vs one host sweep per stream: (device VadSweep, [host VadSweep per stream])"""
    S = len(n_chunks)
    dev = fv.VadSweep(S, cfgs, n_channels=nch)
    bins, _ = dev.bands()
    maxc = max(n_chunks)
    band, rms = synth_inputs(S, nch, maxc, bins, seed)
    nf = [k * CHUNK // 1024 for k in n_chunks]
    stride = band.shape[2]
    d_band = ctx.device_alloc(band.nbytes)
    try:
        ctx.to_device(d_band, band)
        dev.run_device(ctx, d_band, stride, nf, rms, n_chunks)
    finally:
        ctx.device_free(d_band)
    hosts = []
    for s in range(S):
        h = fv.VadSweep(1, cfgs, n_channels=nch)
        h.run(np.ascontiguousarray(band[:, s * nch:(s + 1) * nch, :nf[s]]), np.ascontiguousarray(rms[s * nch:(s + 1) * nch, :n_chunks[s]]),
              n_threads=8)
        hosts.append(h)
    return dev, hosts


def assert_same(dev, hosts, n_configs):
    n_segs = 0
    for c in range(n_configs):
        dsegs = dev.segments(c)
        for s, h in enumerate(hosts):
            assert dsegs[s] == h.segments(c)[0], (s, c)
            assert dev.audit(s, c) == h.audit(0, c), (s, c)
            n_segs += len(dsegs[s])
    return n_segs


def test_device_machines_equal_host_machines(fv, gpu_ctx):
    ctx = gpu_ctx
    cfgs = sweep_configs(64, seed=3)
    n_chunks = [200, 40, 120, 8, 160, 64, 1, 96]    # ragged; most shorter than a 30 s or 180 s long-term ring
    dev, hosts = run_both(fv, ctx, cfgs, n_chunks, 2, seed=21)
    n_segs = assert_same(dev, hosts, len(cfgs))
    assert n_segs > 500
    busiest = max(len(x) for x in dev.segments(1))
    assert busiest >= 20
    # the other lane mapping (a config's streams side by side in a wavefront): the same bits
    ctx.set_option("vad_lane_map", "config")
    try:
        dev3, hosts3 = run_both(fv, ctx, cfgs, n_chunks, 2, seed=21)
        assert_same(dev3, hosts3, len(cfgs))
    finally:
        ctx.set_option("vad_lane_map", None)
    # the overflow path: room for 2 segments per machine in the first launch, a second launch with room for all
    ctx.set_option("vad_seg_cap", "2")
    try:
        dev2, hosts2 = run_both(fv, ctx, cfgs, n_chunks, 2, seed=21)
        assert_same(dev2, hosts2, len(cfgs))
    finally:
        ctx.set_option("vad_seg_cap", None)


def test_two_hour_stream_device_equals_host(fv, gpu_ctx, capsys):
    cfgs = sweep_configs(16, seed=8)
    n_chunks = [14400]  # 2 h
    dev, hosts = run_both(fv, gpu_ctx, cfgs, n_chunks, 2, seed=33)
    n = assert_same(dev, hosts, len(cfgs))
    with capsys.disabled():
        print(f"\n2 h stream, {len(cfgs)} configs, {n} segments; exact long-term evaluations (device / host) per config:")
        print(" ".join(f"{dev.lazy_stats(0, c)[0]}/{hosts[0].lazy_stats(0, c)[0]}" for c in range(len(cfgs))))


def test_run_sweep_rows_equal_run_plan(pkg, fv, gpu_ctx, tmp_path):
    ctx = gpu_ctx
    synth, sim = pkg.synth, pkg.simulator
    insts = []
    for i, (nch, fmt, sec) in enumerate(((1, "f32", 70.0), (2, "pcm16", 45.0), (1, "pcm16", 30.5))):
        pcm, labels = synth.make_stream(sec, seed=400 + i, n_channels=nch)
        write_wav(str(tmp_path / f"s{i}.wav"), pcm, fmt=fmt)
        (tmp_path / f"s{i}.txt").write_text(synth.labels_to_audacity(labels))
        insts.append({"name": f"stream{i}", "audio_path": f"s{i}.wav", "ref_path": f"s{i}.txt"})
    primary = {"speech_threshold_factor": 8}
    alts = [{"speech_min_freq": 300, "speech_max_freq": 3400, "speech_threshold_factor": 5},
            {"long_term_speech_avg_sec": 20, "initial_long_term_avg": None, "min_vad_duration_sec": 0.4},
            {"speech_min_freq": 1000, "speech_max_freq": 4000, "max_speech_gap_sec": 1.0}]
    plan = {"instances": insts, "config": {"vad_config": {"vad_machine_config": primary, "alt_vad_machine_configs": alts}}}
    (tmp_path / "plan.json").write_text(json.dumps(plan))
    ctx.set_option("reproducible", "1")
    try:
        res = sim.run_sweep(str(tmp_path / "plan.json"), ctx=ctx, out=None, json_path=str(tmp_path / "sweep.json"), vad_on="device")
        assert len(res["rows"]) == 4
        host = sim.run_sweep(str(tmp_path / "plan.json"), ctx=ctx, out=None)   # (auto: four configs run on the host)
        assert host["segments"] == res["segments"] and [bytes(a) for a in host["aggregates"]] == [bytes(a) for a in res["aggregates"]]
        for k, cfg in enumerate([primary] + alts):
            p = dict(plan)
            p["config"] = {"vad_config": {"vad_machine_config": cfg}}
            (tmp_path / f"plan{k}.json").write_text(json.dumps(p))
            _, results = sim.run_plan(str(tmp_path / f"plan{k}.json"), ctx=ctx, out=None)
            agg = fv.stats_aggregate([r["stats"] for r in results])
            assert bytes(res["aggregates"][k]) == bytes(agg), k
            assert [r["segments"] for r in results] == res["segments"][k], k
            assert sum(len(r["segments"]) for r in results) > 0
    finally:
        ctx.set_option("reproducible", None)
    assert json.load(open(tmp_path / "sweep.json"))["rows"][0]["config"] == 0
