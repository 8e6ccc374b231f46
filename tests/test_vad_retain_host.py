"""Dropping configs from a VAD batch (fvad_vad_batch_retain_configs) on the host: the argument rules, a retain before any run,
retains between host parts (plain and sized batches, 1 / 2 / 5 channels, several partitions), held and later scores -- each
against a fresh batch of the kept configs run over all the parts, bit for bit -- a few cases pinned to the CPU oracle, and the
harness side of successive halving (simulator.halving_schedule, run_grid's argument checks).  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

import vad_oracle_cases as V
from test_vad_score_host import make_labels, stat_cfgs_of
from test_vad_sizes_host import results, synth_sized
from test_vad_sweep_host import CHUNK, CONFIGS, FS, synth_inputs

FFT = 1024
N_CHUNKS = 96   # six 16-chunk frame-aligned steps at 1024 points


def inputs_by_band(fv, cfgs, S, nch, n_chunks, seed):
    """{(min_bin, max_bin): [lanes][n_frames]} for every band of cfgs, and the chunk RMS [lanes][n_chunks]"""
    probe = fv.VadSweep(S, cfgs, n_channels=nch)
    bins, _ = probe.bands()
    probe.close()
    band, rms = synth_inputs(S, nch, n_chunks, bins, seed)
    return {b: band[j] for j, b in enumerate(bins)}, rms


def blocks_of(sw, by_band):
    bins, _ = sw.bands()
    return np.ascontiguousarray(np.stack([by_band[b] for b in bins]))


def host_parts(fv, sw, by_band, rms, bounds, retains=None):
    """sw over the parts [bounds[k], bounds[k + 1]) (chunks) with fvad_vad_batch_run_part; after part k, retains[k] (indices of
    the batch as it is then) when given"""
    retains = retains or {}
    for k, (c0, c1) in enumerate(zip(bounds[:-1], bounds[1:])):
        f0, f1 = c0 * CHUNK // FFT, c1 * CHUNK // FFT
        band = np.ascontiguousarray(blocks_of(sw, by_band)[:, :, f0:f1])
        r = np.ascontiguousarray(rms[:, c0:c1])
        fv.check(fv.lib().fvad_vad_batch_run_part(sw.h, band.ctypes.data_as(fv.c_float_p), max(f1 - f0, 1), f1 - f0,
                                                  r.ctypes.data_as(fv.c_float_p), r.shape[1], c1 - c0, CHUNK, f0, 4),
                 "fvad_vad_batch_run_part")
        if k in retains:
            sw.retain(None, retains[k])


def composed(n, retains):
    """the original indices the retains leave, in order"""
    idx = list(range(n))
    for k in sorted(retains):
        idx = [idx[j] for j in retains[k]]
    return idx


def fresh_results(fv, cfgs, kept, S, nch, by_band, rms, n_chunks):
    sub = fv.VadSweep(S, [cfgs[i] for i in kept], n_channels=nch)
    try:
        host_parts(fv, sub, by_band, rms, [0, n_chunks])
        return results(sub, S, len(kept)), sub.bands()
    finally:
        sub.close()


def raw_retain(fv, sw, keep, ctx=None):
    arr = (C.c_uint32 * max(len(keep), 1))(*keep)
    return fv.lib().fvad_vad_batch_retain_configs(ctx, sw.h, arr, len(keep))


# ------------------------------------------------------------------ argument rules


def test_argument_rules_leave_the_batch_unchanged(fv):
    S, nch = 3, 2
    cfgs = CONFIGS[:8]
    by_band, rms = inputs_by_band(fv, cfgs, S, nch, N_CHUNKS, seed=1)
    want, _ = fresh_results(fv, cfgs, list(range(8)), S, nch, by_band, rms, N_CHUNKS)
    sw = fv.VadSweep(S, cfgs, n_channels=nch)
    try:
        host_parts(fv, sw, by_band, rms, [0, 32])
        bad = [[], [3, 1], [2, 2], [0, 8], [8], [1, 5, 4]]
        for keep in bad:
            assert raw_retain(fv, sw, keep) == fv.FVAD_ERR_INVALID_ARGUMENT, keep
            assert fv.lib().fvad_vad_batch_n_configs(sw.h) == 8
        assert fv.lib().fvad_vad_batch_retain_configs(None, sw.h, None, 2) == fv.FVAD_ERR_INVALID_ARGUMENT
        arr = (C.c_uint32 * 1)(0)
        assert fv.lib().fvad_vad_batch_retain_configs(None, None, arr, 1) == fv.FVAD_ERR_INVALID_ARGUMENT
        with pytest.raises(fv.FvadError):
            sw.retain(None, [4, 4])
        # the batch runs on as if nothing had been asked
        f0 = 32 * CHUNK // FFT
        band = np.ascontiguousarray(blocks_of(sw, by_band)[:, :, f0:])
        r = np.ascontiguousarray(rms[:, 32:])
        fv.check(fv.lib().fvad_vad_batch_run_part(sw.h, band.ctypes.data_as(fv.c_float_p), band.shape[2], band.shape[2],
                                                  r.ctypes.data_as(fv.c_float_p), r.shape[1], r.shape[1], CHUNK, f0, 4), "run_part")
        assert results(sw, S, 8) == want
    finally:
        sw.close()


# ------------------------------------------------------------------ before any run


def test_retain_before_running_is_create_sweep_of_the_subset(fv):
    keep = [1, 2, 5, 9]
    sw = fv.VadSweep(2, CONFIGS, n_channels=2)
    sub = fv.VadSweep(2, [CONFIGS[i] for i in keep], n_channels=2)
    try:
        sw.retain(None, keep)
        assert sw.n_configs == fv.lib().fvad_vad_batch_n_configs(sw.h) == 4
        assert sw.bands() == sub.bands()
        assert len(sw.bands()[0]) < len(fv.VadSweep(2, CONFIGS).bands()[0])
        by_band, rms = inputs_by_band(fv, CONFIGS, 2, 2, N_CHUNKS, seed=2)
        host_parts(fv, sw, by_band, rms, [0, N_CHUNKS])
        host_parts(fv, sub, by_band, rms, [0, N_CHUNKS])
        assert results(sw, 2, 4) == results(sub, 2, 4)
    finally:
        sw.close()
        sub.close()


def test_sized_retain_drops_a_size_and_a_band(fv):
    cfgs = [dict(CONFIGS[0]), dict(CONFIGS[1]), dict(CONFIGS[2]), dict(CONFIGS[0]), dict(CONFIGS[5])]
    sizes = [512, 1024, 512, 2048, 1024]
    sw = fv.VadSweepSized(2, cfgs, sizes)
    try:
        assert sw.sizes == [512, 1024, 2048]
        keep = [1, 2, 4]   # 2048 goes, and with it band (2048, CONFIGS[0]); CONFIGS[0]'s band at 512 goes too
        sw.retain(None, keep)
        sub = fv.VadSweepSized(2, [cfgs[i] for i in keep], [sizes[i] for i in keep])
        assert sw.sizes == sub.sizes == [1024, 512]
        assert sw.bands() == sub.bands() and sw.size_of_band == sub.size_of_band
        sub.close()
    finally:
        sw.close()


# ------------------------------------------------------------------ host parts


@pytest.mark.parametrize("nch", [1, 2, 5])
def test_retains_between_host_parts_equal_a_fresh_subset(fv, nch):
    S = 3
    cfgs = CONFIGS
    by_band, rms = inputs_by_band(fv, cfgs, S, nch, N_CHUNKS, seed=10 + nch)
    plans = {
        "after part 1 and 3": ([0, 16, 32, 64, 80, N_CHUNKS], {0: [0, 2, 3, 5, 7, 8, 10, 11], 2: [1, 2, 5, 6]}),
        "uneven parts": ([0, 48, 64, N_CHUNKS], {0: [4, 9], 1: [1]}),
        "keep all": ([0, 32, N_CHUNKS], {0: list(range(len(cfgs)))}),
        "keep one": ([0, 16, N_CHUNKS], {0: [6]}),
    }
    n_segs = 0
    for name, (bounds, retains) in plans.items():
        kept = composed(len(cfgs), retains)
        want, want_bands = fresh_results(fv, cfgs, kept, S, nch, by_band, rms, N_CHUNKS)
        sw = fv.VadSweep(S, cfgs, n_channels=nch)
        try:
            host_parts(fv, sw, by_band, rms, bounds, retains)
            assert sw.n_configs == len(kept)
            assert sw.bands() == want_bands, name
            assert results(sw, S, len(kept)) == want, name
            n_segs += sum(len(x) for per in want[0] for x in per)
        finally:
            sw.close()
    assert n_segs > 50


def test_sized_retains_between_host_parts(fv):
    S, nch, K = 2, 2, 64
    cfgs = [dict(CONFIGS[i % len(CONFIGS)]) for i in range(9)]
    sizes = [512, 1024, 2048, 1024, 512, 2048, 1000, 1024, 512]
    sw = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    all_bands, _ = sw.bands()
    band, rms = synth_sized(S, nch, K, all_bands, seed=4)
    by_band = {b: band[j] for j, b in enumerate(all_bands)}

    def run(batch, c0, c1):
        bands, _ = batch.bands()
        blk = np.stack([by_band[b] for b in bands])
        s0 = c0 * CHUNK
        nf = [(c1 * CHUNK) // F - s0 // F for F in batch.sizes]
        # each size's frames from its own first frame (a block of size F holds frame k at column k)
        out = np.zeros((len(bands), S * nch, max(max(nf), 1)), np.float32)
        for j, (F, _, _) in enumerate(bands):
            n = (c1 * CHUNK) // F - s0 // F
            out[j, :, :n] = blk[j, :, s0 // F:s0 // F + n]
        batch.run(out, np.ascontiguousarray(rms[:, c0:c1]), nf, first_sample=s0, n_threads=4)

    assert all(32 * CHUNK % F == 0 and K * CHUNK % F == 0 for F in sizes)   # the part boundary is a frame of every size
    try:
        run(sw, 0, 32)
        keep = [1, 3, 4, 7, 8]   # 2048 and 1000 go
        sw.retain(None, keep)
        assert sorted(sw.sizes) == [512, 1024]
        run(sw, 32, K)
        sub = fv.VadSweepSized(S, [cfgs[i] for i in keep], [sizes[i] for i in keep], n_channels=nch)
        run(sub, 0, K)
        assert sub.bands() == sw.bands()
        assert results(sw, S, len(keep)) == results(sub, S, len(keep))
        sub.close()
    finally:
        sw.close()


# ------------------------------------------------------------------ scores


def test_scores_after_and_across_a_retain(fv):
    S, nch = 4, 2
    cfgs = CONFIGS
    by_band, rms = inputs_by_band(fv, cfgs, S, nch, N_CHUNKS, seed=7)
    rng = np.random.default_rng(3)
    dur = N_CHUNKS * CHUNK / FS
    labels = [make_labels(rng, dur, 8, "mixed") for _ in range(S)]
    scs = stat_cfgs_of(cfgs, seed=5)
    keep = [0, 3, 4, 10]
    sw = fv.VadSweep(S, cfgs, n_channels=nch)
    sub = fv.VadSweep(S, [cfgs[i] for i in keep], n_channels=nch)
    try:
        sw.set_references(labels, scs)
        sub.set_references(labels, [scs[i] for i in keep])
        host_parts(fv, sw, by_band, rms, [0, 48])
        host_parts(fv, sub, by_band, rms, [0, 48])
        sw.score(4)
        sub.score(4)
        held = [sw.config_stats(i).copy() for i in keep]
        sw.retain(None, keep)
        for c in range(len(keep)):   # the scores held from before the retain, compacted
            assert np.array_equal(sw.config_stats(c).view(np.uint32), held[c].view(np.uint32))
            assert np.array_equal(sw.config_stats(c).view(np.uint32), sub.config_stats(c).view(np.uint32))
        f0 = 48 * CHUNK // FFT
        for b in (sw, sub):
            band = np.ascontiguousarray(blocks_of(b, by_band)[:, :, f0:])
            r = np.ascontiguousarray(rms[:, 48:])
            fv.check(fv.lib().fvad_vad_batch_run_part(b.h, band.ctypes.data_as(fv.c_float_p), band.shape[2], band.shape[2],
                                                      r.ctypes.data_as(fv.c_float_p), r.shape[1], r.shape[1], CHUNK, f0, 4), "run_part")
            b.score(4)
        for c in range(len(keep)):
            assert np.array_equal(sw.config_stats(c).view(np.uint32), sub.config_stats(c).view(np.uint32))
    finally:
        sw.close()
        sub.close()


# ------------------------------------------------------------------ against the oracle


@pytest.mark.parametrize("case", [(48000, 2, 512), (48000, 1, 1024), (48000, 3, 960)], ids=lambda c: "%dk-%dch-F%d" % (c[0] // 1000, c[1], c[2]))
def test_configs_dropped_mid_run_equal_oracle(fv, pkg, weights7, case):
    o = V.oracle_case(pkg, weights7, *case)
    rate, nch, F, chunk = o["rate"], o["nch"], o["F"], o["chunk"]
    cfgs = V.case_configs(rate, F, seed=F + nch)
    sw = fv.VadSweep(1, cfgs, n_channels=nch, sample_rate=rate, fft_size=F)
    all_bins, _ = sw.bands()
    band_all = V.band_blocks(o["bins"], all_bins)
    by_band = {b: band_all[j] for j, b in enumerate(all_bins)}
    rms = np.ascontiguousarray(o["rms"].T)
    n_chunks = rms.shape[1]
    nf = n_chunks * chunk // F
    step = math.lcm(chunk, F) // chunk
    cut = (n_chunks // 2) // step * step
    assert 0 < cut < n_chunks
    keep = list(range(0, len(cfgs), 3))
    try:
        for c0, c1, after in ((0, cut, keep), (cut, n_chunks, None)):
            bins, _ = sw.bands()
            f0, f1 = c0 * chunk // F, (nf if c1 == n_chunks else c1 * chunk // F)
            band = np.ascontiguousarray(np.stack([by_band[b] for b in bins])[:, :, f0:f1])
            r = np.ascontiguousarray(rms[:, c0:c1])
            fv.check(fv.lib().fvad_vad_batch_run_part(sw.h, band.ctypes.data_as(fv.c_float_p), max(f1 - f0, 1), f1 - f0,
                                                      r.ctypes.data_as(fv.c_float_p), r.shape[1], c1 - c0, chunk, f0, 4), "run_part")
            if after:
                sw.retain(None, after)
        _, band_of = sw.bands()
        bins, _ = sw.bands()
        want = V.oracle_machines([(cfgs[i], rate, nch, F, by_band[bins[band_of[c]]], o["ratio"]) for c, i in enumerate(keep)])
        n_segs = 0
        for c, (segs, audit) in enumerate(want):
            assert V.seg_bits(sw.segments(c)[0]) == V.seg_bits(segs), (case, keep[c])
            assert V.audit_bits(sw.audit(0, c)) == V.audit_bits(audit), (case, keep[c])
            n_segs += len(segs)
        assert n_segs >= 1
    finally:
        sw.close()


# ------------------------------------------------------------------ harness


@pytest.fixture(scope="module")
def sim(pkg):
    return pkg.simulator


def test_halving_schedule(sim):
    # K = 1024 chunks, slices of 16, eta 4: rungs at K / 16 = 64 and K / 4 = 256 (both on slice boundaries)
    assert sim.halving_schedule(1024, 16, 4, 2) == [64, 256]
    # K / 16 = 62.5 -> the first boundary at or after it is 64; K / 4 = 250 -> 256
    assert sim.halving_schedule(1000, 16, 4, 2) == [64, 256]
    # rungs landing on the same boundary merge: K = 160, slice 64, eta 2, R = 3: 20, 40, 80 -> 64, 64, 128
    assert sim.halving_schedule(160, 64, 2, 3) == [64, 128]
    # a rung at the end is skipped: K = 40, slice 32: 20 -> 32; K / 1 is the end anyway; eta 2, R = 1: 20 -> 32
    assert sim.halving_schedule(40, 32, 2, 1) == [32]
    # every rung at or past the end: none
    assert sim.halving_schedule(16, 16, 4, 2) == []
    assert sim.halving_schedule(100, 64, 2, 1) == [64]
    # many rungs on a short corpus: the small ones all land on the first boundary
    assert sim.halving_schedule(64, 16, 2, 6) == [16, 32]
    with pytest.raises(ValueError):
        sim.halving_schedule(64, 16, 1, 2)
    with pytest.raises(ValueError):
        sim.halving_schedule(64, 16, 2, 0)


@pytest.mark.parametrize("kw,words", [
    (dict(halving_eta=4, halving_rungs=2), "slice_chunks"),
    (dict(halving_eta=4, halving_rungs=2, slice_chunks=16, vad_on="host", score_on="host"), "vad_on"),
    (dict(halving_eta=4, halving_rungs=2, slice_chunks=16, vad_on="device", score_on="host"), "score_on"),
    (dict(halving_eta=1, halving_rungs=2, slice_chunks=16, vad_on="device"), "eta"),
    (dict(halving_eta=4, halving_rungs=0, slice_chunks=16, vad_on="device"), "rungs"),
    (dict(halving_eta=4, slice_chunks=16, vad_on="device"), "together"),
    (dict(halving_rungs=2, slice_chunks=16, vad_on="device"), "together"),
])
def test_halving_argument_errors_before_any_gpu_work(sim, tmp_path, monkeypatch, kw, words):
    def no_ctx(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(sim, "_make_ctx", no_ctx)
    plan = tmp_path / "plan.json"
    plan.write_text('{"instances": []}')
    grid = {"axes": {"speech_threshold_factor": [2.0, 3.0]}}
    with pytest.raises(ValueError, match=words):
        sim.run_grid(str(plan), grid, out=None, **kw)
