"""Dropping configs between device parts (fvad_vad_batch_retain_configs, kernels_vadretain.hip): retains at one and at two
points against a fresh device batch of the survivors and the host machines, bit for bit -- both lane maps, both ring forms (a
retain that moves the rings from global memory to LDS), a sized batch losing a size, device-held segments and scores, segment
room overflow after a retain, a two-hour stream -- device_bytes, the context rules, one case against the CPU oracle, and
simulator.run_grid with successive halving against plain sliced runs."""
import json
import math

import numpy as np
import pytest

import vad_oracle_cases as V
from test_vad_parts_gpu import N_CHUNKS, frames_of, host_results, one_launch, results
from test_harness import write_wav
from test_vad_score_gpu import assert_bits, write_plan
from test_vad_score_host import make_labels, stat_cfgs_of
from test_vad_sizes_host import synth_sized
from test_vad_sweep_gpu import sweep_configs
from test_vad_sweep_host import CHUNK, FS, synth_inputs

pytestmark = pytest.mark.gpu

FFT = 1024


def by_band_inputs(fv, cfgs, n_chunks, nch, seed):
    probe = fv.VadSweep(len(n_chunks), cfgs, n_channels=nch)
    bins, _ = probe.bands()
    probe.close()
    band, rms = synth_inputs(len(n_chunks), nch, max(n_chunks), bins, seed)
    return {b: band[j] for j, b in enumerate(bins)}, rms


def blocks(sw, by_band):
    bins, _ = sw.bands()
    return np.ascontiguousarray(np.stack([by_band[b] for b in bins]))


def device_parts(ctx, sw, by_band, rms, n_chunks, bounds, retains=None):
    """sw over the parts [bounds[k], bounds[k + 1]) (chunks), each part's band sums (the batch's bands as they are then)
    uploaded on their own; retains[k] (indices of the batch as it is then) after part k"""
    retains = retains or {}
    for k, (c0, c1) in enumerate(zip(bounds[:-1], bounds[1:])):
        f0, f1 = frames_of(c0), frames_of(c1)
        nf = [max(0, min(frames_of(n), f1) - f0) for n in n_chunks]
        nc = [max(0, min(n, c1) - c0) for n in n_chunks]
        part = np.ascontiguousarray(blocks(sw, by_band)[:, :, f0:f0 + max(max(nf), 1)])
        prms = np.ascontiguousarray(rms[:, c0:c0 + max(max(nc), 1)])
        d = ctx.device_alloc(part.nbytes)
        try:
            ctx.to_device(d, part)
            sw.run_device_part(ctx, d, part.shape[2], nf, prms, nc, f0)
        finally:
            ctx.device_free(d)
        if k in retains:
            before, n_before = sw.device_bytes(), sw.n_configs
            sw.retain(ctx, retains[k])
            if len(retains[k]) < n_before:   # dropping configs gives memory back
                assert 0 < sw.device_bytes() < before


def composed(n, retains):
    idx = list(range(n))
    for k in sorted(retains):
        idx = [idx[j] for j in retains[k]]
    return idx


def fresh_device(fv, ctx, cfgs, kept, by_band, rms, n_chunks, nch):
    sub = fv.VadSweep(len(n_chunks), [cfgs[i] for i in kept], n_channels=nch)
    try:
        one_launch(fv, ctx, sub, blocks(sub, by_band), rms, n_chunks)
        return results(sub, len(n_chunks), len(kept))
    finally:
        sub.close()


@pytest.mark.parametrize("lane_map", [None, "config"])
@pytest.mark.parametrize("long_short_term", [False, True])
def test_retains_between_device_parts(fv, gpu_ctx, lane_map, long_short_term):
    """with long_short_term every third config has a 5 s short-term ring (global rings); the retains drop all of them, so the
    batch goes on with its rings in LDS"""
    ctx = gpu_ctx
    cfgs = sweep_configs(40, seed=11)
    if long_short_term:
        for c in cfgs[::3]:
            c["short_term_speech_avg_sec"] = 5.0
    S, nch = len(N_CHUNKS), 2
    by_band, rms = by_band_inputs(fv, cfgs, N_CHUNKS, nch, seed=5)
    first = [c for c in range(40) if c % 3 != 0 or not long_short_term]
    plans = {
        "one retain": ([0, 48, 96, 200], {0: first[::2]}),
        "two retains": (list(range(0, 200, 16)) + [200], {1: first[1::2], 6: [0, 2, 3, 7, 9]}),
    }
    if lane_map:
        ctx.set_option("vad_lane_map", lane_map)
    try:
        for name, (bounds, retains) in plans.items():
            kept = composed(40, retains)
            want = fresh_device(fv, ctx, cfgs, kept, by_band, rms, N_CHUNKS, nch)
            sw = fv.VadSweep(S, cfgs, n_channels=nch)
            try:
                device_parts(ctx, sw, by_band, rms, N_CHUNKS, bounds, retains)
                assert results(sw, S, len(kept)) == want, name
            finally:
                sw.close()
            sub_cfgs = [cfgs[i] for i in kept]
            sub_band = np.ascontiguousarray(np.stack([by_band[b] for b in fv.VadSweep(S, sub_cfgs, n_channels=nch).bands()[0]]))
            assert host_results(fv, sub_cfgs, sub_band, rms, N_CHUNKS, nch) == want, name
    finally:
        ctx.set_option("vad_lane_map", None)


def test_sized_device_parts_lose_a_size(fv, gpu_ctx):
    ctx = gpu_ctx
    S, nch, K = 3, 2, 128
    cfgs = sweep_configs(12, seed=4)
    sizes = [[512, 1024, 2048][i % 3] for i in range(12)]
    sw = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    all_bands, _ = sw.bands()
    band, rms = synth_sized(S, nch, K, all_bands, seed=8)
    by_band = {b: band[j] for j, b in enumerate(all_bands)}

    def part(batch, c0, c1, one_shot=False):
        bands, _ = batch.bands()
        s0 = c0 * CHUNK
        nf = [[(c1 * CHUNK) // F - s0 // F] * S for F in batch.sizes]
        n = max(max(r) for r in nf)
        out = np.zeros((len(bands), S * nch, max(n, 1)), np.float32)
        for j, (F, _, _) in enumerate(bands):
            m = (c1 * CHUNK) // F - s0 // F
            out[j, :, :m] = by_band[bands[j]][:, s0 // F:s0 // F + m]
        d = ctx.device_alloc(out.nbytes)
        try:
            ctx.to_device(d, out)
            r = np.ascontiguousarray(rms[:, c0:c1])
            if one_shot:
                batch.run_device(ctx, d, out.shape[2], nf, r, [c1 - c0] * S)
            else:
                batch.run_device_part(ctx, d, out.shape[2], nf, r, [c1 - c0] * S, s0)
        finally:
            ctx.device_free(d)

    keep1 = [c for c in range(12) if sizes[c] != 2048]       # 2048 goes
    keep2 = [0, 1, 3, 4, 6]
    try:
        part(sw, 0, 32)
        sw.retain(ctx, keep1)
        assert sorted(sw.sizes) == [512, 1024]
        part(sw, 32, 64)
        sw.retain(ctx, keep2)
        part(sw, 64, K)
        kept = [keep1[j] for j in keep2]
        sub = fv.VadSweepSized(S, [cfgs[i] for i in kept], [sizes[i] for i in kept], n_channels=nch)
        part(sub, 0, K, one_shot=True)
        assert sub.bands() == sw.bands()
        assert results(sw, S, len(kept)) == results(sub, S, len(kept))
        sub.close()
    finally:
        sw.close()


def test_device_held_segments_scores_and_overflow(fv, gpu_ctx):
    ctx = gpu_ctx
    cfgs = sweep_configs(48, seed=3)
    S, nch = len(N_CHUNKS), 2
    by_band, rms = by_band_inputs(fv, cfgs, N_CHUNKS, nch, seed=13)
    rng = np.random.default_rng(1)
    labels = [make_labels(rng, n * CHUNK / FS, 6, "mixed") for n in N_CHUNKS]
    scs = stat_cfgs_of(cfgs, seed=2)
    retains = {2: list(range(0, 48, 2)), 5: [1, 4, 5, 9, 17, 22]}
    kept = composed(48, retains)
    sub = fv.VadSweep(S, [cfgs[i] for i in kept], n_channels=nch)
    sub.set_references(labels, [scs[i] for i in kept])
    sub.keep_segments(False)
    one_launch(fv, ctx, sub, blocks(sub, by_band), rms, N_CHUNKS)
    want_scores = [sub.config_stats(c).copy() for c in range(len(kept))]
    want = results(sub, S, len(kept), segments=False)
    sub.close()
    ctx.set_option("vad_seg_cap", "2")   # room for 2 segments per machine: parts pause and grow, before and after the retains
    try:
        sw = fv.VadSweep(S, cfgs, n_channels=nch)
        try:
            sw.set_references(labels, scs)
            sw.keep_segments(False)
            device_parts(ctx, sw, by_band, rms, N_CHUNKS, list(range(0, 200, 16)) + [200], retains)
            assert results(sw, S, len(kept), segments=False) == want
            sw.score_device(ctx)
            for c in range(len(kept)):
                assert np.array_equal(sw.config_stats(c).view(np.uint32), want_scores[c].view(np.uint32)), c
        finally:
            sw.close()
    finally:
        ctx.set_option("vad_seg_cap", None)


def test_device_bytes_and_context_rules(fv, gpu_ctx):
    ctx = gpu_ctx
    lib = fv.lib()
    cfgs = sweep_configs(16, seed=2)
    n_chunks = [64, 48]
    by_band, rms = by_band_inputs(fv, cfgs, n_chunks, 1, seed=9)
    keep = [1, 2, 5, 8, 13]
    want = fresh_device(fv, ctx, cfgs, keep, by_band, rms, n_chunks, 1)
    sw = fv.VadSweep(2, cfgs)
    other = fv.Context(0)
    try:
        other.load_synth(7)
        device_parts(ctx, sw, by_band, rms, n_chunks, [0, 16])
        before = sw.device_bytes()
        arr = (fv.C.c_uint32 * len(keep))(*keep)
        INV = fv.FVAD_ERR_INVALID_ARGUMENT
        assert lib.fvad_vad_batch_retain_configs(None, sw.h, arr, len(keep)) == INV     # part state needs its context
        assert lib.fvad_vad_batch_retain_configs(other.h, sw.h, arr, len(keep)) == INV  # not another one
        bad = (fv.C.c_uint32 * 2)(3, 3)
        assert lib.fvad_vad_batch_retain_configs(ctx.h, sw.h, bad, 2) == INV
        assert sw.device_bytes() == before and lib.fvad_vad_batch_n_configs(sw.h) == 16
        # the parts go on after the failed calls, then a retain, then the rest
        device_parts(ctx, sw, by_band, rms, n_chunks, [16, 32], {0: keep})
        assert 0 < sw.device_bytes() < before
        device_parts(ctx, sw, by_band, rms, n_chunks, [32, 64])
        assert results(sw, 2, len(keep)) == want
    finally:
        sw.close()
        other.close()


def test_two_hour_stream_with_retains(fv, gpu_ctx):
    ctx = gpu_ctx
    cfgs = sweep_configs(12, seed=8)
    n_chunks = [14400]
    by_band, rms = by_band_inputs(fv, cfgs, n_chunks, 2, seed=33)
    retains = {1: [0, 2, 4, 5, 7, 9, 11], 4: [1, 3, 6]}
    kept = composed(12, retains)
    want = fresh_device(fv, ctx, cfgs, kept, by_band, rms, n_chunks, 2)
    sw = fv.VadSweep(1, cfgs, n_channels=2)
    try:
        device_parts(ctx, sw, by_band, rms, n_chunks, list(range(0, 14400, 1808)) + [14400], retains)
        assert results(sw, 1, len(kept)) == want
    finally:
        sw.close()


def test_device_retain_equals_oracle(fv, pkg, weights7, gpu_ctx):
    ctx = gpu_ctx
    o = V.oracle_case(pkg, weights7, 48000, 2, 512)
    rate, nch, F, chunk = o["rate"], o["nch"], o["F"], o["chunk"]
    cfgs = V.case_configs(rate, F, seed=F + nch)
    sw = fv.VadSweep(1, cfgs, n_channels=nch, sample_rate=rate, fft_size=F)
    all_bins, _ = sw.bands()
    band_all = V.band_blocks(o["bins"], all_bins)
    by_band = {b: band_all[j] for j, b in enumerate(all_bins)}
    rms = np.ascontiguousarray(o["rms"].T)
    n_chunks = rms.shape[1]
    nf_all = n_chunks * chunk // F
    step = math.lcm(chunk, F) // chunk
    cut = (n_chunks // 2) // step * step
    keep = list(range(1, len(cfgs), 2))
    try:
        for c0, c1, after in ((0, cut, keep), (cut, n_chunks, None)):
            bins, _ = sw.bands()
            f0, f1 = c0 * chunk // F, (nf_all if c1 == n_chunks else c1 * chunk // F)
            part = np.ascontiguousarray(np.stack([by_band[b] for b in bins])[:, :, f0:f1])
            d = ctx.device_alloc(part.nbytes)
            try:
                ctx.to_device(d, part)
                sw.run_device_part(ctx, d, part.shape[2], [f1 - f0], np.ascontiguousarray(rms[:, c0:c1]), [c1 - c0], f0,
                                   chunk_size=chunk)
            finally:
                ctx.device_free(d)
            if after:
                sw.retain(ctx, after)
        bins, band_of = sw.bands()
        want = V.oracle_machines([(cfgs[i], rate, nch, F, by_band[bins[band_of[c]]], o["ratio"]) for c, i in enumerate(keep)])
        for c, (segs, audit) in enumerate(want):
            assert V.seg_bits(sw.segments(c)[0]) == V.seg_bits(segs), keep[c]
            assert V.audit_bits(sw.audit(0, c)) == V.audit_bits(audit), keep[c]
    finally:
        sw.close()


# ------------------------------------------------------------------ run_grid with successive halving

GRID = {"base": {"speech_min_freq": 300, "speech_max_freq": 3000},
        "axes": {"speech_threshold_factor": [2.5, 4.0, 7.0, 10.0], "initial_long_term_avg": [None, 0.3],
                 "min_vad_duration_sec": [0.2, 0.7]}}
STREAMS = [(1, "pcm16", 47.3), (2, "f32", 61.1), (1, "f32", 33.9), (2, "pcm16", 20.2)]


def test_run_grid_halving(fv, pkg, gpu_ctx, tmp_path):
    sim = pkg.simulator
    ctx = gpu_ctx
    plan = write_plan(pkg, tmp_path, STREAMS)
    N, eta, R = 16, 2, 2
    ctx.set_option("reproducible", "1")
    try:
        hv = sim.run_grid(plan, GRID, ctx=ctx, out=None, vad_on="device", score_on="device", slice_chunks=N,
                          halving_eta=eta, halving_rungs=R, json_path=str(tmp_path / "h.json"))
        NC = len(hv["configs"])
        K = max(int(sec * 2) for _, _, sec in STREAMS)
        ends = sim.halving_schedule(K, N, eta, R)
        assert len(ends) == 2 and len(hv["rung_times"]) == 3
        assert [g["end_chunk"] for g in hv["rung_times"][:2]] == ends
        assert len(hv["survivors"]) == math.ceil(math.ceil(NC / eta) / eta)
        assert [c for c in range(NC) if hv["rung"][c] is None] == hv["survivors"]
        assert [r["rung"] for r in hv["rows"]] == hv["rung"]
        doc = json.loads((tmp_path / "h.json").read_text())
        assert doc["survivors"] == hv["survivors"] and [r["rung"] for r in doc["rows"]] == hv["rung"]
        # the survivors' statistics: those of a plain sliced run
        plain = sim.run_grid(plan, GRID, ctx=ctx, out=None, vad_on="device", score_on="device", slice_chunks=N)
        assert_bits(hv["stats"][hv["survivors"]], plain["stats"][hv["survivors"]])
        # the dropped set at rung 1: the API on the prefix -- each instance's audio and labels cut at the rung
        (tmp_path / "p").mkdir()
        insts = json.loads(open(plan).read())
        t_end = ends[0] * CHUNK / FS
        for inst in insts["instances"]:
            pcm, _ = fv.wav_read(str(tmp_path / inst["audio_path"]))
            n = min(pcm.shape[1], ends[0] * CHUNK)
            write_wav(str(tmp_path / "p" / inst["audio_path"]), np.ascontiguousarray(pcm[:, :n]), fmt="f32")
            t = np.float32(min(t_end, (pcm.shape[1] // CHUNK) * CHUNK / FS))   # the rung's end, or the instance's
            labs = fv.parse_audacity((tmp_path / inst["ref_path"]).read_text())
            cut = [(a, min(np.float32(b), t)) for a, b in labs if np.float32(a) < t]
            (tmp_path / "p" / inst["ref_path"]).write_text("".join(f"{a:.9g}\t{b:.9g}\tspeech\n" for a, b in cut))
        (tmp_path / "p" / "plan.json").write_text(json.dumps(insts))
        pre = sim.run_grid(str(tmp_path / "p" / "plan.json"), GRID, ctx=ctx, out=None, vad_on="device", score_on="device",
                           slice_chunks=N)
        ranked = [r["config"] for r in sim._ranked(pre["rows"])]
        kept1 = sorted(ranked[:math.ceil(NC / eta)])
        assert [c for c in range(NC) if hv["rung"][c] != 1] == kept1
    finally:
        ctx.set_option("reproducible", None)
    # the default mode completes
    out = sim.run_grid(plan, GRID, ctx=ctx, out=None, vad_on="device", score_on="device", slice_chunks=32, halving_eta=4,
                       halving_rungs=1)
    assert len(out["survivors"]) == math.ceil(NC / 4)
