"""Device VAD machines in parts (fvad_vad_batch_run_device_part, kernels_vad.hip's resume form) against one launch
(fvad_vad_batch_run_device) and the host machines bit for bit -- ragged streams, 1 / 2 / 5 channels, both lane maps and ring
forms, segment overflow, device scoring of the parts (fvad_vad_batch_score_device), the argument rules -- and
simulator.run_grid in time slices against the unsliced run."""

import numpy as np
import pytest

from test_vad_score_gpu import assert_bits, write_plan
from test_vad_score_host import make_labels, stat_cfgs_of
from test_vad_sweep_gpu import sweep_configs
from test_vad_sweep_host import CHUNK, FS, synth_inputs

pytestmark = pytest.mark.gpu

FFT = 1024
N_CHUNKS = [200, 40, 120, 8, 160, 64, 1, 96]   # ragged: the streams end in different parts


def frames_of(n_chunks):
    return n_chunks * CHUNK // FFT


def make_inputs(fv, cfgs, n_chunks, nch, seed):
    probe = fv.VadSweep(len(n_chunks), cfgs, n_channels=nch)
    bins, _ = probe.bands()
    probe.close()
    return synth_inputs(len(n_chunks), nch, max(n_chunks), bins, seed)


def run_parts(fv, ctx, sw, band, rms, n_chunks, bounds):
    """sw over the parts [bounds[k], bounds[k + 1]) (in chunks): each part's band sums uploaded on their own"""
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        f0, f1 = frames_of(c0), frames_of(c1)
        nf = [max(0, min(frames_of(k), f1) - f0) for k in n_chunks]
        nc = [max(0, min(k, c1) - c0) for k in n_chunks]
        P = max(nf)
        part = np.ascontiguousarray(band[:, :, f0:f0 + max(P, 1)])
        prms = np.ascontiguousarray(rms[:, c0:c0 + max(max(nc), 1)])
        d = ctx.device_alloc(part.nbytes)
        try:
            ctx.to_device(d, part)
            sw.run_device_part(ctx, d, part.shape[2], nf, prms, nc, f0)
        finally:
            ctx.device_free(d)


def one_launch(fv, ctx, sw, band, rms, n_chunks):
    d = ctx.device_alloc(band.nbytes)
    try:
        ctx.to_device(d, band)
        sw.run_device(ctx, d, band.shape[2], [frames_of(k) for k in n_chunks], rms, n_chunks)
    finally:
        ctx.device_free(d)


def results(sw, S, NC, segments=True):
    return ([sw.segments(c) for c in range(NC)] if segments else None,
            [[sw.audit(s, c) for c in range(NC)] for s in range(S)],
            [[sw.lazy_stats(s, c) for c in range(NC)] for s in range(S)])


def host_results(fv, cfgs, band, rms, n_chunks, nch):
    """one host sweep per stream (ragged lengths), in the shape results() gives"""
    NC, S = len(cfgs), len(n_chunks)
    segs = [[None] * S for _ in range(NC)]
    audits, lazy = [], []
    for s, k in enumerate(n_chunks):
        h = fv.VadSweep(1, cfgs, n_channels=nch)
        try:
            h.run(np.ascontiguousarray(band[:, s * nch:(s + 1) * nch, :frames_of(k)]),
                  np.ascontiguousarray(rms[s * nch:(s + 1) * nch, :max(k, 1)]), n_threads=8)
            for c in range(NC):
                segs[c][s] = h.segments(c)[0]
            audits.append([h.audit(0, c) for c in range(NC)])
            lazy.append([h.lazy_stats(0, c) for c in range(NC)])
        finally:
            h.close()
    return segs, audits, lazy


def partitions(K):
    whole = [0, K]
    by16 = list(range(0, K, 16)) + [K]
    uneven = sorted({0, 16, 64, 80, 176, K} & set(range(0, K)) | {K})
    return {"one part": whole, "16-chunk parts": by16, "uneven parts": uneven}


@pytest.mark.parametrize("nch", [1, 2, 5])
def test_parts_equal_one_launch_and_host(fv, gpu_ctx, nch):
    ctx = gpu_ctx
    cfgs = sweep_configs(64, seed=3)   # null initial_long_term_avg, four bands, every field varied
    assert any(c.get("has_initial_long_term_avg", 1) == 0 for c in cfgs) and len({(c.get("speech_min_freq"), c.get("speech_max_freq")) for c in cfgs}) > 2
    S, NC = len(N_CHUNKS), len(cfgs)
    band, rms = make_inputs(fv, cfgs, N_CHUNKS, nch, seed=21 + nch)
    one = fv.VadSweep(S, cfgs, n_channels=nch)
    one_launch(fv, ctx, one, band, rms, N_CHUNKS)
    want = results(one, S, NC)
    one.close()
    assert host_results(fv, cfgs, band, rms, N_CHUNKS, nch) == want
    assert sum(len(x) for per in want[0] for x in per) > 300
    for name, bounds in partitions(max(N_CHUNKS)).items():
        sw = fv.VadSweep(S, cfgs, n_channels=nch)
        try:
            run_parts(fv, ctx, sw, band, rms, N_CHUNKS, bounds)
            assert results(sw, S, NC) == want, name
            assert sw.device_bytes() > 0
        finally:
            sw.close()


@pytest.mark.parametrize("lane_map", [None, "config"])
@pytest.mark.parametrize("long_short_term", [False, True])
def test_lane_maps_and_ring_forms(fv, gpu_ctx, lane_map, long_short_term):
    """vad_lane_map=config and the rings in global memory: a 5 s short-term window is 234 slots, st + cr > 192 (48 KB of LDS
    per 64 machines)"""
    ctx = gpu_ctx
    cfgs = sweep_configs(40, seed=11)
    if long_short_term:
        for c in cfgs[::3]:
            c["short_term_speech_avg_sec"] = 5.0
    S, NC, nch = len(N_CHUNKS), len(cfgs), 2
    band, rms = make_inputs(fv, cfgs, N_CHUNKS, nch, seed=5)
    if lane_map:
        ctx.set_option("vad_lane_map", lane_map)
    try:
        one = fv.VadSweep(S, cfgs, n_channels=nch)
        one_launch(fv, ctx, one, band, rms, N_CHUNKS)
        want = results(one, S, NC)
        one.close()
        for bounds in (list(range(0, 200, 16)) + [200], [0, 48, 96, 200]):
            sw = fv.VadSweep(S, cfgs, n_channels=nch)
            try:
                run_parts(fv, ctx, sw, band, rms, N_CHUNKS, bounds)
                assert results(sw, S, NC) == want
            finally:
                sw.close()
    finally:
        ctx.set_option("vad_lane_map", None)
    assert host_results(fv, cfgs, band, rms, N_CHUNKS, nch) == want


def test_overflow_and_device_scoring(fv, gpu_ctx):
    ctx = gpu_ctx
    cfgs = sweep_configs(64, seed=3)
    S, NC, nch = len(N_CHUNKS), len(cfgs), 2
    band, rms = make_inputs(fv, cfgs, N_CHUNKS, nch, seed=21)
    rng = np.random.default_rng(4)
    refs = [make_labels(rng, k * CHUNK / FS, max(2, int(k * CHUNK / FS / 6)), "empty" if s == 2 else "mixed")
            for s, k in enumerate(N_CHUNKS)]
    scs = stat_cfgs_of(cfgs, 4)
    one = fv.VadSweep(S, cfgs, n_channels=nch)
    one.set_references(refs, scs)
    one_launch(fv, ctx, one, band, rms, N_CHUNKS)
    want = results(one, S, NC)
    want_stats = np.stack([one.config_stats(c) for c in range(NC)])
    one.close()
    bounds = list(range(0, 200, 16)) + [200]
    ctx.set_option("vad_seg_cap", "2")   # every busy machine overflows its room, part after part
    try:
        sw = fv.VadSweep(S, cfgs, n_channels=nch)
        run_parts(fv, ctx, sw, band, rms, N_CHUNKS, bounds)
        assert results(sw, S, NC) == want
        sw.set_references(refs, scs)
        sw.score(8)
        assert_bits(np.stack([sw.config_stats(c) for c in range(NC)]), want_stats)
        sw.close()
        for cap in ("2", None):   # keep_segments 0: the segments stay on the device for score_device
            ctx.set_option("vad_seg_cap", cap)
            sw = fv.VadSweep(S, cfgs, n_channels=nch)
            sw.set_references(refs, scs)
            sw.keep_segments(False)
            run_parts(fv, ctx, sw, band, rms, N_CHUNKS, [0, 16, 64, 80, 176, 200])
            assert results(sw, S, NC, segments=False)[1:] == want[1:]
            with pytest.raises(fv.FvadError):
                sw.segments(0)
            sw.score_device(ctx)
            got = np.stack([sw.config_stats(c) for c in range(NC)])
            assert got.shape == (NC, S, 11)
            assert_bits(got, want_stats)   # every one of the 11 fields, as uint32
            sw.close()
    finally:
        ctx.set_option("vad_seg_cap", None)


def test_part_argument_rules(fv, gpu_ctx):
    ctx = gpu_ctx
    lib = fv.lib()
    cfgs = sweep_configs(8, seed=2)
    n_chunks = [64, 32]
    band, rms = make_inputs(fv, cfgs, n_chunks, 1, seed=9)
    d = ctx.device_alloc(band.nbytes)
    ctx.to_device(d, band)
    sw = fv.VadSweep(2, cfgs)
    other = None
    try:
        def part(first_chunk, n_part_chunks, nf=None, nc=None, h=None, c=None):
            f0 = first_chunk * CHUNK // FFT
            nf = nf or [max(0, min(frames_of(k), frames_of(first_chunk + n_part_chunks)) - f0) for k in n_chunks]
            nc = nc or [max(0, min(k, first_chunk + n_part_chunks) - first_chunk) for k in n_chunks]
            r = np.ascontiguousarray(rms[:, first_chunk:first_chunk + max(max(nc), 1)])
            return lib.fvad_vad_batch_run_device_part((c or ctx).h, (h or sw).h, fv.vp(d + f0 * 4), band.shape[2], (fv.sz * 2)(*nf),
                                                      fv.fptr(r), r.shape[1], (fv.sz * 2)(*nc), CHUNK, f0)
        INV = fv.FVAD_ERR_INVALID_ARGUMENT
        assert lib.fvad_vad_batch_score_device(ctx.h, sw.h) == INV     # no references (and no part state)
        assert part(0, 16) == 0
        assert part(16, 16) == 0
        # off a chunk boundary: first_frame 100
        r = np.ascontiguousarray(rms[:, 4:20])
        assert lib.fvad_vad_batch_run_device_part(ctx.h, sw.h, fv.vp(d), band.shape[2], (fv.sz * 2)(100, 100), fv.fptr(r), 16,
                                                  (fv.sz * 2)(16, 16), CHUNK, 100) == INV
        assert part(48, 16) == INV          # a gap
        assert part(16, 16) == INV          # an overlap
        assert part(0, 16) == 0 and part(16, 16) == 0    # (a fresh run, continued)
        # stream 1 ends in the part [32, 48) with fewer frames than stream 0 (its 32 chunks end at frame 750)
        assert part(32, 16, nf=[375, 0], nc=[16, 0]) == 0
        assert part(48, 16, nf=[375, 375], nc=[16, 16]) == INV   # frames for a stream that has ended
        assert part(48, 16, nf=[375, 0], nc=[16, 1]) == INV      # (chunks too)
        assert lib.fvad_vad_batch_score_device(ctx.h, sw.h) == INV   # still no references
        # another context
        other = fv.Context(0)
        other.load_synth(7)
        assert part(48, 16, nf=[375, 0], nc=[16, 0], c=other) == INV
        assert part(48, 16, nf=[375, 0], nc=[16, 0]) == 0
        # host and device parts do not mix, either way
        b16 = np.ascontiguousarray(band[:, :, 1125:1500])
        r16 = np.ascontiguousarray(rms[:, 64:80])
        assert lib.fvad_vad_batch_run_part(sw.h, fv.fptr(b16), 375, 375, fv.fptr(r16), 16, 16, CHUNK, 1500, 1) == INV
        b0 = np.ascontiguousarray(band[:, :, :375])
        r0 = np.ascontiguousarray(rms[:, :16])
        assert lib.fvad_vad_batch_run_part(sw.h, fv.fptr(b0), 375, 375, fv.fptr(r0), 16, 16, CHUNK, 0, 1) == 0
        assert sw.device_bytes() == 0       # the host run released the device state
        assert part(16, 16) == INV          # a device part after a host run
        # a one-shot device run releases the part state too
        assert part(0, 16) == 0 and sw.device_bytes() > 0
        sw.run_device(ctx, d, band.shape[2], [frames_of(k) for k in n_chunks], np.ascontiguousarray(rms), n_chunks)
        assert sw.device_bytes() == 0 and part(16, 16) == INV
    finally:
        sw.close()
        if other is not None:
            other.close()
        ctx.device_free(d)


def test_two_hour_stream_in_parts(fv, gpu_ctx):
    ctx = gpu_ctx
    cfgs = sweep_configs(16, seed=8)
    n_chunks = [14400]
    band, rms = make_inputs(fv, cfgs, n_chunks, 2, seed=33)
    one = fv.VadSweep(1, cfgs, n_channels=2)
    one_launch(fv, ctx, one, band, rms, n_chunks)
    want = results(one, 1, len(cfgs))
    one.close()
    bounds = list(range(0, 14400, 1808)) + [14400]
    assert len(bounds) == 9
    sw = fv.VadSweep(1, cfgs, n_channels=2)
    try:
        run_parts(fv, ctx, sw, band, rms, n_chunks, bounds)
        assert results(sw, 1, len(cfgs)) == want
        assert max(x[1] for per in want[0] for x in per[0]) > 1 << 24
    finally:
        sw.close()


GRID = {"base": {"speech_min_freq": 300, "speech_max_freq": 3000},
        "axes": {"speech_threshold_factor": [2.5, 4.0, 7.0], "initial_long_term_avg": [None, 0.3],
                 "min_vad_duration_sec": [0.2, 0.7]}}


def test_sliced_grid_equals_unsliced(fv, pkg, gpu_ctx, tmp_path):
    sim = pkg.simulator
    ctx = gpu_ctx
    streams = [(1, "pcm16", 47.3), (2, "f32", 61.1), (1, "f32", 33.9), (2, "pcm16", 20.2)]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plan = write_plan(pkg, tmp_path / "a", streams)
    plan2 = write_plan(pkg, tmp_path / "b", [(c, f, 2 * sec) for c, f, sec in streams])
    ctx.set_option("reproducible", "1")
    try:
        for vad_on, score_on in (("device", "device"), ("device", "host"), ("host", "host")):
            whole = sim.run_grid(plan, GRID, vad_on=vad_on, score_on=score_on, ctx=ctx, out=None)
            assert whole["slices"] == 1 and whole["device_bytes"] is None
            for n in (16, 48):
                sl = sim.run_grid(plan, GRID, vad_on=vad_on, score_on=score_on, ctx=ctx, out=None, slice_chunks=n)
                assert sl["slices"] > 1
                assert_bits(sl["stats"], whole["stats"])
                assert [r["config"] for r in sl["rows"]] == [r["config"] for r in whole["rows"]]
        # device and host memory follow the slice: twice as long instances, the same device_bytes
        for vad_on, score_on in (("device", "device"), ("device", "host")):
            a = sim.run_grid(plan, GRID, vad_on=vad_on, score_on=score_on, ctx=ctx, out=None, slice_chunks=16)
            b = sim.run_grid(plan2, GRID, vad_on=vad_on, score_on=score_on, ctx=ctx, out=None, slice_chunks=16)
            assert b["slices"] > a["slices"]
            assert a["device_bytes"] == b["device_bytes"] > 0
    finally:
        ctx.set_option("reproducible", None)
