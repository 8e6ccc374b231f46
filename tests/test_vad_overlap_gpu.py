"""Device parts that do not wait (fvad_vad_batch_run_device_part_async + fvad_vad_batch_part_wait, kernels_vadratio.hip) on
reproducible contexts, every comparison exact: the device's frame ratios against the host's and the oracle's chain; async parts
against the blocking parts and one launch (segments, audits, lazy statistics, device-held scores; both ring forms and lane maps, a
sized batch, streams that end early, a segment room of two); an engine call between the two calls; the in-flight rules; one case
straight against orc_vad; and simulator.run_grid(overlap=True) against overlap=False."""
import numpy as np
import pytest

import vad_oracle_cases as V
from test_vad_grid_devices_gpu import SIZED, STREAMS
from test_vad_oracle_gpu import assert_machine, upload
from test_vad_oracle_host import cases  # noqa: F401  (the module-scoped oracle pipeline runs)
from test_vad_overlap_host import CASES, CASE_IDS, bits, case_tables, lanes_of, part_starts
from test_vad_parts_gpu import N_CHUNKS, frames_of, host_results, make_inputs, one_launch, results, run_parts
from test_vad_retain_gpu import GRID
from test_vad_score_gpu import assert_bits, write_plan
from test_vad_score_host import make_labels, stat_cfgs_of
from test_vad_sweep_gpu import sweep_configs
from test_vad_sweep_host import CHUNK, FS

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.set_option("reproducible", "1")
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_option("reproducible", None)


# ------------------------------------------------------------------ the ratio kernel

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_device_ratios_equal_host_and_oracle(fv, ctx, case):
    rate, nch, F = case
    chunk, n_chunks, tables = case_tables(rate, nch, F)
    whole = [V.oracle_frame_ratios(t, k * chunk // F, F, chunk) for t, k in zip(tables, n_chunks)]
    sw = fv.VadSweep(2, V.case_configs(rate, F, seed=1)[:2], n_channels=nch, sample_rate=rate, fft_size=F)
    try:
        for start in part_starts(chunk, F, max(n_chunks)):
            f0 = start * chunk // F
            nc = [max(0, k - start) for k in n_chunks]
            nf = [max(0, k * chunk // F - f0) for k in n_chunks]
            rms = lanes_of(tables, start, max(nc))
            host = sw.frame_ratios(rms, nf, nc, first_sample=start * chunk, chunk_size=chunk)
            stride = max(nf) + 3
            got = np.full((2, stride), np.nan, np.float32)
            d_rms, d_out = upload(ctx, rms), upload(ctx, got)
            try:
                sw.frame_ratios_device(ctx, d_rms, rms.shape[1], nf, nc, start * chunk, d_out, stride, chunk_size=chunk)
                ctx.to_host(got, d_out)
            finally:
                ctx.device_free(d_rms)
                ctx.device_free(d_out)
            for s in range(2):
                assert np.array_equal(bits(got[s, :nf[s]]), bits(host[s, :nf[s]])), (case, start, s)
                assert np.array_equal(bits(got[s, :nf[s]]), bits(whole[s][f0:f0 + nf[s]])), (case, start, s)
                assert np.all(got[s, nf[s]:max(nf)] == 0) and np.all(np.isnan(got[s, max(nf):]))   # nothing past the longest row
    finally:
        sw.close()


# ------------------------------------------------------------------ async parts against blocking parts and one launch

def run_parts_async(fv, ctx, sw, band, rms, n_chunks, bounds, between=None):
    """run_parts (test_vad_parts_gpu) with the RMS on the device and every part started and then waited for"""
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        f0, f1 = frames_of(c0), frames_of(c1)
        nf = [max(0, min(frames_of(k), f1) - f0) for k in n_chunks]
        nc = [max(0, min(k, c1) - c0) for k in n_chunks]
        part = np.ascontiguousarray(band[:, :, f0:f0 + max(max(nf), 1)])
        prms = np.ascontiguousarray(rms[:, c0:c0 + max(max(nc), 1)])
        d, r = upload(ctx, part), upload(ctx, prms)
        try:
            sw.run_device_part_async(ctx, d, part.shape[2], nf, r, prms.shape[1], nc, c0 * CHUNK)
            if between:
                between()
            sw.part_wait(ctx)
        finally:
            ctx.device_free(d)
            ctx.device_free(r)


@pytest.mark.parametrize("lane_map", [None, "config"])
@pytest.mark.parametrize("long_short_term", [False, True])
def test_async_parts_equal_blocking_parts_and_one_launch(fv, ctx, lane_map, long_short_term):
    """ragged streams (they end in different parts), both lane maps, the rings in LDS and in global memory (a 5 s short-term
    window), segments kept on the host part after part"""
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
            blocking = fv.VadSweep(S, cfgs, n_channels=nch)
            sw = fv.VadSweep(S, cfgs, n_channels=nch)
            try:
                run_parts(fv, ctx, blocking, band, rms, N_CHUNKS, bounds)
                run_parts_async(fv, ctx, sw, band, rms, N_CHUNKS, bounds)
                assert results(sw, S, NC) == results(blocking, S, NC) == want
                assert sw.device_bytes() == blocking.device_bytes() > 0
            finally:
                blocking.close()
                sw.close()
    finally:
        ctx.set_option("vad_lane_map", None)
    assert sum(len(x) for per in want[0] for x in per) > 100


def test_async_parts_grow_their_room_and_score_on_the_device(fv, ctx):
    """two segments of room per machine: fvad_vad_batch_part_wait grows the room and relaunches, part after part; then the
    segments left on the device scored there"""
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
    assert host_results(fv, cfgs, band, rms, N_CHUNKS, nch) == want
    bounds = list(range(0, 200, 16)) + [200]
    try:
        for cap in ("2", None):
            ctx.set_option("vad_seg_cap", cap)
            sw = fv.VadSweep(S, cfgs, n_channels=nch)
            run_parts_async(fv, ctx, sw, band, rms, N_CHUNKS, bounds)
            assert results(sw, S, NC) == want, cap
            sw.close()
            sw = fv.VadSweep(S, cfgs, n_channels=nch)
            sw.set_references(refs, scs)
            sw.keep_segments(False)
            run_parts_async(fv, ctx, sw, band, rms, N_CHUNKS, [0, 16, 64, 80, 176, 200])
            assert results(sw, S, NC, segments=False)[1:] == want[1:]
            sw.score_device(ctx)
            assert_bits(np.stack([sw.config_stats(c) for c in range(NC)]), want_stats)
            sw.close()
    finally:
        ctx.set_option("vad_seg_cap", None)


def sized_part(band, sizes, bands, c0, c1, n_chunks):
    """the band blocks [n_bands][lanes][stride] of chunks [c0, c1) of a sized batch (band[F]: [lanes][frames]) and n_frames
    [size][stream]"""
    nf = [[max(0, min(k, c1) * CHUNK // F - min(k, c0) * CHUNK // F) for k in n_chunks] for F in sizes]
    stride = max(max(max(row) for row in nf), 1)
    out = np.zeros((len(bands), band[sizes[0]].shape[0], stride), np.float32)
    for j, (F, _, _) in enumerate(bands):
        n = (c1 - c0) * CHUNK // F
        piece = band[F][:, c0 * CHUNK // F:c0 * CHUNK // F + n]
        out[j, :, :piece.shape[1]] = piece * np.float32(1 + 0.1 * j)
    return out, nf


def test_async_parts_of_a_sized_batch(fv, ctx):
    """three frame clocks in one batch, two streams of different length, parts every 32 chunks (where a frame of every size
    starts)"""
    sizes_of = [512, 1024, 2048, 1024, 512, 2048]
    cfgs = sweep_configs(len(sizes_of), seed=6)
    n_chunks, nch = [160, 70], 2
    rng = np.random.default_rng(8)
    rms = rng.uniform(0.01, 0.2, (2 * nch, max(n_chunks))).astype(np.float32)
    band = {}
    for F in sorted(set(sizes_of)):
        n = max(n_chunks) * CHUNK // F
        t = np.arange(n) * F / FS
        burst = (np.sin(2 * np.pi * t / 7.0) > 0.3).astype(np.float32)
        band[F] = (0.002 + 0.3 * burst[None] * rng.uniform(0.5, 1.0, (2 * nch, n))).astype(np.float32)

    def run(how, bounds):
        sw = fv.VadSweepSized(2, cfgs, sizes_of, n_channels=nch)
        bands, _ = sw.bands()
        try:
            for c0, c1 in zip(bounds[:-1], bounds[1:]):
                blk, nf = sized_part(band, sw.sizes, bands, c0, c1, n_chunks)
                nc = [max(0, min(k, c1) - c0) for k in n_chunks]
                prms = np.ascontiguousarray(rms[:, c0:c1])
                d = upload(ctx, blk)
                try:
                    if how == "one":
                        sw.run_device(ctx, d, blk.shape[2], nf, prms, nc)
                    elif how == "blocking":
                        sw.run_device_part(ctx, d, blk.shape[2], nf, prms, nc, c0 * CHUNK)
                    else:
                        r = upload(ctx, prms)
                        try:
                            sw.run_device_part_async(ctx, d, blk.shape[2], nf, r, prms.shape[1], nc, c0 * CHUNK)
                            sw.part_wait(ctx)
                        finally:
                            ctx.device_free(r)
                finally:
                    ctx.device_free(d)
            return results(sw, 2, len(cfgs))
        finally:
            sw.close()

    want = run("one", [0, 160])
    assert sum(len(x) for per in want[0] for x in per) > 20
    bounds = [0, 32, 64, 128, 160]
    assert run("blocking", bounds) == want
    assert run("async", bounds) == want


# ------------------------------------------------------------------ beside the engine, and the rules while a part is in flight

def test_engine_call_between_async_and_wait(fv, ctx):
    """fvad_engine_enqueue_device queued while the part is in flight: the denoised audio, band sums and RMS of the engine call and
    the results of the part are what each gives alone"""
    cfgs = sweep_configs(64, seed=3)
    S, NC, nch = len(N_CHUNKS), len(cfgs), 2
    band, rms = make_inputs(fv, cfgs, N_CHUNKS, nch, seed=21)
    rng = np.random.default_rng(2)
    L, n = 6, 24 * CHUNK
    pcm = (0.05 * rng.standard_normal((L, n))).astype(np.float32)
    d_pcm = upload(ctx, pcm)
    d_den, d_band, d_rms = ctx.device_alloc(pcm.nbytes), ctx.device_alloc(L * (n // 1024 + 1) * 4), ctx.device_alloc(L * 24 * 4)

    def engine():
        ctx.enqueue_device(d_pcm, L, n, n, d_den, d_band, d_rms)
        return tuple(ctx.to_host(np.empty(shape, np.float32), a).copy()
                     for shape, a in (((L, n), d_den), ((L, n // 1024), d_band), ((L, 24), d_rms)))

    try:
        alone = engine()
        blocking = fv.VadSweep(S, cfgs, n_channels=nch)
        bounds = [0, 48, 96, 200]
        run_parts(fv, ctx, blocking, band, rms, N_CHUNKS, bounds)
        want = results(blocking, S, NC)
        blocking.close()
        beside = []
        sw = fv.VadSweep(S, cfgs, n_channels=nch)
        try:
            run_parts_async(fv, ctx, sw, band, rms, N_CHUNKS, bounds, between=lambda: beside.append(engine()))
            assert results(sw, S, NC) == want
        finally:
            sw.close()
        assert len(beside) == 3
        for got in beside:
            for a, b in zip(got, alone):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        for a in (d_pcm, d_den, d_band, d_rms):
            ctx.device_free(a)


def test_rules_while_a_part_is_in_flight(fv, ctx):
    lib = fv.lib()
    INV = fv.FVAD_ERR_INVALID_ARGUMENT
    cfgs = sweep_configs(8, seed=2)
    n_chunks = [64, 32]
    band, rms = make_inputs(fv, cfgs, n_chunks, 1, seed=9)
    d, r = upload(ctx, band), upload(ctx, np.ascontiguousarray(rms))
    rng = np.random.default_rng(1)
    refs = [make_labels(rng, k * CHUNK / FS, 4, "mixed") for k in n_chunks]
    scs = stat_cfgs_of(cfgs, 4)
    blocking = fv.VadSweep(2, cfgs)
    run_parts(fv, ctx, blocking, band, rms, n_chunks, [0, 16, 32, 64])
    want = results(blocking, 2, len(cfgs))
    blocking.close()
    sw = fv.VadSweep(2, cfgs)
    other = None

    def start(c0, c1, c=None):
        f0 = frames_of(c0)
        nf = (fv.sz * 2)(*[max(0, min(frames_of(k), frames_of(c1)) - f0) for k in n_chunks])
        nc = (fv.sz * 2)(*[max(0, min(k, c1) - c0) for k in n_chunks])
        return lib.fvad_vad_batch_run_device_part_async((c or ctx).h, sw.h, fv.vp(d + f0 * 4), band.shape[2], nf, fv.vp(r + c0 * 4),
                                                        rms.shape[1], nc, CHUNK, c0 * CHUNK)

    try:
        sw.set_references(refs, scs)
        other = fv.Context(0)
        other.load_synth(7)
        assert start(16, 32) == INV                     # no part to continue
        assert start(0, 16, c=other) == 0 and lib.fvad_vad_batch_part_wait(other.h, sw.h) == 0   # (any context starts a run)
        assert start(0, 16) == 0
        # ---- in flight: every other call on the batch is refused and leaves it as it is
        nf, nc = (fv.sz * 2)(375, 375), (fv.sz * 2)(16, 16)
        hr = np.ascontiguousarray(rms[:, 16:32])
        hb = np.ascontiguousarray(band[:, :, 375:750])
        assert start(16, 32) == INV                     # a second part
        assert lib.fvad_vad_batch_run_device_part(ctx.h, sw.h, fv.vp(d + 375 * 4), band.shape[2], nf, fv.fptr(hr), 16, nc, CHUNK, 375) == INV
        assert lib.fvad_vad_batch_run_device_part_sized(ctx.h, sw.h, fv.vp(d + 375 * 4), band.shape[2], nf, fv.fptr(hr), 16, nc, CHUNK,
                                                        375 * 1024) == INV
        assert lib.fvad_vad_batch_run_device(ctx.h, sw.h, fv.vp(d), band.shape[2], nf, fv.fptr(hr), 16, nc, CHUNK) == INV
        assert lib.fvad_vad_batch_run_part(sw.h, fv.fptr(hb), 375, 375, fv.fptr(hr), 16, 16, CHUNK, 375, 1) == INV
        assert lib.fvad_vad_batch_run(sw.h, fv.fptr(hb), 375, 375, fv.fptr(hr), 16, 16, CHUNK, 1) == INV
        assert lib.fvad_vad_batch_score(sw.h, 1) == INV
        assert lib.fvad_vad_batch_score_device(ctx.h, sw.h) == INV
        assert lib.fvad_vad_batch_retain_configs(ctx.h, sw.h, (fv.C.c_uint32 * 2)(0, 1), 2) == INV
        assert lib.fvad_vad_batch_set_keep_segments(sw.h, 0) == INV
        assert lib.fvad_vad_batch_total_segments(sw.h) == fv.sz(-1).value
        for call in (lambda: sw.segments(0), lambda: sw.audit(0, 0), lambda: sw.lazy_stats(0, 0), lambda: sw.config_stats(0),
                     lambda: sw.set_references(refs, scs)):
            with pytest.raises(fv.FvadError):
                call()
        assert lib.fvad_vad_batch_part_wait(other.h, sw.h) == INV   # the wrong context
        assert sw.n_configs == lib.fvad_vad_batch_n_configs(sw.h) == len(cfgs)   # (what the batch is can still be asked)
        ctx.synchronize()                               # waits for what the part has queued, too
        sw.part_wait(ctx)
        sw.part_wait(ctx)                               # nothing in flight
        # ---- and on it goes, to the blocking parts' results
        assert start(16, 32) == 0
        ctx.synchronize()
        sw.part_wait(ctx)
        assert start(32, 64) == 0
        sw.part_wait(ctx)
        assert results(sw, 2, len(cfgs)) == want
        # ---- destroyed with a part in flight
        assert start(0, 64) == 0
        sw.close()
        ctx.synchronize()
    finally:
        sw.close()
        if other is not None:
            other.close()
        ctx.device_free(d)
        ctx.device_free(r)


# ------------------------------------------------------------------ straight against orc_vad

@pytest.mark.parametrize("case", [(48000, 2, 2048), (16000, 2, 16384)], ids=["48k-2ch-F2048", "16k-2ch-F16384"])
def test_async_parts_equal_oracle_machines(fv, ctx, cases, case):  # noqa: F811
    """the oracle pipeline's band sums and RMS, orc_vad's machines fed the oracle's frame ratios: frames across two and across
    three chunks, parts at chunk-and-frame boundaries, two segments of room"""
    o = cases[case]
    rate, nch, F = case
    chunk = o["chunk"]
    cfgs = V.case_configs(rate, F, seed=F + nch)
    probe = fv.VadSweep(1, cfgs, n_channels=nch, sample_rate=rate, fft_size=F)
    bins, band_of = probe.bands()
    probe.close()
    band = V.band_blocks(o["bins"], bins)
    rms = np.ascontiguousarray(o["rms"].T)
    nf, nc = band.shape[2], rms.shape[1]
    want = V.oracle_machines([(c, rate, nch, F, band[band_of[i]], o["ratio"]) for i, c in enumerate(cfgs)])
    step = int(np.lcm(chunk, F)) // chunk
    cuts = [k * step for k in range(1, 4) if k * step < nc] + [nc]
    ctx.set_option("vad_seg_cap", "2")
    try:
        sw = fv.VadSweep(1, cfgs, n_channels=nch, sample_rate=rate, fft_size=F)
        d_rms = upload(ctx, rms)
        c0 = 0
        try:
            for c1 in cuts:
                f0, f1 = c0 * chunk // F, min(nf, c1 * chunk // F)
                pb = np.ascontiguousarray(band[:, :, f0:max(f1, f0 + 1)])
                d = upload(ctx, pb)
                try:
                    sw.run_device_part_async(ctx, d, pb.shape[2], [f1 - f0], d_rms + c0 * 4, nc, [c1 - c0], c0 * chunk, chunk_size=chunk)
                    sw.part_wait(ctx)
                finally:
                    ctx.device_free(d)
                c0 = c1
        finally:
            ctx.device_free(d_rms)
        for c in range(len(cfgs)):
            assert_machine(sw, 0, c, want[c], (case, cuts, c, cfgs[c]))
        sw.close()
    finally:
        ctx.set_option("vad_seg_cap", None)


# ------------------------------------------------------------------ the harness

GRIDS = {
    "plain": (GRID, dict(slice_chunks=16)),
    "sized": (SIZED, dict(slice_chunks=32)),
    "halving": (GRID, dict(slice_chunks=16, halving_eta=2, halving_rungs=2)),
}


def assert_same_grid(a, b, halving):
    assert_bits(b["stats"], a["stats"])
    assert [r["config"] for r in b["rows"]] == [r["config"] for r in a["rows"]]
    assert b["slices"] == a["slices"]
    if halving:
        for k in ("survivors", "rung", "evaluated_seconds"):
            assert b[k] == a[k], k
        assert [(g["rung"], g["end_chunk"], g["configs_in"], g["configs_kept"]) for g in b["rung_times"]] == \
               [(g["rung"], g["end_chunk"], g["configs_in"], g["configs_kept"]) for g in a["rung_times"]]


@pytest.mark.parametrize("name", list(GRIDS))
def test_grid_with_overlap_equals_without(pkg, ctx, tmp_path, name):
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, STREAMS)   # mono and stereo, PCM16 and f32, different lengths
    grid, kw = GRIDS[name]
    off = sim.run_grid(plan, grid, ctx=ctx, out=None, vad_on="device", score_on="device", **kw)
    on = sim.run_grid(plan, grid, ctx=ctx, out=None, vad_on="device", score_on="device", overlap=True, **kw)
    assert_same_grid(off, on, "halving_eta" in kw)
    assert "machines_wait" in on["times"] and "machines_wait" not in off["times"]
    assert on["device_bytes"] > off["device_bytes"] > 0   # the second set of bands and rms


def test_two_shares_with_overlap_equal_one_context_without(fv, pkg, ctx, tmp_path):
    sim = pkg.simulator
    plan = write_plan(pkg, tmp_path, STREAMS)
    other = fv.Context(0)
    try:
        other.load_synth(7)
        other.set_option("reproducible", "1")
        grid, kw = GRIDS["halving"]
        off = sim.run_grid(plan, grid, ctx=ctx, out=None, vad_on="device", score_on="device", **kw)
        on = sim.run_grid(plan, grid, ctx=[ctx, other], out=None, vad_on="device", score_on="device", overlap=True, **kw)
        assert_bits(on["stats"], off["stats"])
        for k in ("survivors", "rung", "evaluated_seconds"):
            assert on[k] == off[k], k
        assert [t["instances"] for t in on["share_times"]] == [[0, 2], [1, 3]]
        assert all("machines_wait" in t["times"] for t in on["share_times"])
    finally:
        other.close()
