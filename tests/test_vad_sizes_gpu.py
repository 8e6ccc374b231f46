"""Device VAD machines of several frame sizes in one launch (fvad_vad_batch_run_device_sized, _run_device_part_sized:
kernels_vad.hip's sized form) against the host machines (fvad_vad_batch_run_sized) and one create_sweep device run per size,
bit for bit -- ragged streams, 1 / 2 / 5 channels, both lane maps and lane orders, both ring forms, parts with segment
overflow, device scoring -- and simulator.run_grid over a grid with "fft_size" against one run_grid per size."""
import json

import numpy as np
import pytest

from test_vad_score_gpu import write_plan
from test_vad_score_host import make_labels, stat_cfgs_of
from test_vad_sizes_host import SIZES, bits, seg_bits, synth_sized
from test_vad_sweep_gpu import sweep_configs
from test_vad_sweep_host import CHUNK

pytestmark = pytest.mark.gpu

N_CHUNKS = [64, 12, 40, 1, 33]   # ragged: the streams end in different parts


def sized_configs(n, seed, long_short=False):
    cfgs = sweep_configs(n, seed)
    if long_short:   # short-term windows of 3 s: 282 slots at 512 points, the rings no longer fit in LDS
        for c in cfgs[::3]:
            c["short_term_speech_avg_sec"] = 3.0
    sizes = [SIZES[(i * 3 + i // 4) % len(SIZES)] for i in range(n)]
    return cfgs, sizes


def inputs(fv, cfgs, sizes, n_chunks, nch, seed):
    probe = fv.VadSweepSized(len(n_chunks), cfgs, sizes, n_channels=nch)
    bands, _ = probe.bands()
    probe.close()
    return synth_sized(len(n_chunks), nch, max(n_chunks), bands, seed)


def nf_of(sw, n_chunks):
    return [[k * CHUNK // F for k in n_chunks] for F in sw.sizes]


def results(sw, S, NC, segments=True):
    return ([sw.segments(c) for c in range(NC)] if segments else None,
            [[bits(sw.audit(s, c)) for c in range(NC)] for s in range(S)],
            [[sw.lazy_stats(s, c) for c in range(NC)] for s in range(S)])


def upload(ctx, arr):
    d = ctx.device_alloc(arr.nbytes)
    ctx.to_device(d, arr)
    return d


def host_results(fv, cfgs, sizes, band, rms, n_chunks, nch):
    """one host sized batch per stream (ragged lengths), in results()' shape"""
    NC, S = len(cfgs), len(n_chunks)
    segs = [[None] * S for _ in range(NC)]
    audits, lazy = [], []
    for s, k in enumerate(n_chunks):
        h = fv.VadSweepSized(1, cfgs, sizes, n_channels=nch)
        try:
            nf = [k * CHUNK // F for F in h.sizes]
            h.run(np.ascontiguousarray(band[:, s * nch:(s + 1) * nch, :max(max(nf), 1)]),
                  np.ascontiguousarray(rms[s * nch:(s + 1) * nch, :max(k, 1)]), nf, n_threads=8)
            for c in range(NC):
                segs[c][s] = h.segments(c)[0]
            audits.append([bits(h.audit(0, c)) for c in range(NC)])
            lazy.append([h.lazy_stats(0, c) for c in range(NC)])
        finally:
            h.close()
    return segs, audits, lazy


def per_size_device(fv, ctx, cfgs, sizes, band, rms, n_chunks, nch, bands_sized):
    """config c's results from a create_sweep device run at its size on the sized batch's band blocks"""
    S, out = len(n_chunks), {}
    for F in sorted(set(sizes)):
        idx = [c for c in range(len(cfgs)) if sizes[c] == F]
        ref = fv.VadSweep(S, [cfgs[c] for c in idx], n_channels=nch, fft_size=F)
        try:
            rbins, _ = ref.bands()
            blk = np.ascontiguousarray(np.stack([band[bands_sized.index((F, lo, hi))] for lo, hi in rbins]))
            d = upload(ctx, blk)
            try:
                ref.run_device(ctx, d, blk.shape[2], [k * CHUNK // F for k in n_chunks], rms, n_chunks)
            finally:
                ctx.device_free(d)
            segs, aud, lazy = results(ref, S, len(idx))
            for k, c in enumerate(idx):
                out[c] = (segs[k], [aud[s][k] for s in range(S)], [lazy[s][k] for s in range(S)])
        finally:
            ref.close()
    return out


def assert_same(got, want, NC, S):
    assert seg_bits(got[0]) == seg_bits(want[0])
    assert got[1] == want[1] and got[2] == want[2]


@pytest.mark.parametrize("nch,lane_map,order,long_short", [(1, None, None, False), (2, "config", None, False), (5, None, "caller", False),
                                                           (2, None, None, True), (1, "config", None, True)])
def test_one_shot_equals_host_and_per_size_runs(fv, gpu_ctx, nch, lane_map, order, long_short):
    ctx = gpu_ctx
    cfgs, sizes = sized_configs(20, 3 + nch, long_short)
    S, NC = len(N_CHUNKS), len(cfgs)
    band, rms = inputs(fv, cfgs, sizes, N_CHUNKS, nch, 5 + nch)
    ctx.set_option("vad_lane_map", lane_map)
    ctx.set_option("vad_size_order", order)
    sw = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    try:
        bands, _ = sw.bands()
        d = upload(ctx, band)
        try:
            sw.run_device(ctx, d, band.shape[2], nf_of(sw, N_CHUNKS), rms, N_CHUNKS)
        finally:
            ctx.device_free(d)
        got = results(sw, S, NC)
        assert_same(got, host_results(fv, cfgs, sizes, band, rms, N_CHUNKS, nch), NC, S)
        want = per_size_device(fv, ctx, cfgs, sizes, band, rms, N_CHUNKS, nch, bands)
        for c in range(NC):
            assert seg_bits([got[0][c]]) == seg_bits([want[c][0]]), c
            assert [got[1][s][c] for s in range(S)] == want[c][1] and [got[2][s][c] for s in range(S)] == want[c][2], c
        assert sum(len(x) for c in got[0] for x in c) > 20
    finally:
        sw.close()
        ctx.set_option("vad_lane_map", None)
        ctx.set_option("vad_size_order", None)


def run_parts(ctx, sw, band, rms, n_chunks, bounds):
    """sw over the parts [bounds[k], bounds[k + 1]) (in chunks, multiples of 32: a frame of every size), each part's band
    blocks uploaded on their own (the part's frames of each size from column 0)"""
    bands, _ = sw.bands()
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        s0 = c0 * CHUNK
        nf = [[max(0, min(k * CHUNK // F, c1 * CHUNK // F) - s0 // F) for k in n_chunks] for F in sw.sizes]
        nc = [max(0, min(k, c1) - c0) for k in n_chunks]
        w = max(max(max(r) for r in nf), 1)
        part = np.zeros((len(bands), band.shape[1], w), np.float32)
        for j, (F, _, _) in enumerate(bands):
            src = band[j, :, s0 // F:s0 // F + w]
            part[j, :, :src.shape[1]] = src
        prms = np.ascontiguousarray(rms[:, c0:c0 + max(max(nc), 1)])
        d = upload(ctx, part)
        try:
            sw.run_device_part(ctx, d, w, nf, prms, nc, s0)
        finally:
            ctx.device_free(d)


@pytest.mark.parametrize("nch,lane_map,seg_cap", [(1, None, 2), (2, "config", 3), (5, None, None)])
def test_parts_equal_one_launch(fv, gpu_ctx, nch, lane_map, seg_cap):
    ctx = gpu_ctx
    cfgs, sizes = sized_configs(12, 11 + nch, nch == 2)
    S, NC = len(N_CHUNKS), len(cfgs)
    band, rms = inputs(fv, cfgs, sizes, N_CHUNKS, nch, 13 + nch)
    one = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    parts = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    ctx.set_option("vad_lane_map", lane_map)
    try:
        d = upload(ctx, band)
        try:
            one.run_device(ctx, d, band.shape[2], nf_of(one, N_CHUNKS), rms, N_CHUNKS)
        finally:
            ctx.device_free(d)
        if seg_cap:   # a small room: machines of every size pause mid-part and go on
            ctx.set_option("vad_seg_cap", str(seg_cap))
        run_parts(ctx, parts, band, rms, N_CHUNKS, [0, 32, 64])
        assert_same(results(parts, S, NC), results(one, S, NC), NC, S)
        assert parts.device_bytes() > 0
        # the rules: a start off the grid of every size, and a start that is not where the last part ended
        nf = [[0] * S for _ in parts.sizes]
        z = np.zeros((S * nch, 1), np.float32)
        for s0 in (8 * CHUNK, 32 * CHUNK):
            with pytest.raises(fv.FvadError):
                parts.run_device_part(ctx, None, 1, nf, z, [0] * S, s0)
    finally:
        one.close()
        parts.close()
        ctx.set_option("vad_lane_map", None)
        ctx.set_option("vad_seg_cap", None)


def test_create_sweep_batch_takes_the_sized_device_calls(fv, gpu_ctx):
    """a create_sweep batch at 1024 points: run_device_sized equals run_device and run_device_part_sized in 16-chunk parts
    equals run_device_part, as raw bits; the shorter stream ends inside the second part"""
    ctx = gpu_ctx
    F, nch, n_chunks = 1024, 2, [24, 40]
    cfgs = sweep_configs(8, 41)
    S, NC = len(n_chunks), len(cfgs)
    sws = [fv.VadSweep(S, cfgs, n_channels=nch, fft_size=F) for _ in range(4)]
    frames, sized, frame_parts, sized_parts = sws
    try:
        bins, _ = frames.bands()
        band, rms = synth_sized(S, nch, max(n_chunks), [(F, lo, hi) for lo, hi in bins], 43)
        ends = [k * CHUNK // F for k in n_chunks]
        d = upload(ctx, band)
        try:
            frames.run_device(ctx, d, band.shape[2], ends, rms, n_chunks)
            sized.run_device_sized(ctx, d, band.shape[2], ends, rms, n_chunks)
        finally:
            ctx.device_free(d)
        want = results(frames, S, NC)
        assert_same(results(sized, S, NC), want, NC, S)
        assert sum(len(x) for c in want[0] for x in c) > 8
        for c0 in range(0, max(n_chunks), 16):
            c1 = min(c0 + 16, max(n_chunks))
            f0 = c0 * CHUNK // F
            nf = [max(0, min(e, c1 * CHUNK // F) - f0) for e in ends]
            nc = [max(0, min(k, c1) - c0) for k in n_chunks]
            part = np.ascontiguousarray(band[:, :, f0:f0 + max(nf)])
            prms = np.ascontiguousarray(rms[:, c0:c1])
            d = upload(ctx, part)
            try:
                frame_parts.run_device_part(ctx, d, part.shape[2], nf, prms, nc, f0)
                sized_parts.run_device_part_sized(ctx, d, part.shape[2], [nf] if c0 else nf, prms, nc, c0 * CHUNK)
            finally:
                ctx.device_free(d)
        assert 16 < n_chunks[0] < 32   # (it ended inside the second part)
        assert_same(results(frame_parts, S, NC), want, NC, S)
        assert_same(results(sized_parts, S, NC), want, NC, S)
    finally:
        for sw in sws:
            sw.close()


def test_device_scoring_one_shot_and_parts(fv, gpu_ctx):
    ctx = gpu_ctx
    nch = 2
    cfgs, sizes = sized_configs(16, 21)
    S, NC = len(N_CHUNKS), len(cfgs)
    band, rms = inputs(fv, cfgs, sizes, N_CHUNKS, nch, 22)
    rng = np.random.default_rng(23)
    refs = [make_labels(rng, k * CHUNK / 48000.0, 12, "mixed") for k in N_CHUNKS]
    scs = stat_cfgs_of(cfgs, 24)
    dev = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    dparts = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    host = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    try:
        for sw in (dev, dparts):
            sw.set_references(refs, scs)
            sw.keep_segments(False)
        d = upload(ctx, band)
        try:
            dev.run_device(ctx, d, band.shape[2], nf_of(dev, N_CHUNKS), rms, N_CHUNKS)
            host.run_device(ctx, d, band.shape[2], nf_of(host, N_CHUNKS), rms, N_CHUNKS)   # (keeps its segments)
        finally:
            ctx.device_free(d)
        run_parts(ctx, dparts, band, rms, N_CHUNKS, [0, 32, 64])
        dparts.score_device(ctx)
        host.set_references(refs, scs)
        host.score(8)
        for c in range(NC):
            want = host.config_stats(c).view(np.uint32)
            assert np.array_equal(dev.config_stats(c).view(np.uint32), want), c
            assert np.array_equal(dparts.config_stats(c).view(np.uint32), want), c
    finally:
        dev.close()
        dparts.close()
        host.close()


def test_two_hour_stream_512_and_2048(fv, gpu_ctx):
    ctx = gpu_ctx
    cfgs = [{}, {"long_term_speech_avg_sec": 30.0, "has_initial_long_term_avg": 0, "speech_threshold_factor": 3.0}] * 2
    sizes = [512, 512, 2048, 2048]
    n = [2 * 3600 * 2]   # two hours of 0.5 s chunks
    band, rms = inputs(fv, cfgs, sizes, n, 1, 31)
    sw = fv.VadSweepSized(1, cfgs, sizes)
    try:
        d = upload(ctx, band)
        try:
            sw.run_device(ctx, d, band.shape[2], nf_of(sw, n), rms, n)
        finally:
            ctx.device_free(d)
        got = results(sw, 1, len(cfgs))
        assert_same(got, host_results(fv, cfgs, sizes, band, rms, n, 1), len(cfgs), 1)
        assert all(got[0][c][0] and got[0][c][0][-1][1] > 2 ** 24 for c in (1, 3))   # (sample indices past f32's exact integers)
    finally:
        sw.close()


# ------------------------------------------------------------------ run_grid
GRID = {"base": {"max_speech_gap_sec": 1.0}, "axes": {"speech_threshold_factor": [2.0, 4.0, 8.0], "speech_min_freq": [300.0, 500.0]}}


def _stats_bits(res):
    return res["stats"].view(np.uint32)


@pytest.mark.parametrize("mode", ["device", "host", "sliced"])
def test_run_grid_sizes_equal_one_run_per_size(pkg, fv, gpu_ctx, tmp_path, mode):
    sim = pkg.simulator
    ctx = gpu_ctx
    streams = [(2, "pcm16", 35.0), (1, "f32", 22.5), (2, "pcm16", 16.5)]   # (channels, format, seconds): three slices of 32 chunks
    sizes = [512, 1024, 2048]
    kw = {"vad_on": "host" if mode == "host" else "device", "out": None, "ctx": ctx}
    if mode == "sliced":
        kw["slice_chunks"] = 32
        ctx.set_option("reproducible", "1")
    try:
        plan = write_plan(pkg, tmp_path, streams)
        res = sim.run_grid(plan, dict(GRID, fft_size=sizes), json_path=str(tmp_path / "rows.json"), **kw)
        n = len(sim.expand_grid(GRID))
        assert [r["fft_size"] for r in res["rows"]] == [F for F in sizes for _ in range(n)]
        rows = json.load(open(tmp_path / "rows.json"))["rows"]
        assert [r["fft_size"] for r in rows] == [F for F in sizes for _ in range(n)]
        for g, F in enumerate(sizes):
            p = json.load(open(plan))
            p.setdefault("config", {}).setdefault("vad_config", {})["fft_size"] = F
            (tmp_path / f"plan{F}.json").write_text(json.dumps(p))
            one = sim.run_grid(str(tmp_path / f"plan{F}.json"), GRID, **kw)
            assert np.array_equal(_stats_bits(res)[g * n:(g + 1) * n], _stats_bits(one)), F
            for r, w in zip(res["rows"][g * n:(g + 1) * n], one["rows"]):
                assert r["config"] - g * n == w["config"]
                assert np.float32(r["F"]).view(np.uint32) == np.float32(w["F"]).view(np.uint32)
    finally:
        if mode == "sliced":
            ctx.set_option("reproducible", None)
