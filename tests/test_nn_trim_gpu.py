"""The work the persistent f32 kernels skip (context option nn_trim) changes no bit.

"tiles": fc2 / fc3 issue no MFMAs for the all-padding 39th column tile of their third column block.
"rows":  layer 1's input projection computes rows 4..53 of every chunk (and rows 0..3 of the first chunk of every lane in a
         small launch of the same kernel); gru_rec3 reads the other chunks' rows 0..3 from their predecessor's rows 50..53.
         Launches whose lanes do not all have the same number of chunks compute all 54 rows
         (fvad_ctx_last_nn_path does not end in "gi1 rows 4..53").

Every engine case runs with nn_trim "all" and with "none" (the untrimmed kernels' code path: the yardstick) and the outputs
-- denoised audio, band sums, chunk RMS; the denoised audio is the gains applied (the layers themselves are judged through
fvad_ctx_nn_tap in test_nn_layers_gpu.py) -- are
compared as uint32; "all" is also compared with the oracle pipeline on the same samples (denoised 1e-4 of peak, band sums
and RMS 1e-4 relative, segments exact).  The gains themselves are compared through fvad_nsnet2_forward.
All under option reproducible: persistent GEMM + gru_rec3 at every launch size, batches padded to 128 sequences.
"""
import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

CHUNK = 24000
TRIMMED = "gi1 rows 4..53"


def _stream(pkg, n_chunks, seed):
    pcm, _ = pkg.synth.make_stream(n_chunks * 0.5 + 0.1, seed=seed)
    return pcm[0][: n_chunks * CHUNK].copy()


@pytest.fixture(scope="module")
def streams(pkg):
    """lanes of 1, 2, 5 and 70 chunks, and four of 70 (70 > 64: a chunk's predecessor belongs to another workgroup of
    gru_rec3<4>; neither lane count is a multiple of 64: the launch of the first chunks' rows is padded)"""
    ragged = [_stream(pkg, n, 500 + n) for n in (1, 2, 5, 70)]
    uniform = [ragged[3]] + [_stream(pkg, 70, 600 + i) for i in range(3)]
    return {"ragged": ragged, "uniform": uniform}


_oracle_cache = {}


def _oracle(weights, x):
    key = (x.shape[0], float(x[:1000].sum()), float(x[-1000:].sum()))
    if key not in _oracle_cache:
        p = orc.Pipeline(weights, n_channels=1, keep_denoised=True)
        p.push(x[None])
        _oracle_cache[key] = {"den": p.denoised()[0].copy(), "band": p.band_volumes()[:, 0].copy(), "rms": p.chunk_rms()[:, 0].copy(),
                              "segs": [(s[0], s[1]) for s in p.segments()]}
    return _oracle_cache[key]


def _segments(fv, band, rms):
    """the host stage on the engine's band sums and chunk RMS (one channel)"""
    n_frames = band.shape[0]
    ratio = np.where(rms > 0, np.where(rms < 1, 1.0, 1.0 / np.maximum(rms, 1e-30)), 0.0).astype(np.float32)
    fs = np.arange(n_frames) * 1024
    c0, c1 = fs // CHUNK, np.minimum((fs + 1023) // CHUNK, len(rms) - 1)
    w0 = (np.minimum((c0 + 1) * CHUNK, fs + 1024) - fs).astype(np.float32)
    w1 = np.float32(1024) - w0
    rat = ((ratio[c0] * w0 + np.where(w1 > 0, ratio[c1] * w1, np.float32(0))) / (w0 + w1)).astype(np.float32)
    m = fv.VadMachine()
    fv.vad_run_many([m], [band[:, None]], [rat], n_threads=1)
    segs = [(s[0], s[1]) for s in m.segments()]
    m.close()
    return segs


def _assert_oracle(fv, weights, lanes, out, what):
    for i, (x, o) in enumerate(zip(lanes, out)):
        ref = _oracle(weights, x)
        den, band, rms = o["denoised"], o["band_sum"], o["chunk_rms"]
        assert den.shape == ref["den"].shape and np.all(np.isfinite(den)), (what, i)
        peak = np.abs(ref["den"]).max()
        err = np.abs(den.astype(np.float64) - ref["den"]).max() / peak
        eb = (np.abs(band.astype(np.float64) - ref["band"]) / np.abs(ref["band"])).max()
        er = (np.abs(rms.astype(np.float64) - ref["rms"]) / np.abs(ref["rms"])).max()
        print(f"{what} lane {i}: denoised {err:.3e} of peak, band sums {eb:.3e}, rms {er:.3e}")
        assert err <= 1e-4 and eb <= 1e-4 and er <= 1e-4, (what, i, err, eb, er)
        assert _segments(fv, band, rms) == ref["segs"], (what, i)


def _same_bits(a, b, what):
    for i, (p, q) in enumerate(zip(a, b)):
        for k in ("denoised", "band_sum", "chunk_rms"):
            x, y = np.ascontiguousarray(p[k]), np.ascontiguousarray(q[k])
            assert x.shape == y.shape and np.all(np.isfinite(x)), (what, i, k)
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, i, k, int((x.view(np.uint32) != y.view(np.uint32)).sum()))


def _run(ctx, lanes, trim, **kw):
    with ctx.options(reproducible="1", nn_trim=trim):
        out = ctx.engine_run([x.copy() for x in lanes], want_denoised=True, **kw)
        return out, ctx.last_nn_path()


_off_cache = {}


def _off(ctx, name, lanes, **kw):
    """the untrimmed run of a case, computed once"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _off_cache:
        out, path = _run(ctx, lanes, "none", **kw)
        assert "panel_gemm3" in path and "gru_rec3" in path and TRIMMED not in path, path
        _off_cache[key] = out
    return _off_cache[key]


def test_one_lane_of_one_chunk(fv, gpu_ctx, weights7, streams):
    lanes = streams["ragged"][:1] # every sequence is `first`: all four warm-up rows come from the second launch
    on, path = _run(gpu_ctx, lanes, "all")
    assert TRIMMED in path, path
    _same_bits(on, _off(gpu_ctx, "one", lanes), "1 x 1")
    _assert_oracle(fv, weights7, lanes, on, "1 x 1")


def test_ragged_lanes_compute_all_rows(fv, gpu_ctx, weights7, streams):
    lanes = streams["ragged"]
    on, path = _run(gpu_ctx, lanes, "all")
    assert "panel_gemm3" in path and TRIMMED not in path, path # lanes of 1, 2, 5, 70 chunks: the untrimmed projection ran
    _same_bits(on, _off(gpu_ctx, "ragged", lanes), "ragged")
    _assert_oracle(fv, weights7, lanes, on, "ragged")


def test_uniform_lanes_are_trimmed(fv, gpu_ctx, weights7, streams):
    lanes = streams["uniform"]
    on, path = _run(gpu_ctx, lanes, "all")
    assert TRIMMED in path, path
    _same_bits(on, _off(gpu_ctx, "uniform", lanes), "4 x 70")
    _assert_oracle(fv, weights7, lanes, on, "4 x 70")


@pytest.mark.parametrize("trim", ["tiles", "rows"])
def test_each_half_alone(gpu_ctx, streams, trim):
    lanes = streams["uniform"]
    on, path = _run(gpu_ctx, lanes, trim)
    assert (TRIMMED in path) == (trim == "rows"), path
    _same_bits(on, _off(gpu_ctx, "uniform", lanes), trim)


@pytest.mark.parametrize("name,cap", [("ragged", 40), ("uniform", 35), ("uniform", 100)])
def test_lane_cut_between_launches(gpu_ctx, streams, name, cap):
    # a lane cut mid-way: its continuing chunk is `first` in the next launch and takes the carry's rows.  uniform / 35: eight
    # trimmed launches of one lane's 35 chunks; uniform / 100 and ragged / 40: launches of 70 + 30, 30 + 40 + 30, ... chunks
    # whose lanes differ (all 54 rows) next to launches of one lane (trimmed)
    lanes = streams[name]
    on, path = _run(gpu_ctx, lanes, "all", max_chunks_per_launch=cap)
    assert "panel_gemm3" in path, path
    if (name, cap) == ("uniform", 35):
        assert TRIMMED in path, path
    _same_bits(on, _off(gpu_ctx, name, lanes), (name, cap))


def test_streaming_equals_one_shot(fv, gpu_ctx, streams):
    # the same lanes in two calls through fvad_lane_state: the second call's first chunks take the carry's rows
    lanes = streams["uniform"]
    whole = _off(gpu_ctx, "uniform", lanes)
    sts = [gpu_ctx.lane_state() for _ in lanes]
    try:
        a, pa = _run(gpu_ctx, [x[: 33 * CHUNK] for x in lanes], "all", states=sts)
        b, pb = _run(gpu_ctx, [x[33 * CHUNK:] for x in lanes], "all", states=sts)
    finally:
        for st in sts:
            fv.lib().fvad_lane_state_destroy(st)
    assert TRIMMED in pa and TRIMMED in pb, (pa, pb)
    joined = [{k: np.concatenate([p[k], q[k]]) for k in ("denoised", "band_sum", "chunk_rms")} for p, q in zip(a, b)]
    _same_bits(joined, whole, "two calls")


def test_enqueue_device_with_nan_in_the_workspace(fv, gpu_ctx, streams):
    # Canary: a forward pass over NaN features leaves NaN in every row of the workspace's gi that the next launch covers
    # (384 sequences: what 280 chunks are padded to).  A trimmed launch that read a row it never wrote would carry the NaN
    # into its outputs (at the latest as different bits: the relu of fc2 turns NaN into 0).
    lanes = np.stack(streams["uniform"])
    n_l, n = lanes.shape
    n_chunks, n_frames = n // CHUNK, n // 1024
    d_pcm, d_den = gpu_ctx.device_alloc(lanes.nbytes), gpu_ctx.device_alloc(lanes.nbytes)
    d_band, d_rms = gpu_ctx.device_alloc(n_l * n_frames * 4), gpu_ctx.device_alloc(n_l * n_chunks * 4)
    try:
        gpu_ctx.to_device(d_pcm, lanes)
        got = {}
        with gpu_ctx.options(reproducible="1"):
            for trim in ("none", "all"):
                with gpu_ctx.options(nn_trim=trim):
                    g = gpu_ctx.nsnet2_forward(np.full((384, 54, 161), np.nan, np.float32))
                    # (fc2's relu swallows the NaN: the gains come out as sigmoid(bias), the same in every row)
                    assert np.array_equal(g, np.broadcast_to(g[0, 0], g.shape)) and TRIMMED not in gpu_ctx.last_nn_path()
                    gpu_ctx.enqueue_device(d_pcm, n_l, n, n, d_den, d_band, d_rms)
                    assert (TRIMMED in gpu_ctx.last_nn_path()) == (trim == "all"), gpu_ctx.last_nn_path()
                    got[trim] = [{"denoised": gpu_ctx.to_host(np.empty((n_l, n), np.float32), d_den),
                                  "band_sum": gpu_ctx.to_host(np.empty((n_l, n_frames), np.float32), d_band),
                                  "chunk_rms": gpu_ctx.to_host(np.empty((n_l, n_chunks), np.float32), d_rms)}]
        _same_bits(got["all"], got["none"], "device lanes after NaN")
        ref = _off(gpu_ctx, "uniform", streams["uniform"]) # the host-buffer form of the same call
        for l in range(n_l):
            assert np.array_equal(got["all"][0]["denoised"][l], ref[l]["denoised"]), l
    finally:
        for d in (d_pcm, d_den, d_band, d_rms):
            gpu_ctx.device_free(d)


@pytest.mark.parametrize("T", [54, 7])
def test_forward_keeps_all_rows(gpu_ctx, weights7, T):
    # fvad_nsnet2_forward has no chunk descriptors: the untrimmed projection, the same gains whatever nn_trim says
    rng = np.random.default_rng(T)
    feat = rng.uniform(-11, 2, (3, T, 161)).astype(np.float32)
    gains = {}
    with gpu_ctx.options(reproducible="1"):
        for trim in ("none", "tiles", "all"):
            with gpu_ctx.options(nn_trim=trim):
                gains[trim] = gpu_ctx.nsnet2_forward(feat)
                path = gpu_ctx.last_nn_path()
                assert "panel_gemm3" in path and TRIMMED not in path, path
    for trim in ("tiles", "all"):
        assert np.array_equal(gains[trim].view(np.uint32), gains["none"].view(np.uint32)), trim
    ref = np.stack([orc.nsnet2_forward(weights7, s) for s in feat])
    err = (np.abs(gains["all"].astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-2)).max() # (the floor of the existing gains checks)
    print(f"T = {T}: gains {err:.3e} relative")
    assert err <= 1e-4, err
