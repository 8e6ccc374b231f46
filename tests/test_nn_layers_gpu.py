"""Every NSNet2 layer of every f32 kernel family against float64, one kernel at a time (nn_layer_cases.py: references from the
GPU's own previous-layer outputs, units of rounding error, tolerances of 4 x the oracle's own distance).

The layers come out of the workspace through fvad_ctx_nn_tap.  Before every judged pass a pass over NaN features of the same
shape runs under the same options: h1 / h2 of every row are then NaN and f2 / f3 / gains what the biases alone give, so a row
the judged pass did not write shows -- never as the previous case's correct values.

fvad_nsnet2_forward (skip = 0, no lane descriptors) reaches every family through the context options; the engine's own paths
(skip = 4: fc2's row map, the tail layers over the real rows only, the trimmed first input projection) are judged from the
engine's feature tap.  Worst distances are printed per (family, layer): pytest -s."""
import ctypes as C

import numpy as np
import pytest

import nn_layer_cases as N

pytestmark = pytest.mark.gpu

CHUNK = 24000
TRIMMED = "gi1 rows 4..53"

# id -> (options, real sequence counts at T = 54, what last_nn_path must contain: a forced kernel at every T, the default selection
# at T = 54)
# Large-batch forms: 3 and 200 real sequences (forcing pads them to 384, `reproducible` to 128 / 256): real rows end inside a
# 16-row tile and inside a 64 / 128 / 192-sequence workgroup.  Small-batch forms: 1, 82, 97, 130.
# gru_rec3 needs the persistent GEMM in front of it (below 2048 sequences a forced gru_kernel alone keeps the small-batch GEMMs
# and is demoted to gru_lat), hence gemm_kernel = v3 beside it.  The persistent GEMM takes whole 256-row panels: at T = 1, 7, 55 the
# 384 sequences a small count is padded to do not fill them and the small-batch GEMMs would run instead, so the short and odd
# lengths run 385 sequences there (SHORT_COUNT) -- padded to 768 (512 without a forced recurrence), whose rows are whole panels
# at every T and which 64, 128 and 192 all divide.  gru_lat_tiles takes effect whenever the padded batch is a multiple of
# 16 x tiles (384 is, of both); the path names the tiles that ran.
FAMILIES = {
    "default-1": ({}, [1], ["panel_gemm (fc1 folded)", "gru_ws2k (layers pipelined)"]),
    "default-82": ({}, [82], ["gru_ws2k (layers pipelined, both input projections in the kernel)"]),
    "default-130": ({}, [130], ["gru_ws2m"]),
    "v5w0": ({"gru_kernel": "v5w0"}, [1, 82, 97, 130], ["panel_gemm (fc1 folded)", "gru_ws"]),
    "v4w8": ({"gru_kernel": "v4w8"}, [1, 82, 97, 130], ["panel_gemm (fc1 folded)", "gru_lat"]),
    "v4w8-tiles2": ({"gru_kernel": "v4w8", "gru_lat_tiles": "2"}, [3, 200], ["gru_lat (2 row tiles)"]),
    "v4w8-tiles3": ({"gru_kernel": "v4w8", "gru_lat_tiles": "3"}, [3, 200], ["gru_lat (3 row tiles)"]),
    "v3w4": ({"gemm_kernel": "v3", "gru_kernel": "v3w4"}, [3, 200], ["panel_gemm3 (fc1 folded)", "gru_rec3<4>"]),
    "v3w8": ({"gemm_kernel": "v3", "gru_kernel": "v3w8"}, [3, 200], ["panel_gemm3 (fc1 folded)", "gru_rec3<8>"]),
    "v3w12": ({"gemm_kernel": "v3", "gru_kernel": "v3w12"}, [3, 200], ["panel_gemm3 (fc1 folded)", "gru_rec3<12>"]),
    "gemm-v1": ({"gemm_kernel": "v1"}, [1, 82, 97, 130], ["panel_gemm (fc1 folded)"]),
    "v3nofold": ({"gemm_kernel": "v3nofold"}, [3, 200], ["f32: panel_gemm3 + gru_"]),
    "reproducible": ({"reproducible": "1"}, [3, 200], ["panel_gemm3 (fc1 folded)", "gru_rec3"]),
}
DEFAULT_SELECTION = ("default-1", "default-82", "default-130")   # the kernels depend on (count, T): the path is pinned at T = 54
SHORT_T = (1, 2, 7, 55)
SHORT_COUNT = {"v3w4": 385, "v3w8": 385, "v3w12": 385, "v3nofold": 385}   # the others: max(first count, 5)

_ctxs = {}
_worst = {}


def _ctx(fv, gpu_ctx, weights7, name):
    """the session's context for the seed-7 weights, one more per other model (closed by teardown_module)"""
    if name == "synth":
        return gpu_ctx
    if name not in _ctxs:
        _ctxs[name] = fv.Context(0)
        _ctxs[name].load_weights(N.model(name, weights7).w)
    return _ctxs[name]


def teardown_module(module):
    for c in _ctxs.values():
        c.close()
    _ctxs.clear()
    for (fam, k), v in sorted(_worst.items()):
        print(f"worst over the module: {fam:14s} {k:5s} {v:6.2f} units (tolerance {N.TOL[k]:.2f})")


def _taps(ctx, first, n):
    return {k: ctx.nn_tap(k, first, n) for k in N.LAYERS}


def _assert_within(fam, what, res):
    line = "  ".join(f"{k} {v[0]:.2f}" for k, v in res.items())
    print(f"{fam:14s} {what}: {line}")
    for k, (d, where) in res.items():
        _worst[(fam, k)] = max(_worst.get((fam, k), 0.0), d)
    for k, (d, where) in res.items():
        assert d <= N.TOL[k], (fam, what, k, d, N.TOL[k], "at (sequence, row, unit)", where)


def _forward_case(ctx, m, fam, n, T, seed):
    opts, _, expect = FAMILIES[fam]
    feat = N.make_inputs(n, T, seed)
    with ctx.options(**opts):
        ctx.nsnet2_forward(np.full(feat.shape, np.nan, np.float32))
        g = ctx.nsnet2_forward(feat)
        path = ctx.last_nn_path()
        got = _taps(ctx, 0, n)
    assert path.startswith("f32:"), path
    if T == 54 or fam not in DEFAULT_SELECTION:
        assert all(e in path for e in expect), (fam, n, T, path)
    if fam == "v4w8":
        assert "row tiles" not in path, path                 # one row tile per workgroup unless the option (or 8192 sequences) asks
    # the pipelined recurrence keeps h1 to itself; every other family leaves all five layers
    assert (got["h1"] is None) == ("gru_ws2" in path), path
    assert all(got[k] is not None for k in N.LAYERS[1:]), path
    assert got["h2"].shape == (n, T, 400) and got["f2"].shape == (n, T, 600) and got["gains"].shape == (n, T, 161)
    assert np.array_equal(got["gains"].view(np.uint32), g.view(np.uint32)), "the gains tap is what fvad_nsnet2_forward returned"
    _assert_within(fam, f"{m.name} n = {n} T = {T} [{path.split('+')[-1].strip()}]", N.judge(m, feat, got))


@pytest.mark.parametrize("model", N.MODELS)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_forward_layers_at_the_engines_length(fv, gpu_ctx, weights7, fam, model):
    ctx, m = _ctx(fv, gpu_ctx, weights7, model), N.model(model, weights7)
    counts = FAMILIES[fam][1]
    for n in (counts if model == "synth" else counts[-1:] if counts[-1] < 200 else counts[:1]):
        _forward_case(ctx, m, fam, n, 54, 300 + n)


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_forward_layers_at_short_and_odd_lengths(fv, gpu_ctx, weights7, fam):
    # T = 1: no recurrence, the projection and the gates alone; 2: one recurrent step; 7, 55: rows that fill no panel
    m = N.model("synth", weights7)
    n = SHORT_COUNT.get(fam, max(FAMILIES[fam][1][0], 5))    # (5: every kind of sequence of make_inputs; still one 32-sequence padding)
    for T in SHORT_T:
        _forward_case(gpu_ctx, m, fam, n, T, 400 + T)


def test_tap_argument_rules(fv, gpu_ctx, weights7):
    L = fv.lib()
    rows, width = C.c_size_t(0), C.c_size_t(0)
    buf = np.zeros(54 * 600 * 4, np.float32)
    tap = lambda ctx, layer, first, n, out=buf, r=rows, w=width: L.fvad_ctx_nn_tap(  # noqa: E731
        ctx.h, layer, first, n, fv.fptr(out), C.byref(r) if r is not None else None, C.byref(w) if w is not None else None)
    fresh = fv.Context(0)
    try:
        fresh.load_weights(weights7)
        assert tap(fresh, 0, 0, 1) == fv.FVAD_ERR_NOT_AVAILABLE and fresh.nn_tap("gains", 0, 1) is None     # no pass yet
        f = N.make_inputs(3, 54, 1)
        fresh.nsnet2_forward(f)
        assert tap(fresh, 4, 0, 3) == 0 and (rows.value, width.value) == (54, 161)
        assert tap(fresh, 4, 0, 3, out=None) == fv.FVAD_ERR_INVALID_ARGUMENT
        assert tap(fresh, 4, 0, 3, r=None) == fv.FVAD_ERR_INVALID_ARGUMENT and tap(fresh, 4, 0, 3, w=None) == fv.FVAD_ERR_INVALID_ARGUMENT
        assert tap(fresh, 5, 0, 1) == fv.FVAD_ERR_INVALID_ARGUMENT and tap(fresh, -1, 0, 1) == fv.FVAD_ERR_INVALID_ARGUMENT
        assert tap(fresh, 4, 0, 0) == fv.FVAD_ERR_INVALID_ARGUMENT
        # the batch is padded to 32 sequences; only the 3 real ones are tapped
        assert tap(fresh, 4, 3, 1) == fv.FVAD_ERR_INVALID_ARGUMENT and tap(fresh, 4, 2, 2) == fv.FVAD_ERR_INVALID_ARGUMENT
        assert tap(fresh, 4, 2, 1) == 0 and tap(fresh, 1, 1, 2) == 0 and (rows.value, width.value) == (54, 400)
        with pytest.raises(fv.FvadError):
            fresh.nn_tap("gains", 0, 4)
        # a model loaded (or a buffer reallocated) since the pass: not available, never stale memory
        fresh.load_weights(weights7)
        assert tap(fresh, 4, 0, 1) == fv.FVAD_ERR_NOT_AVAILABLE
        # the emulations keep split fragments: nothing to tap
        for math in ("f16x3", "bf16x3"):
            with fresh.options(nn_math=math):
                fresh.nsnet2_forward(f)
                assert fresh.last_nn_path().startswith(math + ":")
                assert all(fresh.nn_tap(k, 0, 1) is None for k in N.LAYERS)
        fresh.nsnet2_forward(f)
        assert fresh.nn_tap("f3", 0, 3).shape == (3, 54, 600)
    finally:
        fresh.close()


# ------------------------------------------------------------------ the engine's paths

def _stream(pkg, n_chunks, seed):
    pcm, _ = pkg.synth.make_stream(n_chunks * 0.5 + 0.1, seed=seed)
    return pcm[0][: n_chunks * CHUNK].copy()


_streams = {}


def _lanes(pkg, name):
    """test_nn_trim_gpu.py's lanes: 1, 2, 5 and 70 chunks; four of 70 (70 > 64: a chunk's predecessor sits in another workgroup
    of gru_rec3<4>); one of 82 (BASELINE config 3's shape)"""
    if not _streams:
        ragged = [_stream(pkg, n, 500 + n) for n in (1, 2, 5, 70)]
        _streams.update(ragged=ragged, uniform=[ragged[3]] + [_stream(pkg, 70, 600 + i) for i in range(3)], cfg3=[_stream(pkg, 82, 700)])
    return _streams[name]


_judged = {}


def _engine_case(fv, ctx, m, lanes, what, **opts):
    n = sum(x.shape[0] // CHUNK for x in lanes)
    with ctx.options(**opts):
        ctx.nsnet2_forward(np.full((n, 54, 161), np.nan, np.float32))
        out = ctx.engine_run([x.copy() for x in lanes], want_taps=True, want_denoised=True)
        path = ctx.last_nn_path()
        got = _taps(ctx, 0, n)
        with pytest.raises(fv.FvadError, match="InvalidArgument"):
            ctx.nn_tap("gains", n, 1)                         # the first sequence past the pass's real ones
    feat = np.concatenate([o["features"] for o in out])      # sequences in launch order: lane-contiguous
    assert feat.shape == (n, 54, 161)
    key = (what, tuple(None if v is None else hash(v.tobytes()) for v in got.values()), hash(feat.tobytes()))
    if key not in _judged:                                    # (the same bits under another option: the same judgment)
        _judged[key] = N.judge(m, feat, got, N.SKIP)
    return feat, got, path, out, _judged[key]


def test_engine_uniform_lanes_trimmed_and_untrimmed(fv, pkg, gpu_ctx, weights7):
    m, lanes = N.model("synth", weights7), _lanes(pkg, "uniform")
    taps = {}
    for trim in ("all", "none"):
        feat, got, path, out, res = _engine_case(fv, gpu_ctx, m, lanes, "4 x 70", reproducible="1", nn_trim=trim)
        assert "panel_gemm3" in path and "gru_rec3" in path and path.endswith(TRIMMED) == (trim == "all"), path
        assert got["h1"].shape == (280, 54, 400) and got["f2"].shape == (280, 50, 600) and got["gains"].shape == (280, 50, 161)
        _assert_within("engine " + trim, "4 x 70 chunks", res)
        # the rows the trimmed projection does not compute: h1 rows 0..3 of every chunk that is not the first of its lane
        later = np.setdiff1d(np.arange(280), np.arange(0, 280, 70))
        ref, unit = N.ref_gru(m, "h1", feat[later, :4], got["h1"][later, :4])
        d, where = N.distance(got["h1"][later, :4], ref, unit)
        print(f"engine {trim}: h1 rows 0..3 of the 276 later chunks {d:.2f} units")
        assert d <= N.TOL["h1"], (trim, d, where)
        # K3's input is what was tapped: under `reproducible` fvad_nsnet2_forward gives the feature tap those very bits
        with gpu_ctx.options(reproducible="1"):
            g = gpu_ctx.nsnet2_forward(feat)
        assert np.array_equal(g[:, N.SKIP:].view(np.uint32), got["gains"].view(np.uint32)), trim
        taps[trim] = got
    for k in N.LAYERS:
        assert np.array_equal(taps["all"][k].view(np.uint32), taps["none"][k].view(np.uint32)), k


def test_engine_ragged_lanes_compute_all_rows(fv, pkg, gpu_ctx, weights7):
    m, lanes = N.model("synth", weights7), _lanes(pkg, "ragged")
    feat, got, path, out, res = _engine_case(fv, gpu_ctx, m, lanes, "ragged", reproducible="1", nn_trim="all")
    assert "panel_gemm3" in path and "gru_rec3" in path and TRIMMED not in path, path
    assert got["h1"].shape == (78, 54, 400) and got["f3"].shape == (78, 50, 600)
    _assert_within("engine ragged", "1 + 2 + 5 + 70 chunks", res)
    with gpu_ctx.options(reproducible="1"):
        g = gpu_ctx.nsnet2_forward(feat)
    assert np.array_equal(g[:, N.SKIP:].view(np.uint32), got["gains"].view(np.uint32))


def test_engine_82_chunks_in_the_default_mode(fv, pkg, gpu_ctx, weights7):
    # config 3's shape: the pipelined recurrence, then fc2 .. fc4 over the 82 real sequences' rows only (96 padded)
    m, lanes = N.model("synth", weights7), _lanes(pkg, "cfg3")
    feat, got, path, out, res = _engine_case(fv, gpu_ctx, m, lanes, "82")
    assert "gru_ws2k" in path, path
    assert got["h1"] is None and got["h2"].shape == (82, 54, 400) and got["f2"].shape == (82, 50, 600)
    assert "h12" in res and "h1" not in res
    _assert_within("engine 82", "1 x 82 chunks", res)
    with pytest.raises(fv.FvadError, match="InvalidArgument"):
        gpu_ctx.nn_tap("h2", 80, 3)                           # 82 real of 96: the padding is not tapped
    assert gpu_ctx.nn_tap("h2", 81, 1).shape == (1, 54, 400)
