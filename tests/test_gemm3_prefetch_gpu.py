"""panel_gemm3 requests its activation operands two super-steps ahead, straight through item boundaries.

What could go wrong is a boundary: the operands of an item's first two super-steps are requested by the previous item's last
two (rows of another panel), and a workgroup's last item re-requests rows of its own.  A lane's results must therefore not depend
on where its rows fall in the launch:

  * one lane of 96 chunks, padded to 128 sequences: 27 / 25 row panels x 5 / 3 / 1 column blocks = at most 135 items, one per
    workgroup (every item is a workgroup's first and last);
  * the same lane as the first, and as the last, of four (384 sequences: 405 / 225 / 75 items over 256 workgroups -- workgroups
    with two items and with one; as the last lane its rows sit in other panels, at other offsets into them).

The lane's five layer taps (fvad_ctx_nn_tap), denoised audio, band sums and chunk RMS are compared as uint32 between the three
launches, and with the oracle pipeline on the same samples (denoised 1e-4 of peak, band sums and RMS 1e-4 relative: the bounds of
test_nn_trim_gpu.py).  All under option reproducible: the persistent GEMM + gru_rec3 at every launch size.  A pass over NaN
features in front of every run leaves no earlier run's values in the workspace.
"""
import numpy as np
import pytest

import nn_layer_cases as N
import orc

pytestmark = pytest.mark.gpu

CHUNK = 24000
N_CHUNKS = 96


def _stream(pkg, seed):
    pcm, _ = pkg.synth.make_stream(N_CHUNKS * 0.5 + 0.1, seed=seed)
    return pcm[0][: N_CHUNKS * CHUNK].copy()


@pytest.fixture(scope="module")
def lanes(pkg):
    return [_stream(pkg, 800 + i) for i in range(4)]


def _run(ctx, lanes, at):
    """engine outputs and layer taps of lane `at` of the launch"""
    n = len(lanes) * N_CHUNKS
    n_pad = (n + 127) // 128 * 128
    with ctx.options(reproducible="1"):
        ctx.nsnet2_forward(np.full((n_pad, 54, 161), np.nan, np.float32))
        out = ctx.engine_run([x.copy() for x in lanes], want_denoised=True)
        path = ctx.last_nn_path()
        taps = {k: ctx.nn_tap(k, at * N_CHUNKS, N_CHUNKS) for k in N.LAYERS}
    assert "panel_gemm3 (fc1 folded)" in path and "gru_rec3" in path, path
    return out[at], taps


def _same_bits(a, b, what):
    (out_a, taps_a), (out_b, taps_b) = a, b
    for k in N.LAYERS:
        x, y = taps_a[k], taps_b[k]
        assert x is not None and y is not None and x.shape == y.shape and np.all(np.isfinite(x)), (what, k)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, k, int((x.view(np.uint32) != y.view(np.uint32)).sum()))
    for k in ("denoised", "band_sum", "chunk_rms"):
        x, y = np.ascontiguousarray(out_a[k]), np.ascontiguousarray(out_b[k])
        assert x.shape == y.shape and np.all(np.isfinite(x)), (what, k)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, k, int((x.view(np.uint32) != y.view(np.uint32)).sum()))


@pytest.fixture(scope="module")
def alone(gpu_ctx, lanes):
    return _run(gpu_ctx, lanes[:1], 0)


def test_one_item_per_workgroup_matches_oracle(gpu_ctx, weights7, lanes, alone):
    out, _ = alone
    p = orc.Pipeline(weights7, n_channels=1, keep_denoised=True)
    p.push(lanes[0][None])
    den, band, rms = p.denoised()[0], p.band_volumes()[:, 0], p.chunk_rms()[:, 0]
    assert out["denoised"].shape == den.shape
    err = np.abs(out["denoised"].astype(np.float64) - den).max() / np.abs(den).max()
    eb = (np.abs(out["band_sum"].astype(np.float64) - band) / np.abs(band)).max()
    er = (np.abs(out["chunk_rms"].astype(np.float64) - rms) / np.abs(rms)).max()
    print(f"96 chunks alone: denoised {err:.3e} of peak, band sums {eb:.3e}, rms {er:.3e}")
    assert err <= 1e-4 and eb <= 1e-4 and er <= 1e-4, (err, eb, er)


def test_first_of_four_lanes_same_bits(gpu_ctx, lanes, alone):
    _same_bits(_run(gpu_ctx, lanes, 0), alone, "first of four")


def test_last_of_four_lanes_same_bits(gpu_ctx, lanes, alone):
    _same_bits(_run(gpu_ctx, lanes[1:] + lanes[:1], 3), alone, "last of four")
