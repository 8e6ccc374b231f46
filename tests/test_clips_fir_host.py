"""The host side of the filtered Recorder (no GPU): fvad_clips_fir_design against the numpy design of clip_fir_cases.py and the
frequency responses it has to reach, every refusal of the design and of fvad_clips_fir_check, and the proof that the table
bites -- five wrong versions of the model each fail it."""
import ctypes as C

import numpy as np
import pytest

import clip_cases as cc
import clip_fir_cases as fc

INVALID = -100
TABLE = fc.Table()
SRC = TABLE.source(False)


def raw_design(fv, step, half, cutoff, beta, taps="own"):
    t = np.full(fc.TAPS_MAX + 1, 77.0, np.float32)
    return fv.lib().fvad_clips_fir_design(step, half, cutoff, beta, fv.fptr(t) if taps == "own" else None), t


@pytest.mark.parametrize("args", [(1, 0, 0.0, 0.0), (2, 0, 0.0, 0.0), (3, 0, 0.0, 0.0), (6, 0, 0.0, 0.0), (16, 0, 0.0, 0.0), (3, 48, 0.15, 8.0),
                                  (3, 1, 0.5, 0.0), (2, 256, 0.01, 12.5), (16, 7, 0.03, 0.5), (5, 100, 0.1, 0.0), (1, 256, 0.5, 30.0)])
def test_the_design_is_numpys(fv, args):
    step, half, cutoff, beta = args
    got = fv.clips_fir_design(step, half, cutoff, beta)
    want = fc.design(step, half, cutoff, beta)
    assert got.dtype == np.float32 and len(got) == len(want) == 2 * (half or 16 * step) + 1
    assert np.all(np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + 1e-12), float(np.max(np.abs(got - want)))
    assert got.tobytes() == got[::-1].tobytes()                            # symmetric
    assert abs(float(np.sum(got.astype(np.float64))) - 1.0) <= 1e-6
    status, t = raw_design(fv, *args)
    assert status == 0 and np.all(t[len(got):] == 77.0)                    # nothing behind the taps is written
    assert fv.clips_fir_check(got) == 0


@pytest.mark.parametrize("step", [2, 3, 6])
def test_the_default_design_passes_the_band_and_stops_the_images(fv, step):
    taps = fv.clips_fir_design(step)
    assert len(taps) == 32 * step + 1
    f = np.linspace(0.0, 0.5, 20001)                                       # cycles per input sample
    db = 20 * np.log10(np.maximum(fc.response(taps, f), 1e-300))
    nyq = 0.5 / step                                                       # the output rate's Nyquist frequency
    passband, stopband = db[f <= 0.8 * nyq], db[f >= 1.2 * nyq]
    assert passband.max() <= 0.12 and passband.min() >= -0.12, (passband.min(), passband.max())
    assert stopband.max() <= -68.0, stopband.max()


def test_the_design_refuses(fv):
    for what, args in (("step 0", (0, 0, 0.0, 0.0)), ("step above the limit", (17, 0, 0.0, 0.0)), ("half above 256", (3, 257, 0.0, 0.0)),
                       ("a negative cutoff", (3, 0, -0.1, 0.0)), ("a cutoff above 0.5", (3, 0, 0.5000001, 0.0)),
                       ("a NaN cutoff", (3, 0, float("nan"), 0.0)), ("an infinite cutoff", (3, 0, float("inf"), 0.0)),
                       ("a negative beta", (3, 0, 0.0, -1.0)), ("a NaN beta", (3, 0, 0.0, float("nan"))),
                       ("an infinite beta", (3, 0, 0.0, float("inf")))):
        status, t = raw_design(fv, *args)
        assert status == INVALID and np.all(t == 77.0), what
    assert raw_design(fv, 3, 0, 0.0, 0.0, taps=None)[0] == INVALID, "NULL taps"
    # a beta whose I0 overflows float64 has no normalised form: refused as well, nothing written
    status, t = raw_design(fv, 3, 0, 0.0, 1.0e4)
    assert status == INVALID and np.all(t == 77.0)
    assert raw_design(fv, 16, 256, 0.5, 0.0)[0] == 0 and raw_design(fv, 1, 1, 1e-6, 700.0)[0] == 0


def test_the_check_refuses(fv):
    good = fv.clips_fir_design(3)
    assert fv.clips_fir_check(good) == 0 and fv.clips_fir_check(np.ones(1, np.float32)) == 0
    assert fv.clips_fir_check(np.zeros(fc.TAPS_MAX, np.float32)) == 0
    f = fv.lib().fvad_clips_fir_check
    assert f(None, 97) == INVALID, "NULL taps"
    assert f(fv.fptr(good), 0) == INVALID, "no taps"
    assert f(fv.fptr(good), 96) == INVALID, "an even n_taps"
    assert fv.clips_fir_check(np.zeros(fc.TAPS_MAX + 2, np.float32)) == INVALID, "n_taps above the maximum"
    assert fv.clips_fir_check(np.zeros(fc.TAPS_MAX + 1, np.float32)) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 48, 96):
            t = good.copy()
            t[at] = bad
            assert fv.clips_fir_check(t) == INVALID, (bad, at)
    assert fv.CLIP_FIR_TAPS_MAX == fc.TAPS_MAX


# ------------------------------------------------------------------ the table bites
def fails(got, want):
    try:
        fc.compare(got, want)
    except AssertionError:
        return True
    return False


def cases_of(step):
    return [c for c in TABLE.cases if c.step == step]


@pytest.fixture(scope="module")
def right():
    """the model over the cases the wrong models are held against, once"""
    return {repr(c): fc.model_export_fir(SRC, TABLE.clips[c.idx], TABLE.skips(c), c.step, c.taps) for c in cases_of(3) + cases_of(6)}


def test_the_model_agrees_with_itself_and_with_a_full_rate_filter(right):
    case = cases_of(3)[1]
    want = right[repr(case)]
    assert not fails(want, want)
    # the centres are those of the full-rate clip filtered as a finite signal: np.convolve of the picked channel, [skip::step]
    for i, k in zip(range(len(case.idx)), TABLE.skips(case)):
        l0, _, a, b = (int(v) for v in TABLE.clips[case.idx[i]])
        x = cc.as_f32(SRC[l0 + want["best_channel"][i], a:b]).astype(np.float64)
        full = np.convolve(x, case.taps.astype(np.float64)[::-1])[case.H:case.H + len(x)]
        assert np.allclose(want["y"][i], full[int(k)::3], rtol=0, atol=1e-12), i
    assert all(np.array_equal(want[f], cc.model_export(SRC, TABLE.clips[case.idx], False)[f]) for f in ("best_channel", "best_rms", "runner_up_rms"))


@pytest.mark.parametrize("mutation", ["reversed", "skip0", "replicate", "filtered"])
def test_a_wrong_model_fails_the_table(right, mutation):
    caught = [c for c in cases_of(3) + cases_of(6)
              if fails(fc.model_export_fir(SRC, TABLE.clips[c.idx], TABLE.skips(c), c.step, c.taps, mutation=mutation), right[repr(c)])]
    # skip0 is the right model where every skip is 0: it must fail every case that has another skip, and all the others fail all
    must = [c for c in cases_of(3) + cases_of(6) if mutation != "skip0" or TABLE.skips(c).any()]
    assert [repr(c) for c in caught] == [repr(c) for c in must]


def test_a_filter_restarted_at_the_seam_fails_the_table():
    for case in (cases_of(3)[2], cases_of(2)[1]):
        lay, skips = fc.split_case(TABLE, case, SRC)
        want = fc.model_export_split_fir(lay, skips, case.step, case.taps)
        assert not fails(want, want)
        assert fails(fc.model_export_split_fir(lay, skips, case.step, case.taps, mutation="restart"), want)
        # the split model is the contiguous one of the same clips, whatever the seam
        whole = fc.model_export_fir(SRC, TABLE.clips[lay.base], skips, case.step, case.taps)
        assert all(np.array_equal(a, b) for a, b in zip(want["y"], whole["y"]))
        # the seams the table has to hold: 1, H - 1, H, H + 1 from either end, around kept samples, a_len < H and b_len < H
        n, k = int(lay.rows[0, 3] + lay.rows[0, 6]), int(skips[0])
        sig = set(int(s) for s in lay.sigma[lay.base == lay.base[0]])
        H = case.H
        assert {0, n, 1, n - 1, H - 1, H, H + 1, n - H - 1, n - H, n - H + 1, k, k + 1} <= sig
        To = fc.tile_out(case.step, H)
        c2 = k + To * case.step
        assert any(c2 - H < s < c2 for s in sig) and any(c2 < s < c2 + (To - 1) * case.step for s in sig) and any(n - H < s < n for s in sig)


def test_the_table_has_what_it_promises():
    assert [(c.step, c.H) for c in TABLE.cases] == [(s, h) for s, h in fc.CASES for _ in range(s)]
    for case in TABLE.cases:
        To = fc.tile_out(case.step, case.H)
        lens = (TABLE.clips[case.edge, 3] - TABLE.clips[case.edge, 2]).astype(np.int64)
        outs = [-(-(int(n) - int(k)) // case.step) for n, k in zip(lens, TABLE.skips(case, case.edge))]
        assert outs == [t for t in (To - 1, To, To + 1, 2 * To + 1, 1) for _ in range(8)], case
        assert sorted(set(int(a) % 8 for a in TABLE.clips[case.edge[:8], 2])) == list(range(8))
        assert (To - 1) * case.step + 1 + 2 * case.H <= fc.TILE and To % 8 == 0
        assert len(case.taps) == 2 * case.H + 1 and case.taps.tobytes() != case.taps[::-1].tobytes()
    assert sum(len(c.refused) for c in TABLE.cases) > 10
