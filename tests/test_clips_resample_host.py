"""The host side of the resampled Recorder (no GPU): fvad_clips_plan_resampled and fvad_clips_resample_tile against brute force in
python integers, every rule of fvad_clips_resample_check in its order, the default designs against the numpy design of
ingest_resample_cases.py, the model against the definition term by term, the proof that the tables bite -- five wrong versions
of the model, and which rows tell each -- and what run_clips refuses with "resample"."""
import ctypes as C

import numpy as np
import pytest

import clip_cases as cc
import clip_resample_cases as rc
import ingest_resample_cases as rr

INVALID = -100
U64 = (1 << 64) - 1
# the tables the wrong models are held against: a short filter below 1, a ratio above 1, and the long ratio
BITE = ((2, 3, 4, "sinc"), (7, 5, 2, "sinc"), (147, 640, 1, "sinc"))


def raw_plan(fv, lens, up, down, fmt=0, null=()):
    lens = np.ascontiguousarray(np.asarray(lens, np.uint64))
    n = len(lens)
    out_lens, offsets, total = np.full(n + 1, 77, np.uint64), np.full(n + 1, 77, np.uint64), C.c_uint64(77)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    st = fv.lib().fvad_clips_plan_resampled(None if "lens" in null else p(lens), n, up, down, fmt, None if "out_lens" in null else p(out_lens),
                                            None if "offsets" in null else p(offsets), None if "total" in null else C.byref(total))
    return st, out_lens, offsets, total.value


def test_the_plan_against_python_integers(fv):
    rng = np.random.default_rng(2)
    for up, down in ((147, 160), (2, 3), (147, 320), (147, 640), (1, 3), (2, 1), (7, 5), (640, 1), (1, 1), (1, 4000000000)):
        for pcm16 in (False, True):
            lens = [1, 2, 3, down, down + 1, 29_300_000, 1 << 40] + [int(v) for v in rng.integers(1, 1 << 30, 20)]
            out_lens, offsets, total = fv.clips_plan_resampled(lens, up, down, pcm16)
            want = [-(-n * up // down) for n in lens]
            w_off, w_total = rc.plan(want, pcm16)
            assert [int(v) for v in out_lens] == want and np.array_equal(offsets, w_off) and total == w_total
            assert all(int(o) % (8 if pcm16 else 4) == 0 for o in offsets)
            assert all(fv.resample_out_frames(n, up, down) == w for n, w in zip(lens, want))
    # lengths near 2^64 / up, where up > down: the count saturates at UINT64_MAX (fvad_resample_out_frames) and such a plan is
    # refused; just below, it is planned exactly
    for up, down in ((7, 5), (640, 1), (2, 1)):
        edge = U64 * down // up
        assert fv.resample_out_frames(edge + 1000, up, down) == U64 == min(U64, -(-(edge + 1000) * up // down))
        assert fv.resample_out_frames(U64, up, down) == U64
        st, out_lens, offsets, total = raw_plan(fv, [5, U64], up, down)
        assert st == INVALID and total == 77 and offsets[2] == 77
        n = (U64 - 64) * down // up - down
        st, out_lens, offsets, total = raw_plan(fv, [n], up, down)
        assert st == 0 and int(out_lens[0]) == -(-n * up // down) and total == -(-int(out_lens[0]) // 4) * 4
        assert raw_plan(fv, [n, n], up, down)[0] == INVALID                # the total passes 64 bits
    # below 1 nothing saturates: the longest clip there is is planned exactly, two of them pass 64 bits
    st, out_lens, offsets, total = raw_plan(fv, [U64], 147, 160)
    assert st == 0 and int(out_lens[0]) == -(-U64 * 147 // 160) and raw_plan(fv, [U64, U64], 147, 160)[0] == INVALID
    assert raw_plan(fv, [U64], 1, 1)[0] == INVALID and raw_plan(fv, [U64 - 8], 1, 1)[0] == 0
    # what it refuses, as fvad_clips_plan_strided refuses its own
    for what, kw in (("up 0", dict(lens=[5], up=0, down=3)), ("up above the maximum", dict(lens=[5], up=641, down=3)), ("down 0", dict(lens=[5], up=2, down=0)),
                     ("a clip of length 0", dict(lens=[5, 0, 5], up=2, down=3)), ("a bad format", dict(lens=[5], up=2, down=3, fmt=2)),
                     ("NULL lens", dict(lens=[5], up=2, down=3, null=("lens",))), ("NULL out_lens", dict(lens=[5], up=2, down=3, null=("out_lens",))),
                     ("NULL offsets", dict(lens=[5], up=2, down=3, null=("offsets",))), ("NULL total", dict(lens=[5], up=2, down=3, null=("total",)))):
        st, out_lens, offsets, total = raw_plan(fv, **kw)
        assert st == INVALID and total == 77 and out_lens[-1] == 77 and offsets[-1] == 77, what
    assert raw_plan(fv, [], 2, 3, null=("lens", "out_lens", "offsets"))[::3] == (0, 0)      # no clips: a total of 0


def test_the_tile_against_brute_force(fv):
    rng = np.random.default_rng(4)
    cases = [(147, 160, 5121), (147, 640, 20481), (147, 320, 10241), (2, 3, 97), (1, 3, 97), (1, 6, 193), (2, 1, 65), (1, 1, 1), (640, 1, 20481),
             (1, 1000, 1), (1, 1170, 1), (1, 1171, 1), (1, 1, 8191), (1, 1, 8193), (1, 7, 8137), (1, 48000, 25)]
    cases += [(int(rng.integers(1, 641)), int(rng.integers(1, 3000)), 1 + 2 * int(rng.integers(0, 10241))) for _ in range(300)]
    zero = 0
    for up, down, n_taps in cases:
        got, want = fv.clips_resample_tile(up, down, n_taps), rc.tile_out(up, down, n_taps)
        assert got == want and got % 8 == 0 and got <= rc.TILE_MAX, (up, down, n_taps, got, want)
        if got:
            assert ((got - 1) * down + n_taps - 1) // up + 1 <= rc.WINDOW
            assert got == rc.TILE_MAX or (got + 7) * down + n_taps - 1 >= rc.WINDOW * up
        zero += got == 0
    assert zero >= 3
    assert fv.clips_resample_tile(147, 160, 5121) == 7488 and fv.clips_resample_tile(147, 640, 20481) == 1848
    for up, down, n_taps in ((0, 3, 97), (641, 3, 97), (2, 0, 97), (2, 3, 0), (2, 3, 96), (2, 3, rc.TAPS_MAX + 2)):
        assert fv.clips_resample_tile(up, down, n_taps) == 0


def test_the_check_refuses_in_order(fv):
    good = rc.case_taps(2, 3, 4, "sinc")
    f = fv.lib().fvad_clips_resample_check
    assert fv.clips_resample_check(2, 3, good) == 0 and fv.clips_resample_check(1, 1, np.ones(1, np.float32)) == 0
    assert fv.clips_resample_check(147, 640, np.zeros(rc.TAPS_MAX, np.float32)) == 0 and fv.clips_resample_check(640, 1, good) == 0
    nan = good.copy()
    nan[3] = np.nan
    # the ratio rules, then the tap rules, then the tile: each call breaks the named rule and none before it
    for what, args in (("up 0", (0, 3, fv.fptr(good), 25)), ("up above the maximum", (641, 3, fv.fptr(good), 25)), ("down 0", (2, 0, fv.fptr(good), 25)),
                       ("NULL taps", (2, 3, None, 25)), ("no taps", (2, 3, fv.fptr(good), 0)), ("an even n_taps", (2, 3, fv.fptr(good), 24)),
                       ("a tap that is not finite", (2, 3, fv.fptr(nan), 25)), ("a tile of 0", (1, 48000, fv.fptr(good), 25))):
        assert f(*args) == INVALID, what
    assert fv.clips_resample_check(2, 3, np.zeros(rc.TAPS_MAX + 2, np.float32)) == INVALID, "n_taps above the maximum"
    for bad in (np.inf, -np.inf):
        for at in (0, 12, 24):
            t = good.copy()
            t[at] = bad
            assert fv.clips_resample_check(2, 3, t) == INVALID, (bad, at)
    # the tap rules are fvad_ingest_resample_check's: the same taps, the same answer
    for t in (good, nan, good[:24], np.zeros(rc.TAPS_MAX + 2, np.float32)):
        assert (fv.clips_resample_check(3, 2, t) == 0) == (fv.ingest_resample_check(np.zeros((0, 11), np.uint64), 0, 3, 2, t, 1, 8, 8) == 0)
    assert (fv.RESAMPLE_UP_MAX, fv.RESAMPLE_TAPS_MAX) == (rc.UP_MAX, rc.TAPS_MAX)


@pytest.mark.parametrize("rate,ratio,n_taps", [(44100, (147, 160), 5121), (32000, (2, 3), 97), (22050, (147, 320), 10241), (11025, (147, 640), 20481),
                                               (16000, (1, 3), 97), (96000, (2, 1), 65)])
def test_the_default_designs(fv, rate, ratio, n_taps):
    assert fv.resample_ratio(48000, rate) == ratio
    up, down = ratio
    got, want = fv.resample_design(up, down), rr.design(up, down)
    assert got.dtype == np.float32 and len(got) == len(want) == n_taps
    assert np.all(np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + 1e-12)
    assert abs(float(got.astype(np.float64).sum()) - up) <= 1e-4 * up
    assert fv.clips_resample_check(up, down, got) == 0 and fv.clips_resample_tile(up, down, n_taps) >= 64


# ------------------------------------------------------------------ the model and the tables
@pytest.fixture(scope="module")
def tables():
    out = {}
    for case in BITE:
        t = rc.Table(*case)
        src = t.source(False)
        out[case] = (t, src, rc.model_export(src, t.clips, t.taps, t.up, t.down))
    return out


def test_the_model_is_the_definition_term_by_term():
    rng = np.random.default_rng(9)
    for up, down, half, kind in rc.CASES[:5] + ((147, 640, 1, "sinc"),):
        taps = rc.case_taps(up, down, half, kind)
        R = rc.reach(len(taps), up)
        for n in (1, 2, R, 2 * R + 3, 41):
            x = rng.uniform(-1, 1, n).astype(np.float32)
            full = {"best_channel": [0], "best_rms": [0.0], "runner_up_rms": [0.0]}
            m = rc.resampled_of(full, [x], taps, up, down)
            assert len(m["y"][0]) == rc.out_len(n, up, down) == -(-n * up // down)
            for o in range(len(m["y"][0])):
                assert abs(m["y"][0][o] - rr.brute(x.astype(np.float64), taps.astype(np.float64), up, down, o)) <= 1e-12 * max(1.0, float(m["bound"][0][o])), (up, down, n, o)


def test_the_tables_have_what_they_promise():
    for case in rc.CASES:
        t = rc.Table(*case)
        outs = [int(v) for v in t.out_lens[t.edge]]
        for j, target in enumerate((t.To - 1, t.To, t.To + 1, 2 * t.To + 1, 1)):
            got = set(outs[8 * j:8 * j + 8])
            assert len(got) == 1 and target <= got.pop() <= target + (1 if t.up > t.down else 0), (t, target)
        assert all(sorted(int(a) % 8 for a in t.clips[t.edge[8 * j:8 * j + 8], 2]) == list(range(8)) for j in range(5))
        assert {1, 2, t.R, t.R + 1, 2 * t.R + 1} <= set(int(v) for v in t.clips[t.short, 3] - t.clips[t.short, 2])
        assert len(t.taps) == 2 * t.half * max(t.up, t.down) + 1 and t.taps.tobytes() != t.taps[::-1].tobytes()
        # NaN directly in front of and behind every clip of stream E, in both channels
        src = t.source(False)
        for k in list(t.edge) + list(t.short):
            _, _, a, b = (int(v) for v in t.clips[k])
            assert np.isnan(src[rc.E_LANE:rc.E_LANE + 2, a - 1]).all() and np.isnan(src[rc.E_LANE:rc.E_LANE + 2, b]).all() and np.isfinite(src[rc.E_LANE:, a:b]).all()
        assert (src[rc.E_LANE + 1, int(t.clips[t.edge[0], 2])] != src[rc.E_LANE, int(t.clips[t.edge[0], 2])])
    assert sum(k == "noise" for _, _, _, k in rc.CASES) == 2


@pytest.mark.parametrize("mutation", ["reversed", "floor", "lane", "tile"])
def test_a_wrong_model_fails_the_table_and_these_rows_tell(tables, mutation):
    for case, (t, src, want) in tables.items():
        assert rc.failing(want, want) == []
        wrong = rc.model_export(src, t.clips, t.taps, t.up, t.down, mutation=mutation, To=t.To)
        lens = (t.clips[:, 3] - t.clips[:, 2]).astype(np.int64)
        starts = t.clips[:, 2].astype(np.int64)
        if mutation == "floor":
            # the last output is missing wherever len * up is no multiple of down: the lengths tell
            short = [i for i in range(len(lens)) if len(wrong["samples"][i]) != len(want["y"][i])]
            assert short == [i for i in range(len(lens)) if int(lens[i]) * t.up % t.down and int(lens[i]) * t.up >= t.down] and len(short) >= 30
            continue
        bad = set(rc.failing(wrong, want))
        silent = {i for i in range(len(lens)) if not np.any(want["bound"][i])}                # digital silence tells nothing
        if mutation == "reversed":
            # (a clip of a sample or two may meet only taps that mirror onto taps of equal weight in its few outputs)
            assert bad <= set(range(len(lens))) - silent and {i for i in range(len(lens)) if lens[i] > t.R} - silent <= bad and len(bad) >= 40, case
        elif mutation == "lane":
            # a clip whose start is a whole number of output periods into the lane has the right phase; every other one tells
            aligned = {i for i in range(len(lens)) if int(starts[i]) * t.up % t.down == 0}
            assert bad == set(range(len(lens))) - aligned - silent and len(bad) >= 30, (case, len(bad))
        else:
            # only clips of more than one tile have a tile edge inside them
            multi = {i for i in range(len(lens)) if len(want["y"][i]) > t.To}
            assert bad == multi - silent and len(bad) >= 16, (case, sorted(bad ^ multi))


def test_a_phase_restarted_at_the_seam_fails_the_table(tables):
    for case, (t, src, _) in tables.items():
        lay = rc.split_case(t, src)
        want = rc.model_export_split(lay, t.taps, t.up, t.down)
        assert rc.failing(want, want) == []
        whole = rc.model_export(src, t.clips[lay.base], t.taps, t.up, t.down)   # the split model is the contiguous one, whatever the seam
        assert all(np.array_equal(a, b) for a, b in zip(want["y"], whole["y"]))
        bad = set(rc.failing(rc.model_export_split(lay, t.taps, t.up, t.down, mutation="restart"), want))
        inner = {i for i, r in enumerate(lay.rows.astype(np.int64)) if r[3] > 0 and r[6] > 0}
        assert bad <= inner and len(bad) >= len(inner) - 2 and len(bad) >= 10, (case, sorted(inner - bad))
        # the seams the table has to hold
        n = int(lay.rows[0, 3] + lay.rows[0, 6])
        sig = set(int(s) for s in lay.sigma[lay.base == lay.base[0]])
        R = t.R
        assert {0, n, 1, n - 1, R - 1, R, R + 1, n - R - 1, n - R, n - R + 1} <= sig
        c2 = t.To * t.down // t.up
        assert any(c2 - R <= s < c2 for s in sig) and any(c2 < s < 2 * c2 - R for s in sig) and any(2 * c2 - 1 <= s <= 2 * c2 + R for s in sig)
        assert (lay.rows[:, 3] < R).any() and (lay.rows[:, 6] < R).any()


def test_what_run_clips_refuses_with_resample(pkg, tmp_path):
    out = tmp_path / "never"
    for kw in (dict(original_rate=48000, original_filter="resample"), dict(original_rate=44101, original_filter="resample"),
               dict(original_rate=0, original_filter="resample"), dict(original_rate="44100", original_filter="resample"),
               dict(denoised_rate=48000, denoised_filter="resample"), dict(denoised_rate=44101, denoised_filter="resample"),
               dict(denoised_rate=0, denoised_filter="resample"), dict(denoised_rate="22050", denoised_filter="resample"),
               dict(denoised_filter="resample"), dict(original_rate=44100), dict(original_rate=44100, original_filter="fir")):
        with pytest.raises(ValueError):
            pkg.simulator.run_clips(str(tmp_path / "no-such-plan.json"), str(out), **kw)   # (neither a plan nor a context is ever opened)
    assert not out.exists()
    rates, firs = pkg.simulator._clip_rates(44100, 22050, "resample", "resample")
    assert rates == {"original": 44100, "denoised": 22050}
    assert (firs["original"]["up"], firs["original"]["down"], len(firs["original"]["taps"])) == (147, 160, 5121)
    assert (firs["denoised"]["up"], firs["denoised"]["down"], len(firs["denoised"]["taps"])) == (147, 320, 10241)
    for rate in (32000, 11025, 16000, 24000, 8000):
        assert pkg.simulator._clip_rates(rate, 48000, "resample", "none")[1]["original"]["taps"].size % 2 == 1
