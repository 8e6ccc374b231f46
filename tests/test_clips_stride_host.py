"""The host side of the strided Recorder (no GPU): fvad_clips_phase_skips and fvad_clips_plan_strided against the model of
clip_stride_cases.py, every error of the planner, and the proof that the table bites -- four wrong versions of the model each
fail it, and which clips catch which is stated here."""
import ctypes as C

import numpy as np
import pytest

import clip_cases as cc
import clip_stride_cases as st

INVALID = -100
TABLE = st.Table()


def lens_of(idx):
    return (TABLE.clips[idx, 3] - TABLE.clips[idx, 2]).astype(np.int64)


def test_phase_skips_keep_the_lane_indices_of_the_phase(fv):
    starts = np.concatenate([TABLE.clips[:, 2], np.array([0, 1, 2, 3, 2 ** 40 + 1, 2 ** 64 - 1], np.uint64)])
    for step in range(1, st.STEP_MAX + 1):
        for phase in range(step):
            skips = fv.clips_phase_skips(starts, step, phase)
            assert skips.dtype == np.uint32 and np.all(skips < step)
            assert all((int(a) + int(k)) % step == phase for a, k in zip(starts, skips))
            assert [int(k) for k in skips] == [st.phase_skip(a, step, phase) for a in starts]
    assert len(fv.clips_phase_skips([], 3, 2)) == 0


def raw_skips(fv, n, step, phase, starts="own", skips="own"):
    a, k = np.arange(max(n, 1), dtype=np.uint64), np.full(max(n, 1), 77, np.uint32)
    status = fv.lib().fvad_clips_phase_skips(a.ctypes.data_as(C.POINTER(C.c_uint64)) if starts == "own" else None, n, step, phase,
                                             k.ctypes.data_as(C.POINTER(C.c_uint32)) if skips == "own" else None)
    return status, k


def test_phase_skips_errors(fv):
    for what, kw in (("step 0", dict(step=0, phase=0)), ("step above the limit", dict(step=st.STEP_MAX + 1, phase=0)),
                     ("phase not below the step", dict(step=3, phase=3)), ("NULL starts", dict(step=3, phase=0, starts=None)),
                     ("NULL skips", dict(step=3, phase=0, skips=None))):
        status, k = raw_skips(fv, 4, **kw)
        assert status == INVALID and np.all(k == 77), what
    assert raw_skips(fv, 0, 3, 0, starts=None, skips=None)[0] == 0          # no clips: nothing to do
    assert raw_skips(fv, 4, st.STEP_MAX, st.STEP_MAX - 1)[0] == 0


def test_plan_is_the_models(fv):
    for case in TABLE.cases:
        lens, skips = lens_of(case.idx), TABLE.skips(case)
        for pcm16 in (False, True):
            got = fv.clips_plan_strided(lens, skips, case.step, pcm16)
            want = st.plan_strided(lens, skips, case.step, pcm16)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (case, pcm16)
            assert not np.any(got[1] % (8 if pcm16 else 4))                 # every slot on a 16-byte boundary
    lens = lens_of(slice(None))
    for pcm16 in (False, True):                                              # step 1 is fvad_clips_plan; skips NULL means all zero
        out_lens, offsets, total = fv.clips_plan_strided(lens, None, 1, pcm16)
        want = fv.clips_plan(TABLE.clips, pcm16)
        assert np.array_equal(out_lens, lens.astype(np.uint64)) and np.array_equal(offsets, want[0]) and total == want[1]
        a, b = fv.clips_plan_strided(lens, None, 3, pcm16), fv.clips_plan_strided(lens, np.zeros(len(lens), np.uint32), 3, pcm16)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert fv.clips_plan_strided([], None, 3)[2] == 0


def raw_plan(fv, lens, skips, step, out_format=0, null=()):
    lens = np.asarray(lens, np.uint64)
    n = len(lens)
    skips = None if skips is None else np.asarray(skips, np.uint32)
    out_lens, offsets, total = np.full(n + 1, 77, np.uint64), np.full(n + 1, 77, np.uint64), C.c_uint64(77)
    p64 = C.POINTER(C.c_uint64)
    status = fv.lib().fvad_clips_plan_strided(None if "lens" in null else lens.ctypes.data_as(p64),
                                              None if skips is None else skips.ctypes.data_as(C.POINTER(C.c_uint32)), n, step, out_format,
                                              None if "out_lens" in null else out_lens.ctypes.data_as(p64),
                                              None if "offsets" in null else offsets.ctypes.data_as(p64), None if "total" in null else C.byref(total))
    assert out_lens[n] == 77 and offsets[n] == 77
    return status, total.value


def test_plan_errors(fv):
    M = 2 ** 64
    for what, kw in (
            ("step 0", dict(lens=[10, 20], skips=None, step=0)),
            ("step above the limit", dict(lens=[10, 20], skips=None, step=st.STEP_MAX + 1)),
            ("a skip equal to the step", dict(lens=[10, 20], skips=[0, 3], step=3)),
            ("a skip above the step", dict(lens=[10, 20], skips=[2 ** 32 - 1, 0], step=3)),
            ("a skip with step 1", dict(lens=[10, 20], skips=[0, 1], step=1)),
            ("a clip of no samples", dict(lens=[10, 0], skips=None, step=3)),
            ("len equal to the skip: no sample kept", dict(lens=[10, 2], skips=[0, 2], step=3)),
            ("len below the skip", dict(lens=[1, 20], skips=[2, 0], step=3)),
            ("a bad format", dict(lens=[10, 20], skips=None, step=3, out_format=2)),
            ("a negative format", dict(lens=[10, 20], skips=None, step=3, out_format=-1)),
            ("NULL lens", dict(lens=[10, 20], skips=None, step=3, null=("lens",))),
            ("NULL out_lens", dict(lens=[10, 20], skips=None, step=3, null=("out_lens",))),
            ("NULL offsets", dict(lens=[10, 20], skips=None, step=3, null=("offsets",))),
            ("NULL total", dict(lens=[10, 20], skips=None, step=3, null=("total",))),
            ("a total that does not fit", dict(lens=[M - 1, M - 1], skips=None, step=1)),
            ("a total that does not fit after rounding", dict(lens=[M - 2], skips=None, step=1))):
        status, total = raw_plan(fv, **kw)
        assert status == INVALID and total == 77, what
    # lengths near 2^64 whose kept thirds fit
    assert raw_plan(fv, [M - 1, M - 1], [0, 1], 3) == (0, sum((-(-(M - 1 - k) // 3) + 3) // 4 * 4 for k in (0, 1)))
    assert raw_plan(fv, [M - 1, M - 1, M - 1], [0, 1, 2], 3) == (INVALID, 77)   # three thirds of it do not
    assert raw_plan(fv, [3], [2], 3) == (0, 4) and raw_plan(fv, [1], None, st.STEP_MAX) == (0, 4)
    assert raw_plan(fv, [], None, 3, null=("lens", "out_lens", "offsets")) == (0, 0)


# ------------------------------------------------------------------ the table bites
@pytest.fixture(scope="module")
def models():
    src = TABLE.source(False)
    return src, cc.model_export(src, TABLE.clips, False)


def fails(got, want):
    try:
        cc.compare(got, want)
    except AssertionError:
        return True
    return False


def test_the_right_model_passes_and_each_wrong_model_fails(models):
    src, full = models
    caught = {m: 0 for m in ("skip0", "floor", "kept")}
    for case in TABLE.cases:
        clips, skips, lens = TABLE.clips[case.idx], TABLE.skips(case), lens_of(case.idx)
        want = st.strided_of(full, case.idx, skips, case.step, False, lens)
        right = st.model_export_strided(src, clips, skips, case.step, False)
        cc.compare(right, want, str(case))
        assert [len(s) for s in right["samples"]] == [st.out_len(n, k, case.step) for n, k in zip(lens, skips)]
        for m in caught:
            assert fails(st.model_export_strided(src, clips, skips, case.step, False, mutation=m), want), (case, m)
            caught[m] += 1
        # which clips tell: a clip with skip != 0 has other samples when the phase is counted from its first sample ...
        one = [int(np.flatnonzero(skips != 0)[0])] if np.any(skips) else None
        if one:
            assert fails(st.model_export_strided(src, clips[one], skips[one], case.step, False, "skip0"), st.strided_of(full, case.idx[one], skips[one], case.step, False, lens[one]))
        # ... one whose stride does not end on its last sample loses that sample to floor ...
        rest = (lens - skips) % case.step
        one = [int(np.flatnonzero((rest != 0) & (lens - skips > case.step))[0])]
        assert fails(st.model_export_strided(src, clips[one], skips[one], case.step, False, "floor"), st.strided_of(full, case.idx[one], skips[one], case.step, False, lens[one]))
        # ... and every clip of more than a few samples has another RMS over a third of them (far more than an ulp)
        one = [int(np.flatnonzero(lens > 1000)[0])]
        assert fails(st.model_export_strided(src, clips[one], skips[one], case.step, False, "kept"), st.strided_of(full, case.idx[one], skips[one], case.step, False, lens[one]))
    assert all(v == len(TABLE.cases) for v in caught.values())
    # phase 0 over clips that all start on a multiple of the step could not tell skip0 apart: the table's starts cover every residue
    for case in TABLE.cases:
        assert set(int(k) for k in TABLE.skips(case)) == set(range(case.step)), case


def test_the_table_holds_the_gather_tiles_edges():
    for case in TABLE.cases:
        To = st.tile_out(case.step)
        assert To % 8 == 0 and (To - 1) * case.step + 1 <= st.TILE < (To + 8) * case.step
        outs = [st.out_len(n, k, case.step) for n, k in zip(lens_of(case.edge), TABLE.skips(case, case.edge))]
        assert outs == [t for t in (To - 1, To, To + 1, 2 * To + 1, 1) for _ in range(8)]
        assert sorted(int(a) % 8 for a in TABLE.clips[case.edge[:8], 2]) == list(range(8))
        assert len(case.refused) > 0 and all(lens_of([k])[0] <= TABLE.skips(case, [k])[0] for k in case.refused)
    assert st.tile_out(3) == 2728 and (2728 - 1) * 3 + 1 == 8182


def test_a_stride_restarted_at_the_seam_fails(models):
    src, _ = models
    for case in (TABLE.cases[1], TABLE.cases[4], TABLE.cases[9]):
        # a few of the case's edge clips at every seam
        sub = st.Case(case.step, case.phase, case.idx, case.refused, case.edge[[0, 9, 34]])
        lay, skips = st.split_case(TABLE, sub, src)
        right = st.model_export_split_strided(lay, skips, case.step, False)
        lens = (lay.rows[:, 3] + lay.rows[:, 6]).astype(np.int64)
        want = st.model_export_strided(src, TABLE.clips[lay.base], skips, case.step, False)
        cc.compare(right, want, f"split {case}")                           # wherever the seam is: the contiguous clip's result
        wrong = st.model_export_split_strided(lay, skips, case.step, False, mutation="restart")
        assert fails(wrong, want), case
        # the rows that tell: the seam inside the clip and not a whole number of steps behind the first kept sample
        tells = [i for i in range(len(lay.rows)) if wrong["samples"][i].tobytes() != right["samples"][i].tobytes()]
        assert tells and all(0 < lay.sigma[i] < lens[i] and (lay.sigma[i] - int(skips[i])) % case.step != 0 for i in tells)
        # the seams around the first kept sample and directly before and after a kept sample are there
        k, n = int(skips[0]), int(lens[0])
        mine = set(int(s) for s in lay.sigma[lay.base == lay.base[0]])
        mid = k + (n // 2 - k) // case.step * case.step
        assert {s for s in (k - 1, k, k + 1, mid, mid + 1) if 0 <= s <= n} <= mine


def test_run_clips_refuses_other_rates_before_any_work(pkg, tmp_path):
    for kw in (dict(denoised_rate=44100), dict(original_rate=8000), dict(denoised_rate=16000, original_rate=0), dict(denoised_rate="16000")):
        with pytest.raises(ValueError):
            pkg.simulator.run_clips(str(tmp_path / "no-such-plan.json"), str(tmp_path / "out"), **kw)
    assert not (tmp_path / "out").exists()
