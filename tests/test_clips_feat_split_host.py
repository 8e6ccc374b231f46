"""The split-source feature exports without a device: fvad_clips_split_mel_check and fvad_clips_split_fbank_check rule by rule in
the order include/fvad.h states, the numpy model of the split read (clip_feat_split_cases.py) against the contiguous model over
the whole seam table, four wrong split models shown to be far off, and what run_clips refuses around features_sliced."""
import numpy as np
import pytest

import clip_fbank_cases as fc
import clip_feat_split_cases as sc
import clip_mel_cases as mc

INVALID, OUT_OF_RANGE, TOO_SMALL = -100, -6, -106
F32, PCM16 = 0, 1
MEL, FBANK = mc.SHAPES[0], fc.SHAPES[0]


def _checkers(fv):
    """per family: (status(**changes) over one good call of two split clips, the plan's (offsets, total))"""
    a, b = (0x10000, 3, 7000, 6000), (0x80000, 2, 9000, 8000)
    clips = np.array([[2, 0, 100, 1000, 0, 50, 2000], [1, 2, 7, 0, 1, 9, 5000]], np.uint64)    # lens 3000 and 5000
    skips = [1, 2]
    w_m, M_m = mc.hann(400), mc.matrix_for(MEL)
    w_f, M_f = fc.povey(400), fc.matrix_for(FBANK)
    shared = dict(a=a, b=b, src_format=F32, clips=clips, out=0x400000, out_capacity=1 << 20, device_out=True, step=3, skips=skips)
    mel = dict(shared, n_fft=400, hop=160, window=w_m, n_mels=80, matrix=M_m, floor=1e-10, norm=None)
    fbank = dict(shared, win_length=400, n_fft=512, hop=160, window=w_f, n_mels=80, matrix=M_f, scale=32768.0, preemph=0.97, remove_dc=1,
                 floor=2.0 ** -23, cmn=1)
    return {"mel": (lambda **kw: fv.clips_split_mel_check(**dict(mel, **kw)), fv.clips_plan_mel([3000, 5000], skips, 3, 400, 160, 80)),
            "fbank": (lambda **kw: fv.clips_split_fbank_check(**dict(fbank, **kw)), fv.clips_plan_fbank([3000, 5000], skips, 3, 400, 160, 80))}


@pytest.mark.parametrize("family", ["mel", "fbank"])
def test_check_rules_in_order(fv, family):
    check, (frames, offsets, total) = _checkers(fv)[family]
    st, got_frames, got_offsets, got_total = check()
    assert st == 0 and got_total == total and got_offsets.tolist() == offsets.tolist() and got_frames.tolist() == frames.tolist()
    assert check(out_capacity=total)[0] == 0 and check(device_out=False, out=0x400004)[0] == 0
    bad_w, bad_m = np.ones(400, np.float32), np.ones((80, 201 if family == "mel" else 257), np.float32)
    bad_w[7], bad_m[3, 5] = np.nan, np.inf
    past_a = [[2, 0, 5001, 1000, 0, 50, 2000], [1, 2, 7, 0, 1, 9, 5000]]
    past_b = [[2, 0, 100, 1000, 1, 50, 2000], [1, 2, 7, 0, 1, 9, 5000]]
    # the stated order, group by group; every entry is refused with its group's status
    groups = [
        ("split rules to the rows' own", INVALID, [dict(out=0), dict(src_format=2), dict(out_format=5), dict(window=None), dict(matrix=None),
                                                   dict(out_format=PCM16), dict(a=(0,) + (3, 7000, 6000)), dict(b=(0,) + (2, 9000, 8000)),
                                                   dict(a=(0x10002, 3, 7000, 6000)), dict(out=0x400004), dict(a=(0x10000, 3, 5999, 6000)),
                                                   dict(b=(0x80000, 2, 7999, 8000)), dict(clips=[[2, 0, 100, 0, 0, 50, 0], [1, 2, 7, 0, 1, 9, 5000]]),
                                                   dict(clips=[[0, 0, 100, 1000, 0, 50, 2000], [1, 2, 7, 0, 1, 9, 5000]])]),
        ("the family's rules", INVALID, [dict(step=0), dict(step=17), dict(n_fft=2050), dict(hop=0), dict(hop=401), dict(n_mels=0), dict(n_mels=129),
                                         dict(skips=[3, 0]), dict(clips=[[2, 0, 100, 100, 0, 50, 3 * 399 - 100 + 1 - 3 * 199 * (family == "mel")], [1, 2, 7, 0, 1, 9, 5000]]),
                                         dict(window=bad_w), dict(matrix=bad_m), dict(floor=0.0), dict(floor=float("nan"))]
         + ([dict(n_fft=399), dict(norm=[8.0, np.inf, 0.25])] if family == "mel" else
            [dict(win_length=1), dict(win_length=513), dict(scale=0.0), dict(preemph=1.5), dict(remove_dc=2), dict(cmn=2)])),
        ("the pieces' ranges", OUT_OF_RANGE, [dict(clips=past_a), dict(clips=past_b), dict(a=(0x10000, 1, 7000, 6000)), dict(b=(0x80000, 2, 9000, 2049))]),
        ("the capacity", TOO_SMALL, [dict(out_capacity=total - 1), dict(out_capacity=0)]),
        ("the output over a source", INVALID, [dict(out=0x10000), dict(out=0x80000 + 16), dict(out=0x10000 - 16)]),
    ]
    for what, want, cases in groups:
        for kw in cases:
            assert check(**kw)[0] == want, (what, kw)
    # an earlier group's rule wins over every later group's
    for g, (what, want, cases) in enumerate(groups):
        for later_what, _, later in groups[g + 1:]:
            kw = dict(later[0], **cases[0])
            assert check(**kw)[0] == want, (what, "before", later_what)
    # within the first group: the feature NULLs and the output format sit directly behind the format rule, in front of the NULL sources
    assert check(window=None, a=(0,) + (3, 7000, 6000))[0] == INVALID and check(src_format=2, window=None)[0] == INVALID
    # the slot walk fills what it reached: a refusal behind the family's rules still reports the plan
    st, _, got_offsets, got_total = check(out_capacity=total - 1)
    assert st == TOO_SMALL and got_total == total and got_offsets.tolist() == offsets.tolist()
    # no clips: nothing is asked
    assert check(clips=np.zeros((0, 7), np.uint64), skips=None, window=None, matrix=None, out=0)[0] == 0
    # too many tiles of frames for one grid comes last: a clip of 2^40 samples at hop 1, its pieces in range
    tiny = dict(n_fft=4, hop=1, n_mels=1, window=np.ones(4, np.float32), matrix=np.ones((1, 3), np.float32))
    if family == "fbank":
        tiny["win_length"] = 4
    huge = dict(tiny, clips=[[1, 0, 0, 1 << 39, 0, 0, 1 << 39]], skips=None, step=1, a=(0x10000, 1, 1 << 39, 1 << 39), b=(1 << 50, 1, 1 << 39, 1 << 39),
                out=1 << 60, out_capacity=1 << 62)
    assert check(**huge)[0] == INVALID and check(**dict(huge, out_capacity=0))[0] == TOO_SMALL


def _noise_clip(n, seed=5):
    return (0.3 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("step", [1, 3])
def test_split_model_is_the_contiguous_model_over_the_seam_table(step):
    for skip in range(step):
        n = skip + (40 * 4 + 5 - 1) * step + 1 + (step - 1)
        x = _noise_clip(n, seed=step + skip)
        whole = x[skip::step]
        for taps, hop, centred in ((8, 4, True), (6, 4, False)):
            table = sc.seams(n, skip, step, taps, hop, centred, tile_frames=32)
            assert {0, 1, skip, skip + 1, n - 1, n} <= set(table) and len(table) >= 12
            assert {s % step for s in table} == set(range(step)), "a mid seam at every residue"
            for a_len in table:
                got = sc.split_stream(x[:a_len], x[a_len:], skip, step)
                assert got.tobytes() == whole.tobytes(), (step, skip, a_len)
                assert sc.n_a(a_len, skip, step) == len(x[:a_len][skip::step])


def test_wrong_split_models_are_far_off():
    """each wrong read of the seam moves a feature by more than 50 tolerances on a noise clip"""
    step, skip, hop = 3, 1, 160
    w, M = mc.hann(400), mc.matrix_for(MEL)
    wf, Mf = fc.povey(400), fc.matrix_for(FBANK)
    n = skip + (12 * hop + 7 - 1) * step + 2
    x = _noise_clip(n)
    a_len = n // 2 - (n // 2 - skip) % step + 1                     # off the stride: the stride lands 2 samples into B
    assert (a_len - skip) % step == 1
    right = sc.split_stream(x[:a_len], x[a_len:], skip, step)
    ref, U = mc.model(right, w, M, hop)
    ref_f, U_f = fc.model(right, wf, Mf, FBANK, scale=32768.0)
    for mutation in ("drop", "dup", "b_from"):
        wrong = sc.split_stream(x[:a_len], x[a_len:], skip, step, mutation)
        got, _ = mc.model(wrong, w, M, hop)
        T = min(len(got), len(ref))
        d = mc.distance(got[:T], ref[:T], U[:T])
        got_f, _ = fc.model(wrong, wf, Mf, FBANK, scale=32768.0)
        Tf = min(len(got_f), len(ref_f))
        d_f = fc.distance(got_f[:Tf], ref_f[:Tf], U_f[:Tf])
        print(f"{mutation}: {d:.0f} units log-mel, {d_f:.0f} units fbank")
        assert d > 50 * mc.TOL and d_f > 50 * fc.TOL, mutation
    # reflection from piece A only, the seam inside the left reflected zone (a_len < step n_fft / 4)
    a_len = step * 60 + 2
    assert a_len < step * 400 // 4
    got = sc.mel_reflect_a_only(x[:a_len], x[a_len:], skip, step, w, M, hop)
    d = mc.distance(got, ref, U)
    print(f"reflection from A only: {d:.0f} units")
    assert d > 50 * mc.TOL
    # and the right read of the same seam is the model itself
    same = sc.mel_reflect_a_only(x, x[:0], skip, step, w, M, hop)
    assert mc.distance(same, ref, U) < 1e-6


def test_public_signatures_of_the_split_feature_calls(fv):
    import inspect
    want = {
        "Context.clips_export_split_mel": "(self, a, b, src_pcm16, clips, window, matrix, step=1, skips=None, hop=160, floor=1e-10, norm=None, d_out=None, "
                                          "out_capacity=None)",
        "Context.clips_export_split_fbank": "(self, a, b, src_pcm16, clips, window, matrix, n_fft=512, step=1, skips=None, hop=160, scale=32768.0, preemph=0.97, "
                                            "remove_dc=True, floor=1.1920928955078125e-07, cmn=False, d_out=None, out_capacity=None)",
        "clips_split_mel_check": "(a, b, src_format, clips, out, out_capacity, device_out, step, skips, n_fft, hop, window, n_mels, matrix, floor, norm, "
                                 "out_format=0)",
        "clips_split_fbank_check": "(a, b, src_format, clips, out, out_capacity, device_out, step, skips, win_length, n_fft, hop, window, n_mels, matrix, "
                                   "scale, preemph, remove_dc, floor, cmn, out_format=0)"}
    for name, sig in want.items():
        f = fv
        for part in name.split("."):
            f = getattr(f, part)
        assert str(inspect.signature(f)) == sig, name


def test_what_run_clips_refuses_around_features_sliced(pkg, tmp_path):
    sim = pkg.simulator
    out, plan = tmp_path / "never", str(tmp_path / "no-such-plan.json")
    for features in ("logmel", "fbank"):
        with pytest.raises(ValueError, match="split-source"):       # the pinned refusal stays, and names the opt-in
            sim.run_clips(plan, str(out), features=features, slice_chunks=16)
        with pytest.raises(ValueError, match="features_sliced"):
            sim.run_clips(plan, str(out), features=features, slice_chunks=16)
        with pytest.raises(ValueError, match="features_sliced"):
            sim.run_clips(plan, str(out), features=features, features_sliced=True)
        # with all three the refusal is gone: the run gets as far as the plan that does not exist
        with pytest.raises(Exception) as e:
            sim.run_clips(plan, str(out), features=features, slice_chunks=16, features_sliced=True)
        assert not isinstance(e.value, ValueError) or "features" not in str(e.value), e.value
        assert isinstance(e.value, OSError), e.value
    with pytest.raises(ValueError, match="features_sliced"):
        sim.run_clips(plan, str(out), slice_chunks=16, features_sliced=True)
    for argv in (["-i", plan, "--export-clips", str(out), "--clips-features", "logmel", "--clips-features-sliced"],
                 ["-i", plan, "--export-clips", str(out), "--slice-chunks", "16", "--clips-features-sliced"],
                 ["-i", plan, "--clips-features-sliced"]):
        with pytest.raises(ValueError):
            sim.main(argv)
    with pytest.raises(OSError):
        sim.main(["-i", plan, "--export-clips", str(out), "--clips-features", "fbank", "--slice-chunks", "16", "--clips-features-sliced"])
    assert not out.exists()
