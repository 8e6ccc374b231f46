"""The host side of the filter-bank clip export (no GPU): fvad_mel_design_kaldi against Kaldi's formula written out in numpy,
fvad_clips_plan_fbank's counts and slots against python integers and every refusal, every rule of fvad_clips_fbank_check in its
order, what run_clips and main() refuse before a context exists, the committed tolerance literal against its measurement, and
the proof that the case table bites: eight wrong versions of the float64 model."""
import ctypes as C

import numpy as np
import pytest

import clip_fbank_cases as fc

INVALID, OUT_OF_RANGE, TOO_SMALL = -100, -6, -106
U64 = (1 << 64) - 1
F32, PCM16 = 0, 1


# ------------------------------------------------------------------ the designer
@pytest.mark.parametrize("sr,n_fft,n_mels,low,high", [(16000, 512, 80, 20, 0), (16000, 512, 128, 20, 0), (16000, 8, 3, 20, 0), (16000, 400, 23, 20, -400),
                                                      (48000, 2048, 40, 50, 12000), (22050, 254, 5, 300.5, 11025), (16000, 4, 1, 0, 8000)])
def test_design_is_kaldi_formula(fv, sr, n_fft, n_mels, low, high):
    got, want = fv.mel_design_kaldi(sr, n_fft, n_mels, low, high), fc.design(sr, n_fft, n_mels, low, high)
    assert got.shape == want.shape == (n_mels, n_fft // 2 + 1) and got.dtype == np.float32
    # both evaluate the same expression in double and round once: log may differ in the last place of the double
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23 and (got >= 0).all()
    assert (np.abs(got - want) > 0).mean() < 0.01
    assert (got[:, -1] == 0).all(), "the Nyquist column"
    assert got.max() <= 1.0, "no normalisation: a triangle peaks at 1 at most"
    for row in got:   # a band's support is one run of bins
        nz = np.flatnonzero(row)
        assert nz.size == 0 or nz[-1] - nz[0] + 1 == nz.size
    if n_mels >= 23 and n_mels <= 80 and n_fft >= 400:
        assert (got.sum(axis=1) > 0).all()   # every band sees a bin
        assert (np.diff(got.argmax(axis=1)) >= 0).all()


def test_design_high_freq_counts_from_nyquist(fv):
    assert fv.mel_design_kaldi(16000, 512, 80, 20, 0).tobytes() == fv.mel_design_kaldi(16000, 512, 80, 20, 8000).tobytes()
    assert fv.mel_design_kaldi(16000, 512, 80, 20, -400).tobytes() == fv.mel_design_kaldi(16000, 512, 80, 20, 7600).tobytes()


def test_design_refusals(fv):
    for args in ((16000, 512, 80, -1.0, 8000), (16000, 512, 80, 0, 8000.5), (16000, 512, 80, 4000, 4000), (16000, 512, 80, 5000, 4000),
                 (16000, 512, 80, 20, -8000), (0, 512, 80, 0, 0), (-16000, 512, 80, 0, 8000), (float("nan"), 512, 80, 0, 8000), (16000, 401, 80, 0, 8000),
                 (16000, 2, 80, 0, 8000), (16000, 2050, 80, 0, 8000), (16000, 512, 0, 0, 8000), (16000, 512, 129, 0, 8000),
                 (16000, 512, 80, float("nan"), 8000), (16000, 512, 80, 0, float("nan"))):
        with pytest.raises(fv.FvadError) as e:
            fv.mel_design_kaldi(*args)
        assert e.value.status == INVALID, args
    assert fv.lib().fvad_mel_design_kaldi(16000.0, 512, 80, 20.0, 0.0, None) == INVALID


# ------------------------------------------------------------------ the plan
def plan_py(lens, skips, step, win, hop, n_mels):
    frames, offsets, at = [], [], 0
    for n, k in zip(lens, skips):
        L = -(-(n - k) // step)
        frames.append(1 + (L - win) // hop)
        offsets.append(at)
        at += (frames[-1] * n_mels + 3) // 4 * 4
    return frames, offsets, at


@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "/".join(map(str, s)))
def test_plan_counts_and_slots(fv, shape):
    win, _, hop, n_mels = shape
    rng = np.random.default_rng(win)
    for step in (1, 3, 16):
        Ls = [win, win + hop - 1, win + hop, win + 7 * hop + hop // 2] + [int(v) for v in rng.integers(win, 40 * win, 12)]
        skips = [int(v) for v in rng.integers(0, step, len(Ls))]
        lens = [k + (L - 1) * step + 1 + int(rng.integers(0, step)) for L, k in zip(Ls, skips)]
        frames, offsets, total = fv.clips_plan_fbank(lens, skips, step, win, hop, n_mels)
        want = plan_py(lens, skips, step, win, hop, n_mels)
        assert [int(v) for v in frames] == want[0] == [fc.n_frames(L, win, hop) for L in Ls]
        assert [int(v) for v in frames[:3]] == [1, 1, 2]
        assert [int(v) for v in offsets] == want[1] and total == want[2] and all(int(o) % 4 == 0 for o in offsets)
        # L = win - 1: refused
        with pytest.raises(fv.FvadError) as e:
            fv.clips_plan_fbank([(win - 2) * step + 1], None, step, win, hop, n_mels)
        assert e.value.status == INVALID
    assert fv.clips_plan_fbank([], None, 1, win, hop, n_mels)[2] == 0


def test_plan_refusals(fv):
    good = dict(lens=[3000, 2000], skips=[1, 2], step=3, win_length=400, hop=160, n_mels=80)

    def refused(**kw):
        a = dict(good, **kw)
        with pytest.raises(fv.FvadError) as e:
            fv.clips_plan_fbank(a["lens"], a["skips"], a["step"], a["win_length"], a["hop"], a["n_mels"])
        return e.value.status == INVALID
    fv.clips_plan_fbank(**good)
    for kw in (dict(step=0), dict(step=17), dict(win_length=1), dict(win_length=2049), dict(hop=0), dict(hop=401), dict(n_mels=0),
               dict(n_mels=129), dict(skips=[3, 0]), dict(lens=[1, 2000], skips=[1, 0]),
               dict(lens=[3 * 399 + 1, 2000], skips=[1, 0]),     # L = 399 < win
               dict(lens=[U64, U64], skips=None, step=1, win_length=2, hop=1, n_mels=128)):   # the total does not fit 64 bits
        assert refused(**kw), kw
    assert int(fv.clips_plan_fbank([3 * 399 + 2], [1], 3, 400, 160, 80)[0][0]) == 1   # exactly win stream samples pass
    assert fv.clips_plan_fbank([5], None, 1, 5, 2, 2)[0].tolist() == [1]               # an odd win_length


# ------------------------------------------------------------------ the check, rule by rule in its order
def test_check_rules_in_order(fv):
    shape = fc.SHAPES[0]
    w, M = fc.povey(400), fc.matrix_for(shape)
    clips = np.array([[0, 2, 10, 10 + 3000], [1, 1, 7, 7 + 5000]], np.uint64)
    skips = [fc.phase_skip(10, 3, 2), fc.phase_skip(7, 3, 2)]
    good = dict(d_src=0x10000, src_format=F32, n_lanes=2, lane_stride=6000, n_samples=6000, clips=clips, out=0x20000, out_capacity=1 << 20,
                device_out=True, step=3, skips=skips, win_length=400, n_fft=512, hop=160, window=w, n_mels=80, matrix=M, scale=32768.0,
                preemph=0.97, remove_dc=1, floor=2.0 ** -23, cmn=1)
    st, frames, offsets, total = fv.clips_fbank_check(**good)
    want = fv.clips_plan_fbank([3000, 5000], skips, 3, 400, 160, 80)
    assert st == 0 and frames.tolist() == want[0].tolist() and offsets.tolist() == want[1].tolist() and total == want[2]

    def status(**kw):
        return fv.clips_fbank_check(**dict(good, **kw))[0]
    bad_w, bad_m = w.copy(), M.copy()
    bad_w[399], bad_m[79, 200] = np.inf, np.nan
    rules = [  # each entry breaks its own rule and every LATER one's argument stays good; then pairs show the order
        (dict(d_src=0), INVALID), (dict(out=0), INVALID), (dict(window=None), INVALID), (dict(matrix=None), INVALID),
        (dict(src_format=2), INVALID), (dict(out_format=PCM16), INVALID), (dict(out=0x20004), INVALID), (dict(d_src=0x10002), INVALID),
        (dict(lane_stride=5999), INVALID), (dict(clips=[[0, 2, 10, 10], [1, 1, 7, 5007]]), INVALID), (dict(clips=[[0, 0, 10, 3010]], skips=skips[:1]), INVALID),
        (dict(step=0), INVALID), (dict(step=17), INVALID), (dict(n_fft=511), INVALID), (dict(n_fft=2050), INVALID), (dict(n_fft=398), INVALID),
        (dict(win_length=1), INVALID), (dict(win_length=513), INVALID), (dict(hop=0), INVALID), (dict(hop=401), INVALID),
        (dict(n_mels=0), INVALID), (dict(n_mels=129), INVALID), (dict(skips=[3, 0]), INVALID),
        (dict(clips=[[0, 2, 10, 10 + 3 * 399], [1, 1, 7, 5007]]), INVALID), (dict(window=bad_w), INVALID), (dict(matrix=bad_m), INVALID),
        (dict(scale=0.0), INVALID), (dict(scale=float("inf")), INVALID), (dict(scale=float("nan")), INVALID),
        (dict(preemph=-0.01), INVALID), (dict(preemph=1.01), INVALID), (dict(preemph=float("nan")), INVALID),
        (dict(remove_dc=2), INVALID), (dict(remove_dc=-1), INVALID),
        (dict(floor=0.0), INVALID), (dict(floor=-1e-10), INVALID), (dict(floor=float("inf")), INVALID), (dict(floor=float("nan")), INVALID),
        (dict(cmn=2), INVALID), (dict(n_samples=5006), OUT_OF_RANGE), (dict(clips=[[1, 2, 10, 3010], [1, 1, 7, 5007]]), OUT_OF_RANGE),
        (dict(clips=[[2, 1, 10, 3010], [1, 1, 7, 5007]]), OUT_OF_RANGE), (dict(out_capacity=total - 1), TOO_SMALL)]
    for kw, want_st in rules:
        assert status(**kw) == want_st, kw
    assert status(out_capacity=total) == 0 and status(cmn=0, remove_dc=0, preemph=0.0) == 0 and status(preemph=1.0, scale=-1.0) == 0
    assert status(device_out=False, out=0x20004) == 0 and status(win_length=512, hop=512, window=np.ones(512, np.float32)) == 0
    # the window is read up to win_length only
    long_w = np.concatenate([w, [np.nan]]).astype(np.float32)
    assert status(window=long_w) == 0
    # the order: an earlier rule wins over a later one
    assert status(n_samples=5006, out_capacity=0) == OUT_OF_RANGE and status(floor=0.0, n_samples=5006) == INVALID
    assert status(step=0, out_capacity=0) == INVALID and status(src_format=2, n_samples=1) == INVALID
    assert status(cmn=2, n_samples=5006) == INVALID and status(scale=0.0, out_capacity=0) == INVALID
    # n_clips == 0 asks nothing
    assert fv.clips_fbank_check(**dict(good, clips=np.zeros((0, 4), np.uint64), d_src=0, out=0, window=None, matrix=None, skips=None))[0] == 0
    # too many tiles of frames for one grid: a clip of 2^40 samples at hop 1
    huge = dict(good, clips=[[0, 1, 0, 1 << 40]], skips=None, step=1, win_length=4, n_fft=4, hop=1, n_mels=1, window=np.ones(4, np.float32),
                matrix=np.ones((1, 3), np.float32), n_samples=1 << 40, lane_stride=1 << 40, out_capacity=1 << 62)
    assert fv.clips_fbank_check(**huge)[0] == INVALID


def test_check_without_the_frame_arrays(fv):
    """n_frames and offsets NULL, as the host-output export calls the rules: the status and the total of the call with them, for
    accepted and refused inputs of test_check_rules_in_order; an accepted input's total is the plan's"""
    w, M = fc.povey(400), fc.matrix_for(fc.SHAPES[0])
    clips = np.array([[0, 2, 10, 10 + 3000], [1, 1, 7, 7 + 5000]], np.uint64)
    skips = [fc.phase_skip(10, 3, 2), fc.phase_skip(7, 3, 2)]
    good = dict(d_src=0x10000, n_lanes=2, lane_stride=6000, n_samples=6000, clips=clips, out=0x20000, out_capacity=1 << 20, device_out=True, step=3,
                skips=skips, win_length=400, n_fft=512, hop=160, window=w, n_mels=80, matrix=M, scale=32768.0, preemph=0.97, remove_dc=1,
                floor=2.0 ** -23, cmn=1)
    plan = fv.clips_plan_fbank([3000, 5000], skips, 3, 400, 160, 80)[2]

    def raw(null, d_src, n_lanes, lane_stride, n_samples, clips, out, out_capacity, device_out, step, skips, win_length, n_fft, hop, window, n_mels, matrix,
            scale, preemph, remove_dc, floor, cmn):
        r = np.ascontiguousarray(np.asarray(clips, np.uint64).reshape(-1, 4))
        k = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32))
        keep = [np.ascontiguousarray(np.asarray(a, np.float32)) for a in (window, matrix)]
        frames, offsets, total = np.zeros(len(r), np.uint64), np.zeros(len(r), np.uint64), C.c_uint64(0)
        st = fv.lib().fvad_clips_fbank_check(fv.vp(d_src), F32, n_lanes, lane_stride, n_samples, r.ctypes.data_as(C.POINTER(C.c_uint64)), len(r), F32, fv.vp(out),
                                             out_capacity, int(device_out), step, None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint32)), win_length,
                                             n_fft, hop, fv.fptr(keep[0]), n_mels, fv.fptr(keep[1]), scale, preemph, remove_dc, floor, cmn,
                                             None if null else frames.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             None if null else offsets.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(total))
        return st, int(total.value)
    bad_w = w.copy()
    bad_w[399] = np.inf
    huge = dict(clips=[[0, 1, 0, 1 << 40]], skips=None, step=1, win_length=4, n_fft=4, hop=1, n_mels=1, window=np.ones(4, np.float32),
                matrix=np.ones((1, 3), np.float32), n_samples=1 << 40, lane_stride=1 << 40, out_capacity=1 << 62)
    table = [(dict(), 0), (dict(out_capacity=plan), 0), (dict(cmn=0, remove_dc=0, preemph=0.0), 0), (dict(device_out=False, out=0x20004), 0),
             (dict(step=0), INVALID), (dict(win_length=513), INVALID), (dict(hop=401), INVALID), (dict(skips=[3, 0]), INVALID),
             (dict(clips=[[0, 2, 10, 10 + 3 * 399], [1, 1, 7, 5007]]), INVALID), (dict(window=bad_w), INVALID), (dict(scale=0.0), INVALID),
             (dict(cmn=2), INVALID), (dict(n_samples=5006), OUT_OF_RANGE), (dict(out_capacity=plan - 1), TOO_SMALL), (huge, INVALID)]
    for kw, want in table:
        args = dict(good, **kw)
        with_arrays, without = raw(False, **args), raw(True, **args)
        assert with_arrays[0] == want and without == with_arrays, kw
        assert fv.clips_fbank_check(src_format=F32, **args)[::3] == with_arrays, kw
        if want == 0:
            assert without[1] == plan, kw


def test_public_signatures_of_the_feature_calls(fv):
    """the Python entry points of both families, as literals: names, order and defaults"""
    import inspect
    want = {
        "Context.clips_export_mel": "(self, d_src, src_pcm16, n_lanes, lane_stride, n_samples, clips, window, matrix, step=1, skips=None, hop=160, "
                                    "floor=1e-10, norm=None, d_out=None, out_capacity=None)",
        "Context.clips_export_fbank": "(self, d_src, src_pcm16, n_lanes, lane_stride, n_samples, clips, window, matrix, n_fft=512, step=1, skips=None, "
                                      "hop=160, scale=32768.0, preemph=0.97, remove_dc=True, floor=1.1920928955078125e-07, cmn=False, d_out=None, "
                                      "out_capacity=None)",
        "clips_plan_mel": "(lens, skips, step, n_fft, hop, n_mels)",
        "clips_plan_fbank": "(lens, skips, step, win_length, hop, n_mels)",
        "clips_mel_check": "(d_src, src_format, n_lanes, lane_stride, n_samples, clips, out, out_capacity, device_out, step, skips, n_fft, hop, window, "
                           "n_mels, matrix, floor, norm, out_format=0)",
        "clips_fbank_check": "(d_src, src_format, n_lanes, lane_stride, n_samples, clips, out, out_capacity, device_out, step, skips, win_length, n_fft, "
                             "hop, window, n_mels, matrix, scale, preemph, remove_dc, floor, cmn, out_format=0)"}
    for name, sig in want.items():
        f = fv
        for part in name.split("."):
            f = getattr(f, part)
        assert str(inspect.signature(f)) == sig, name


# ------------------------------------------------------------------ the harness's refusals
def test_what_run_clips_and_main_refuse(pkg, tmp_path):
    out = tmp_path / "never"
    sim = pkg.simulator
    plan = str(tmp_path / "no-such-plan.json")
    for kw in (dict(features="fbank", features_norm="whisper"), dict(features="logmel", features_norm="cmn"), dict(features_norm="cmn"),
               dict(features="fbank", features_norm="zscore"), dict(features="fbank", slice_chunks=16), dict(features="Fbank")):
        with pytest.raises(ValueError):
            sim.run_clips(plan, str(out), **kw)   # (neither a plan nor a context is ever opened)
    with pytest.raises(ValueError, match="split-source"):
        sim.run_clips(plan, str(out), features="fbank", slice_chunks=16)
    with pytest.raises(ValueError, match="split-source"):
        sim.run_clips(plan, str(out), features="fbank", features_norm="cmn", slice_chunks=16)
    for argv in (["-i", plan, "--export-clips", str(out), "--clips-features", "fbank", "--clips-features-norm", "whisper"],
                 ["-i", plan, "--export-clips", str(out), "--clips-features", "logmel", "--clips-features-norm", "cmn"],
                 ["-i", plan, "--export-clips", str(out), "--clips-features-norm", "cmn"],
                 ["-i", plan, "--export-clips", str(out), "--clips-features", "fbank", "--slice-chunks", "16"],
                 ["-i", plan, "--clips-features", "fbank"]):
        with pytest.raises(ValueError):
            sim.main(argv)
    assert not out.exists()
    # what the harness passes on is what the tests model
    assert sim.fbank_window().tobytes() == fc.povey(400).tobytes()
    p = sim.FBANK
    assert (p["win_length"], p["n_fft"], p["hop"], p["n_mels"]) == fc.SHAPES[0] and p["step"] == 3 and p["scale"] == 32768.0 and p["remove_dc"] == 1
    assert np.float32(p["preemph"]) == fc.PREEMPH and np.float32(p["floor"]) == fc.FLOOR == np.finfo(np.float32).eps
    assert (p["sample_rate"], p["low_freq"], p["high_freq"]) == (16000, 20.0, 0.0)


# ------------------------------------------------------------------ the yardstick
@pytest.fixture(scope="module")
def table():
    t = fc.case_table()
    return t, [c.model() for c in t]


def test_the_table_has_its_cases(table):
    cases, _ = table
    assert len(cases) == 9 * 3 * 2 and {c.shape for c in cases} == {(400, 512, 160, 80), (512, 512, 128, 128), (6, 8, 4, 3)}
    assert {c.scale for c in cases} == {1.0, 32768.0} and len({c.name for c in cases}) == 9


def test_f32_worst_distance_is_the_committed_literal(table):
    cases, refs = table
    worst = max(fc.distance(c.f32(), ref, U) for c, (ref, U) in zip(cases, refs))
    assert round(worst, 4) == fc.F32_WORST, worst
    assert fc.F32_WORST < 10, "a healthy evaluation costs a few units: the unit is wrong"
    assert fc.TOL == 4 * fc.F32_WORST


def test_silence_is_exact_in_the_model():
    shape = fc.SHAPES[0]
    w, M = fc.povey(400), fc.matrix_for(shape)
    for scale in fc.SCALES:
        feat, _ = fc.model(np.zeros(1000, np.float32), w, M, shape, scale=scale)
        assert feat.shape == (4, 80) and (feat == np.log(np.float64(fc.FLOOR))).all()
    # a constant is silence once its DC is removed
    feat, _ = fc.model(np.full(1000, 0.5, np.float32), w, M, shape)
    assert (feat == np.log(np.float64(fc.FLOOR))).all()
    assert np.float32(np.log(np.float64(fc.FLOOR))) == np.float32(-15.942385)


@pytest.mark.parametrize("mutation", ["y0", "pre-first", "mean-nfft", "centred", "win-first", "log10", "phase1", "loud"])
def test_the_table_tells_a_wrong_model(table, mutation):
    cases, refs = table
    worst = 0.0
    for c, (ref, U) in zip(cases, refs):
        got, _ = c.model(mutation)
        T = min(len(got), len(ref))   # (another phase or framing may give another count: compare the frames both have)
        worst = max(worst, fc.distance(got[:T], ref[:T], U[:T]))
    assert worst > 50 * fc.TOL, (mutation, worst / fc.TOL)


def test_a_dropped_last_frame_fails_the_count(table):
    cases, refs = table
    for c, (ref, _) in zip(cases, refs):
        assert c.model("lastframe")[0].shape[0] == ref.shape[0] - 1
        with pytest.raises(AssertionError):
            fc.distance(c.model("lastframe")[0], ref, refs[0][1])
