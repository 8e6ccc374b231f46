"""The host side of the log-mel clip export (no GPU): fvad_mel_design against Slaney's formula written out in numpy,
fvad_clips_plan_mel's counts and slots against python integers and every refusal, every rule of fvad_clips_mel_check in its
order, what run_clips and main() refuse before a context exists, the committed tolerance literal against its measurement, and
the proof that the case table bites: six wrong versions of the float64 model."""
import ctypes as C

import numpy as np
import pytest

import clip_mel_cases as mc

INVALID, OUT_OF_RANGE, TOO_SMALL = -100, -6, -106
U64 = (1 << 64) - 1
F32, PCM16 = 0, 1


# ------------------------------------------------------------------ the designer
@pytest.mark.parametrize("sr,n_fft,n_mels,fmin,fmax", [(16000, 400, 80, 0, 8000), (16000, 512, 128, 0, 8000), (16000, 8, 3, 0, 8000),
                                                       (48000, 2048, 40, 50, 12000), (22050, 254, 5, 300.5, 11025), (16000, 4, 1, 0, 8000)])
def test_design_is_slaney_formula(fv, sr, n_fft, n_mels, fmin, fmax):
    got, want = fv.mel_design(sr, n_fft, n_mels, fmin, fmax), mc.design(sr, n_fft, n_mels, fmin, fmax)
    assert got.shape == want.shape == (n_mels, n_fft // 2 + 1) and got.dtype == np.float32
    # both evaluate the same expression in double and round once: log / exp may differ in the last place of the double
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23 * np.abs(want).max() and (got >= 0).all()
    assert (np.abs(got - want) > 0).mean() < 0.01
    if n_mels >= 3 and n_fft >= 254:
        assert (got.sum(axis=1) > 0).all()   # every band sees a bin


def test_design_has_whisper_properties(fv):
    M = fv.mel_design(16000, 400, 80, 0, 8000)
    # Slaney normalisation: a band's area in Hz is 1 wherever bins sample its triangle densely (the wide upper bands)
    assert abs(float(M[-1].sum()) * 40.0 - 1.0) < 0.05
    peak = M.argmax(axis=1)
    assert (np.diff(peak) >= 0).all() and peak[0] >= 1 and peak[-1] < 200


def test_design_refusals(fv):
    for args in ((16000, 400, 80, -1.0, 8000), (16000, 400, 80, 0, 8000.5), (16000, 400, 80, 4000, 4000), (16000, 400, 80, 5000, 4000),
                 (0, 400, 80, 0, 0), (-16000, 400, 80, 0, 8000), (float("nan"), 400, 80, 0, 8000), (16000, 401, 80, 0, 8000),
                 (16000, 2, 80, 0, 8000), (16000, 2050, 80, 0, 8000), (16000, 400, 0, 0, 8000), (16000, 400, 129, 0, 8000),
                 (16000, 400, 80, float("nan"), 8000), (16000, 400, 80, 0, float("nan"))):
        with pytest.raises(fv.FvadError) as e:
            fv.mel_design(*args)
        assert e.value.status == INVALID, args
    assert fv.lib().fvad_mel_design(16000.0, 400, 80, 0.0, 8000.0, None) == INVALID


# ------------------------------------------------------------------ the plan
def plan_py(lens, skips, step, n_fft, hop, n_mels):
    frames, offsets, at = [], [], 0
    for n, k in zip(lens, skips):
        L = -(-(n - k) // step)
        frames.append(L // hop)
        offsets.append(at)
        at += (frames[-1] * n_mels + 3) // 4 * 4
    return frames, offsets, at


@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "/".join(map(str, s)))
def test_plan_counts_and_slots(fv, shape):
    n_fft, hop, n_mels = shape
    rng = np.random.default_rng(n_fft)
    for step in (1, 3, 16):
        pad1 = n_fft // 2 + 1
        Ls = [max(pad1, hop), max(pad1, hop) + 1, 7 * hop + pad1, 8 * hop + pad1 - 1, 8 * hop + pad1 + 1] + [int(v) for v in rng.integers(max(pad1, hop), 40 * n_fft, 12)]
        skips = [int(v) for v in rng.integers(0, step, len(Ls))]
        lens = [k + (L - 1) * step + 1 + int(rng.integers(0, step)) for L, k in zip(Ls, skips)]
        frames, offsets, total = fv.clips_plan_mel(lens, skips, step, n_fft, hop, n_mels)
        want = plan_py(lens, skips, step, n_fft, hop, n_mels)
        assert [int(v) for v in frames] == want[0] == [L // hop for L in Ls]
        assert [int(v) for v in offsets] == want[1] and total == want[2] and all(int(o) % 4 == 0 for o in offsets)
    f0, o0, t0 = fv.clips_plan_mel([3 * n_fft + 5] * 2, None, 1, n_fft, hop, n_mels)
    assert [int(v) for v in f0] == [(3 * n_fft + 5) // hop] * 2 and int(o0[1]) == t0 // 2
    assert fv.clips_plan_mel([], None, 1, n_fft, hop, n_mels)[2] == 0


def test_plan_refusals(fv):
    good = dict(lens=[1000, 2000], skips=[1, 2], step=3, n_fft=400, hop=160, n_mels=80)

    def refused(**kw):
        a = dict(good, **kw)
        with pytest.raises(fv.FvadError) as e:
            fv.clips_plan_mel(a["lens"], a["skips"], a["step"], a["n_fft"], a["hop"], a["n_mels"])
        return e.value.status == INVALID
    fv.clips_plan_mel(**good)
    for kw in (dict(step=0), dict(step=17), dict(n_fft=2), dict(n_fft=401), dict(n_fft=2050), dict(hop=0), dict(hop=401), dict(n_mels=0),
               dict(n_mels=129), dict(skips=[3, 0]), dict(lens=[1, 2000], skips=[1, 0]),
               dict(lens=[3 * 200 + 1, 2000], skips=[1, 0]),     # L = 200 < pad + 1
               dict(lens=[1000, 50], n_fft=8, hop=8, skips=[0, 0], step=16),   # L = 4 < pad + 1 = 5
               dict(lens=[U64, U64], skips=None, step=1, hop=1, n_mels=128)):             # the total does not fit 64 bits
        assert refused(**kw), kw
    # L >= pad + 1 but below hop: no frame
    assert refused(lens=[6], skips=None, step=1, n_fft=8, hop=8, n_mels=1) is True
    fv.clips_plan_mel([8], None, 1, 8, 8, 1)
    # exactly pad + 1 stream samples pass
    assert int(fv.clips_plan_mel([3 * 200 + 2], [1], 3, 400, 160, 80)[0][0]) == 1


# ------------------------------------------------------------------ the check, rule by rule in its order
def test_check_rules_in_order(fv):
    w, M = mc.hann(400), mc.matrix_for((400, 160, 80))
    clips = np.array([[0, 2, 10, 10 + 3000], [1, 1, 7, 7 + 5000]], np.uint64)
    skips = [mc.phase_skip(10, 3, 2), mc.phase_skip(7, 3, 2)]
    good = dict(d_src=0x10000, src_format=F32, n_lanes=2, lane_stride=6000, n_samples=6000, clips=clips, out=0x20000, out_capacity=1 << 20,
                device_out=True, step=3, skips=skips, n_fft=400, hop=160, window=w, n_mels=80, matrix=M, floor=1e-10, norm=(8, 4, 0.25))
    st, frames, offsets, total = fv.clips_mel_check(**good)
    want = fv.clips_plan_mel([3000, 5000], skips, 3, 400, 160, 80)
    assert st == 0 and frames.tolist() == want[0].tolist() and offsets.tolist() == want[1].tolist() and total == want[2]

    def status(**kw):
        return fv.clips_mel_check(**dict(good, **kw))[0]
    bad_w, bad_m = w.copy(), M.copy()
    bad_w[399], bad_m[79, 200] = np.inf, np.nan
    rules = [  # each entry breaks its own rule and every LATER one's argument stays good; then pairs show the order
        (dict(d_src=0), INVALID), (dict(out=0), INVALID), (dict(window=None), INVALID), (dict(matrix=None), INVALID),
        (dict(src_format=2), INVALID), (dict(out_format=PCM16), INVALID), (dict(out=0x20004), INVALID), (dict(d_src=0x10002), INVALID),
        (dict(lane_stride=5999), INVALID), (dict(clips=[[0, 2, 10, 10], [1, 1, 7, 5007]]), INVALID), (dict(clips=[[0, 0, 10, 3010]], skips=skips[:1]), INVALID),
        (dict(step=0), INVALID), (dict(step=17), INVALID), (dict(hop=401), INVALID),
        (dict(n_fft=399), INVALID), (dict(hop=0), INVALID), (dict(n_mels=0), INVALID), (dict(n_mels=129), INVALID), (dict(skips=[3, 0]), INVALID),
        (dict(clips=[[0, 2, 10, 10 + 600], [1, 1, 7, 5007]]), INVALID), (dict(window=bad_w), INVALID), (dict(matrix=bad_m), INVALID),
        (dict(floor=0.0), INVALID), (dict(floor=-1e-10), INVALID), (dict(floor=float("inf")), INVALID), (dict(floor=float("nan")), INVALID),
        (dict(norm=(8, float("nan"), 0.25)), INVALID), (dict(n_samples=5006), OUT_OF_RANGE), (dict(clips=[[1, 2, 10, 3010], [1, 1, 7, 5007]]), OUT_OF_RANGE),
        (dict(clips=[[2, 1, 10, 3010], [1, 1, 7, 5007]]), OUT_OF_RANGE), (dict(out_capacity=total - 1), TOO_SMALL)]
    for kw, want_st in rules:
        assert status(**kw) == want_st, kw
    assert status(out_capacity=total) == 0 and status(norm=None) == 0 and status(device_out=False, out=0x20004) == 0
    # the order: an earlier rule wins over a later one
    assert status(n_samples=5006, out_capacity=0) == OUT_OF_RANGE and status(floor=0.0, n_samples=5006) == INVALID
    assert status(step=0, out_capacity=0) == INVALID and status(src_format=2, n_samples=1) == INVALID
    # n_clips == 0 asks nothing
    assert fv.clips_mel_check(**dict(good, clips=np.zeros((0, 4), np.uint64), d_src=0, out=0, window=None, matrix=None, skips=None))[0] == 0
    # too many tiles of frames for one grid: a clip of 2^40 samples at hop 1
    huge = dict(good, clips=[[0, 1, 0, 1 << 40]], skips=None, step=1, n_fft=4, hop=1, n_mels=1, window=np.ones(4, np.float32), matrix=np.ones((1, 3), np.float32),
                n_samples=1 << 40, lane_stride=1 << 40, out_capacity=1 << 62)
    assert fv.clips_mel_check(**huge)[0] == INVALID


def test_check_without_the_frame_arrays(fv):
    """n_frames and offsets NULL, as the host-output export calls the rules: the status and the total of the call with them, for
    accepted and refused inputs of test_check_rules_in_order; an accepted input's total is the plan's"""
    w, M = mc.hann(400), mc.matrix_for((400, 160, 80))
    clips = np.array([[0, 2, 10, 10 + 3000], [1, 1, 7, 7 + 5000]], np.uint64)
    skips = [mc.phase_skip(10, 3, 2), mc.phase_skip(7, 3, 2)]
    good = dict(d_src=0x10000, n_lanes=2, lane_stride=6000, n_samples=6000, clips=clips, out=0x20000, out_capacity=1 << 20, device_out=True, step=3,
                skips=skips, n_fft=400, hop=160, window=w, n_mels=80, matrix=M, floor=1e-10, norm=(8, 4, 0.25))
    plan = fv.clips_plan_mel([3000, 5000], skips, 3, 400, 160, 80)[2]

    def raw(null, d_src, n_lanes, lane_stride, n_samples, clips, out, out_capacity, device_out, step, skips, n_fft, hop, window, n_mels, matrix, floor, norm):
        r = np.ascontiguousarray(np.asarray(clips, np.uint64).reshape(-1, 4))
        k = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32))
        keep = [None if a is None else np.ascontiguousarray(np.asarray(a, np.float32)) for a in (window, matrix, norm)]
        frames, offsets, total = np.zeros(len(r), np.uint64), np.zeros(len(r), np.uint64), C.c_uint64(0)

        def ptr(a):
            return None if a is None else fv.fptr(a)
        st = fv.lib().fvad_clips_mel_check(fv.vp(d_src), F32, n_lanes, lane_stride, n_samples, r.ctypes.data_as(C.POINTER(C.c_uint64)), len(r), F32, fv.vp(out),
                                           out_capacity, int(device_out), step, None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint32)), n_fft, hop,
                                           ptr(keep[0]), n_mels, ptr(keep[1]), floor, ptr(keep[2]),
                                           None if null else frames.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           None if null else offsets.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(total))
        return st, int(total.value)
    bad_w = w.copy()
    bad_w[399] = np.inf
    huge = dict(clips=[[0, 1, 0, 1 << 40]], skips=None, step=1, n_fft=4, hop=1, n_mels=1, window=np.ones(4, np.float32), matrix=np.ones((1, 3), np.float32),
                n_samples=1 << 40, lane_stride=1 << 40, out_capacity=1 << 62)
    table = [(dict(), 0), (dict(out_capacity=plan), 0), (dict(norm=None), 0), (dict(device_out=False, out=0x20004), 0),
             (dict(step=0), INVALID), (dict(hop=401), INVALID), (dict(skips=[3, 0]), INVALID), (dict(clips=[[0, 2, 10, 10 + 600], [1, 1, 7, 5007]]), INVALID),
             (dict(window=bad_w), INVALID), (dict(floor=0.0), INVALID), (dict(n_samples=5006), OUT_OF_RANGE), (dict(out_capacity=plan - 1), TOO_SMALL),
             (huge, INVALID)]
    for kw, want in table:
        args = dict(good, **kw)
        with_arrays, without = raw(False, **args), raw(True, **args)
        assert with_arrays[0] == want and without == with_arrays, kw
        assert fv.clips_mel_check(src_format=F32, **args)[::3] == with_arrays, kw
        if want == 0:
            assert without[1] == plan, kw


# ------------------------------------------------------------------ the harness's refusals
def test_what_run_clips_and_main_refuse(pkg, tmp_path):
    out = tmp_path / "never"
    sim = pkg.simulator
    for kw in (dict(features="mfcc"), dict(features="logmel", features_norm="zscore"), dict(features_norm="whisper"),
               dict(features="logmel", slice_chunks=16), dict(features=True)):
        with pytest.raises(ValueError):
            sim.run_clips(str(tmp_path / "no-such-plan.json"), str(out), **kw)   # (neither a plan nor a context is ever opened)
    with pytest.raises(ValueError, match="split-source"):
        sim.run_clips(str(tmp_path / "no-such-plan.json"), str(out), features="logmel", slice_chunks=16)
    plan = str(tmp_path / "no-such-plan.json")
    for argv in (["-i", plan, "--export-clips", str(out), "--clips-features", "mfcc"],
                 ["-i", plan, "--export-clips", str(out), "--clips-features", "logmel", "--clips-features-norm", "zscore"],
                 ["-i", plan, "--export-clips", str(out), "--clips-features-norm", "whisper"],
                 ["-i", plan, "--export-clips", str(out), "--clips-features", "logmel", "--slice-chunks", "16"],
                 ["-i", plan, "--clips-features", "logmel"]):
        with pytest.raises(ValueError):
            sim.main(argv)
    assert not out.exists()
    assert sim.logmel_window().tobytes() == mc.hann(400).tobytes()


# ------------------------------------------------------------------ the yardstick
def test_f32_worst_distance_is_the_committed_literal():
    worst = mc.f32_worst()
    assert round(worst, 4) == mc.F32_WORST, worst
    assert mc.F32_WORST < 10, "a healthy evaluation costs tens of units: the unit is wrong"


def test_silence_is_exact_in_the_model():
    w, M = mc.hann(400), mc.matrix_for((400, 160, 80))
    feat, _ = mc.model(np.zeros(1000, np.float32), w, M, 160)
    assert feat.shape == (6, 80) and (feat == np.log10(np.float64(mc.FLOOR))).all()
    assert np.float32(np.log10(np.float64(mc.FLOOR))) == np.float32(-10.0)


@pytest.fixture(scope="module")
def table():
    t = mc.case_table()
    return t, [c.model() for c in t]


@pytest.mark.parametrize("mutation", ["edge", "late", "phase1", "row", "loud"])
def test_the_table_tells_a_wrong_model(table, mutation):
    cases, refs = table
    worst = 0.0
    for c, (ref, U) in zip(cases, refs):
        got, _ = c.model(mutation)
        T = min(len(got), len(ref))   # (another phase may keep one sample more or less: compare the frames both have)
        worst = max(worst, mc.distance(got[:T], ref[:T], U[:T]))
    assert worst > 50 * mc.TOL, (mutation, worst / mc.TOL)


def test_a_dropped_last_frame_fails_the_count(table):
    cases, refs = table
    for c, (ref, _) in zip(cases, refs):
        assert c.model("lastframe")[0].shape[0] == ref.shape[0] - 1
        with pytest.raises(AssertionError):
            mc.distance(c.model("lastframe")[0], ref, refs[0][1])
