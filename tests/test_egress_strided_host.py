"""The host side of the strided resampling egress (fvad_egress_resample_strided_check; no GPU) against a python-integer
restatement, the case tables of egress_strided_cases.py, the harness's filter rule per rate (run_denoise(source="network")), and
two facts in float64 numpy: what the lerped 48 kHz lanes do to a network tone, and what the lagged 3/1 design does instead."""
import numpy as np
import pytest

import egress_resample_cases as er
import egress_strided_cases as es
import ingest_resample_cases as rc

OK, INVALID, RANGE = es.OK, es.INVALID, es.RANGE
U64_MAX = (1 << 64) - 1


def test_the_exports_exist(fv):
    for name in ("fvad_egress_resample_strided_check", "fvad_egress_resample_strided_device", "fvad_egress_resample_strided"):
        assert name in fv.SIGNATURES and getattr(fv.lib(), name)
    assert fv.EGRESS_STEP_MAX == es.STEP_MAX == 16
    assert callable(fv.egress_resample_strided_check) and callable(fv.Context.egress_resample_strided)
    assert fv.lib().fvad_abi_version() == 3   # new entry points only


# ---------------------------------------------------------------- fvad_egress_resample_strided_check
# test_egress_resample_host.py's good row, 3 apart: 2/3 with 25 taps; a stereo PCM16 file of a stream of 60 strided samples;
# outputs [12, 32) read stream samples [12, 53); the lanes hold stream samples [10, 55) from lane sample 5 on, the last at
# 5 + 44 * 3 = 137 of 138
UP, DOWN, TAPS, STEP = 2, 3, np.linspace(0.1, 1.0, 25).astype(np.float32), 3
GOOD = (44, 20, 2, er.PCM16, 2, 5, 10, 45, 60, 12)
NAMES = ("byte_offset", "n_out", "n_channels", "format", "first_lane", "src_offset", "frame_base", "n_frames", "stream_frames", "out_from")
GEOM = dict(out_bytes=1000, up=UP, down=DOWN, taps=TAPS, step=STEP, src_format=0, n_lanes=6, lane_stride=139, n_samples=138)


def both(fv, rows, **kw):
    """the library's status, held against the restatement's"""
    g = dict(GEOM, **kw)
    rows = [tuple(int(v) for v in r) for r in rows]
    got = fv.egress_resample_strided_check(np.asarray(rows, np.uint64).reshape(-1, 10), g["out_bytes"], g["up"], g["down"], g["taps"], g["step"],
                                           g["n_lanes"], g["lane_stride"], g["n_samples"], src_pcm16=g["src_format"] == 1)
    want = es.check_model(rows, g["out_bytes"], g["up"], g["down"], g["taps"], g["step"], g["src_format"], g["n_lanes"], g["lane_stride"], g["n_samples"])
    assert got == want, (rows, kw, got, want)
    return got


def edit(**kw):
    return tuple(kw.get(n, v) for n, v in zip(NAMES, GOOD))


def test_check_accepts_and_the_step_rules(fv):
    assert both(fv, [GOOD]) == OK
    assert both(fv, []) == OK
    for step in range(1, 17):
        assert both(fv, [GOOD], step=step, n_samples=5 + 44 * step + 1, lane_stride=5 + 44 * step + 2) == OK
    # the step's rule: directly behind the ratio's, in front of the taps' and of "no sinks"
    for step in (0, 17, 1 << 31, (1 << 32) - 1):
        assert both(fv, [GOOD], step=step) == INVALID and both(fv, [], step=step) == INVALID
    assert both(fv, [], step=0, taps=None) == INVALID and both(fv, [], step=3, taps=None) == INVALID
    L, u64p = fv.lib(), fv.C.POINTER(fv.C.c_uint64)
    one = np.array([GOOD], np.uint64)
    assert L.fvad_egress_resample_strided_check(one.ctypes.data_as(u64p), 1, 1000, UP, DOWN, fv.fptr(TAPS), 25, 3, 0, 6, 139, 138) == OK
    assert L.fvad_egress_resample_strided_check(one.ctypes.data_as(u64p), 1, 1000, UP, DOWN, fv.fptr(TAPS), 25, 3, 1, 6, 139, 138) == INVALID   # PCM16 lanes
    assert L.fvad_egress_resample_strided_check(None, 1, 1000, UP, DOWN, fv.fptr(TAPS), 25, 3, 0, 6, 139, 138) == INVALID
    assert L.fvad_egress_resample_strided_check(None, 0, 0, UP, DOWN, fv.fptr(TAPS), 25, 17, 0, 0, 0, 0) == INVALID


def test_the_strided_range_rule_at_its_boundary(fv):
    # the last strided sample at n_samples - 1 is accepted, at n_samples refused
    assert both(fv, [GOOD], n_samples=138) == OK and both(fv, [GOOD], n_samples=137, lane_stride=139) == RANGE
    assert both(fv, [edit(src_offset=6)]) == RANGE and both(fv, [edit(src_offset=5)]) == OK
    for step in (1, 2, 16):
        last = 5 + 44 * step
        assert both(fv, [GOOD], step=step, n_samples=last + 1, lane_stride=last + 1) == OK
        assert both(fv, [GOOD], step=step, n_samples=last, lane_stride=last + 1) == RANGE
    # no frames touch no sample, wherever src_offset points
    assert both(fv, [edit(n_out=0, n_frames=0, src_offset=U64_MAX)]) == OK
    # one frame: the sample itself
    one = edit(out_from=0, n_out=1, frame_base=0, n_frames=1, stream_frames=1)
    at = lambda src: tuple(src if n == "src_offset" else v for n, v in zip(NAMES, one))
    assert both(fv, [at(137)], taps=[1.0], up=1, down=1) == OK and both(fv, [at(138)], taps=[1.0], up=1, down=1) == RANGE
    # near 2^64: nothing wraps
    assert both(fv, [edit(src_offset=U64_MAX)]) == RANGE and both(fv, [edit(src_offset=U64_MAX - 44 * 3)]) == RANGE
    assert both(fv, [edit(src_offset=U64_MAX - 44 * 3 + 1)]) == RANGE                            # (n_frames - 1) step + src_offset wraps to 0
    big = (1 << 62) // 2 - 1                                                                  # stream_frames * up < 2^62
    row = edit(stream_frames=big, frame_base=0, n_frames=big, out_from=0, n_out=4, src_offset=7, n_channels=1)
    assert both(fv, [row], step=16, n_samples=U64_MAX, lane_stride=U64_MAX, n_lanes=3) == RANGE   # (big - 1) * 16 passes 2^64
    assert both(fv, [row], step=3, n_samples=U64_MAX, lane_stride=U64_MAX, n_lanes=3) == OK
    assert both(fv, [row], step=3, n_samples=7 + (big - 1) * 3, lane_stride=U64_MAX, n_lanes=3) == RANGE
    assert both(fv, [row], step=3, n_samples=7 + (big - 1) * 3 + 1, lane_stride=U64_MAX, n_lanes=3) == OK


def test_check_against_the_restatement_over_seeded_tables(fv):
    rng = np.random.default_rng(77)
    pick = lambda values: values[int(rng.integers(len(values)))]   # (python integers: no float on the way)
    near = lambda: pick([0, 1, 2, U64_MAX, U64_MAX - 1, 1 << 63, (1 << 62) - 1, (1 << 62) // 2, 1 << 32])
    seen = {OK: 0, INVALID: 0, RANGE: 0}
    for k in range(600):
        step = int(rng.choice([0, 1, 2, 3, 3, 3, 7, 16, 17]))
        n_samples = 5 + 44 * max(step, 1) + int(rng.integers(0, 3))
        rows = []
        for i in range(int(rng.integers(1, 4))):
            r = list(edit(byte_offset=44 + 100 * i))
            for _ in range(int(rng.integers(0, 3))):
                col = int(rng.integers(0, 10))
                r[col] = near() if rng.random() < 0.4 else min(U64_MAX, max(0, r[col] + int(rng.integers(-2, 3))))
            rows.append(tuple(r))
        up, down = (UP, DOWN) if rng.random() < 0.9 else (int(rng.choice([0, 1, 641])), int(rng.choice([0, 1, 3])))
        seen[both(fv, rows, step=step, up=up, down=down, n_samples=n_samples, lane_stride=n_samples + int(rng.integers(-1, 2)),
                  out_bytes=pick([1000, 400, U64_MAX]))] += 1
    assert min(seen.values()) >= 20, seen


def test_what_fvad_egress_resample_check_refuses_is_refused(fv):
    # the parent's rules and their order are kept: its own tables of bad rows give the same status with step 1
    assert both(fv, [GOOD], src_format=1) == INVALID
    assert both(fv, [GOOD], taps=TAPS[:24]) == INVALID and both(fv, [GOOD], taps=np.zeros(20483, np.float32)) == INVALID
    t = TAPS.copy()
    t[7] = np.nan
    assert both(fv, [GOOD], taps=t) == INVALID
    assert both(fv, [GOOD], lane_stride=137) == INVALID
    assert both(fv, [edit(format=3)]) == INVALID and both(fv, [edit(n_channels=0)]) == INVALID and both(fv, [edit(n_channels=65, first_lane=0)], n_lanes=100) == INVALID
    assert both(fv, [edit(stream_frames=(1 << 62) // 2)]) == INVALID
    assert both(fv, [edit(out_from=21, frame_base=24, n_frames=36)]) == INVALID and both(fv, [edit(out_from=U64_MAX, n_out=2)]) == INVALID
    assert both(fv, [edit(frame_base=16, n_frames=45)]) == INVALID and both(fv, [edit(frame_base=U64_MAX)]) == INVALID
    assert both(fv, [edit(frame_base=13, n_frames=42)]) == INVALID and both(fv, [edit(n_frames=42)]) == INVALID
    assert both(fv, [edit(n_frames=42, first_lane=6)]) == INVALID                              # the given-frames rule before the ranges
    assert both(fv, [edit(first_lane=6)]) == RANGE and both(fv, [edit(first_lane=U64_MAX)]) == RANGE
    assert both(fv, [edit(byte_offset=1000 - 79)]) == RANGE and both(fv, [edit(byte_offset=U64_MAX)], out_bytes=U64_MAX) == RANGE
    assert both(fv, [GOOD, GOOD]) == INVALID and both(fv, [GOOD, edit(byte_offset=124)]) == OK
    assert both(fv, [GOOD, GOOD, edit(first_lane=6)]) == RANGE                                  # a range before the overlap
    for rows in ([GOOD], [edit(n_frames=42)], [edit(first_lane=6)], [GOOD, GOOD], [edit(src_offset=94)], [edit(src_offset=95)]):
        same = fv.egress_resample_check(rows, 1000, UP, DOWN, TAPS, 6, 139, 138)
        assert both(fv, rows, step=1) == same, rows


# ---------------------------------------------------------------- the case tables
@pytest.fixture(scope="module", params=es.CASES, ids=es.case_id)
def table(request, fv):
    up, down, _, step = request.param
    taps = es.case_taps(request.param)
    base = er.case_table(up, down, taps.size)
    return up, down, step, taps, base, es.strided(base, step, seed=step), fv


def test_the_case_tables(table):
    up, down, step, taps, base, t, fv = table
    assert taps.size == {(3, 1): 101, (1, 1): 1, (441, 160): 14701, (7, 5): 29, (2, 1): 13, (147, 160): 5121}[(up, down)]
    assert (-(-taps.size // up) * up > 6144) == ((up, down) == (441, 160))                       # the one table in global memory
    c = es.compacted(t)
    for tb, st in ((t, step), (er.twin_f32(t), step), (c, 1)):
        assert fv.egress_resample_strided_check(tb["rows"], tb["out_bytes"], up, down, taps, st, tb["n_lanes"], tb["lane_stride"], tb["n_samples"]) == OK
    assert fv.egress_resample_check(c["rows"], c["out_bytes"], up, down, taps, c["n_lanes"], c["lane_stride"], c["n_samples"]) == OK
    rows = t["rows"].astype(np.int64)
    assert np.array_equal(np.delete(t["rows"], 5, 1), np.delete(base["rows"], 5, 1)) and t["data"] is base["data"]   # the same rows, the same model
    assert {int(v) % 4 for v in rows[:, 5]} == {0, 1, 2, 3} and t["lane_stride"] % 2 == 1 and c["lane_stride"] % 2 == 1
    assert {0, 1, 5} <= set(rows[:, 8].tolist()) and len(t["big"]) == 6 and set(rows[:, 2].tolist()) == {1, 2, 3, 64}
    # finite on the stride, NaN everywhere else: between two strided samples too
    mask = np.ones(t["lanes"].shape, bool)
    for (_, _, C, _, l0, src, _, nf, _, _), v in zip(rows.tolist(), t["data"]):
        if nf:
            sl = (slice(l0, l0 + C), slice(src, src + (nf - 1) * step + 1, step))
            assert np.array_equal(t["lanes"][sl], v.T.astype(np.float32))
            mask[sl] = False
    assert np.isnan(t["lanes"][mask]).all()
    if step > 1:
        i = t["big"][0]
        src, nf = int(rows[i, 5]), int(rows[i, 7])
        assert np.isnan(t["lanes"][int(rows[i, 4]), src + 1:src + step]).all() and np.isnan(t["lanes"][int(rows[i, 4]), src + (nf - 1) * step - 1])
    # the compacted lanes hold the same samples
    for (_, _, C, _, l0, src, _, nf, _, _), v in zip(c["rows"].tolist(), c["data"]):
        assert np.array_equal(c["lanes"][l0:l0 + C, src:src + nf], v.T.astype(np.float32))
    # one sample short of the last strided one does not pass
    assert fv.egress_resample_strided_check(t["rows"], t["out_bytes"], up, down, taps, step, t["n_lanes"], t["lane_stride"],
                                            int((rows[:, 5] + np.maximum(rows[:, 7] - 1, 0) * step).max())) == RANGE


# ---------------------------------------------------------------- the harness's filter per rate
def test_the_harness_filter_per_rate(pkg):
    sim, fv = pkg.simulator, pkg.binding
    assert (sim.NETWORK_STEP, sim.NETWORK_PHASE, sim.NETWORK_RATE) == (3, 2, 16000)
    want = {48000: (3, 1, 2, 0, 101), 44100: (441, 160, 294, 0, 14701), 22050: (441, 320, 294, 0, 14113 + 588), 24000: (3, 2, 2, 0, 101),
            96000: (6, 1, 4, 0, 201), 32000: (2, 1, 0, 2, 65), 8000: (1, 2, 0, 2, 65), 16000: (1, 1, 0, 2, 1)}
    for rate, (up, down, lag, lead, n_taps) in want.items():
        f = sim._network_resample(rate)
        assert (f["up"], f["down"], f["lag"], f["lead"], f["taps"].size) == (up, down, lag, lead, n_taps), rate
        assert f == {**f, "rate": rate, "source": "network", "step": 3, "phase": 2}
        assert es.network_filter(rate) == dict(up=up, down=down, lag=lag, lead=lead, n_taps=n_taps)
        assert (up, down) == fv.resample_ratio(16000, rate) and (up % 3 == 0) == (lead == 0) and lag == (2 * up // 3 if up % 3 == 0 else 0)
        assert f["taps"].dtype == np.float32 and fv.egress_resample_tile(up, down, n_taps, 2, er.PCM16) > 0
        if rate == 16000:
            assert f["taps"].tolist() == [1.0] and f["half"] is None
        else:
            d = fv.resample_design(up, down)
            assert np.array_equal(f["taps"][2 * lag:], d) and not f["taps"][:2 * lag].any() and f["half"] == 16 and f["cutoff"] == 0.45 / max(up, down)
    for rate in (11025, 44101, 0, -16000, True, "48000", 1 << 32):
        with pytest.raises(ValueError):
            sim._network_resample(rate)
    assert es.network_filter(11025) is None and es.network_filter(44101) is None
    assert fv.resample_design(441, 640).size + 588 == 20481 + 588 > fv.RESAMPLE_TAPS_MAX      # 11025: the lagged design is too long
    # the file's frames are the lanes path's at the same rate
    for rate, (up, down, *_) in want.items():
        for n in (0, 1, 9, 37):
            assert fv.resample_out_frames(n * 8000, up, down) == fv.resample_out_frames(n * 24000, *fv.resample_ratio(48000, rate))


def test_the_refusals_need_no_device(pkg, tmp_path):
    sim = pkg.simulator
    out = tmp_path / "out"
    for kw in (dict(source="nets"), dict(source=None), dict(source="network", kinds=("denoised", "residual")), dict(source="network", kinds=("original",)),
               dict(source="network", rate=11025), dict(source="network", rate=44101), dict(source="network", rate=0)):
        with pytest.raises(ValueError):
            sim.run_denoise(str(tmp_path / "no-such-plan.json"), str(out), **kw)
    assert not out.exists()
    with pytest.raises(ValueError, match="--denoised-source needs --export-denoised"):
        sim.check_modes(sim.arg_parser().parse_args(["-i", "p.json", "--denoised-source", "network"]))
    sim.check_modes(sim.arg_parser().parse_args(["-i", "p.json", "--export-denoised", str(out), "--denoised-source", "network"]))


# ---------------------------------------------------------------- two facts in float64
A, F_TONE, N_NET = 0.5, 6000.0, 1600   # 1600 network samples = 4800 lane samples = 0.1 s: whole periods of 6, 10 and 22 kHz


def _network_tone():
    j = np.arange(N_NET)
    return A * np.sin(2 * np.pi * F_TONE * (3 * j + 2) / 48000)   # sample j is the tone at lane time 3 j + 2


def _level_db(x, f):
    """the amplitude of the component at f Hz of x (48 kHz, whole periods) against A, in dB"""
    t = np.arange(x.size)
    return 20 * np.log10(2 * abs(np.sum(x * np.exp(-2j * np.pi * f * t / 48000))) / x.size / A)


def test_the_lerped_lanes_droop_and_image():
    # the defect, pinned as a fact: K3's lanes are [lerp, lerp, sample] per network sample (periodic here: whole periods)
    x = _network_tone()
    prev = np.roll(x, 1)
    lanes = np.empty(3 * N_NET)
    lanes[2::3], lanes[0::3], lanes[1::3] = x, prev + (x - prev) / 3, prev + (x - prev) * 2 / 3
    assert abs(_level_db(lanes, 6000) - (-3.8)) < 0.05
    assert abs(_level_db(lanes, 10000) - (-11.8)) < 0.1
    assert abs(_level_db(lanes, 22000) - (-20.3)) < 0.1


def test_the_lagged_design_puts_the_tone_at_lane_time(fv):
    # the library's default 3/1 taps lagged by 2: output o is the tone at lane time o, within the design's pass-band ripple
    # (0.11 dB) and twice its stop band (-69.8 dB: the images at 10 and 22 kHz) -- include/fvad.h's figures
    taps = es.lagged(fv.resample_design(3, 1), 2).astype(np.float64)
    assert taps.size == 101
    x = _network_tone()
    y, _ = rc.resample_model(x[:, None], taps, 3, 1, 0, 3 * N_NET)
    want = A * np.sin(2 * np.pi * F_TONE * np.arange(3 * N_NET) / 48000)
    tol = A * (10 ** (0.11 / 20) - 1) + 2 * A * 10 ** (-69.8 / 20)
    edge = 3 * 40   # the filter's reach at both ends
    err = np.abs(y[0] - want)[edge:-edge].max()
    print("lagged 3/1 design, 6 kHz network tone: max error", err, "tolerance", tol)
    assert err <= tol
    # without the lag the file would be two lane samples early: the error is the tone's slope, far past the tolerance
    y0, _ = rc.resample_model(x[:, None], fv.resample_design(3, 1).astype(np.float64), 3, 1, 0, 3 * N_NET)
    assert np.abs(y0[0] - want)[edge:-edge].max() > 50 * tol
