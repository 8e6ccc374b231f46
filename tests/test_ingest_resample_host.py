"""The host side of the resampling ingest (fvad_resample_ratio / _out_frames / _design / _window, fvad_ingest_resample_tile,
fvad_ingest_resample_check; no GPU), and the model of ingest_resample_cases.py against the definition term by term."""
import numpy as np
import pytest

import ingest_resample_cases as rc

OK, INVALID, RANGE = 0, -100, -6
U64_MAX = (1 << 64) - 1


# ---------------------------------------------------------------- ratio, output count, window
def test_the_ratio_table(fv):
    table = {44100: (160, 147), 32000: (3, 2), 22050: (320, 147), 16000: (3, 1), 24000: (2, 1), 8000: (6, 1), 96000: (1, 2),
             11025: (640, 147), 48000: (1, 1)}
    for rate, want in table.items():
        assert fv.resample_ratio(rate) == want, rate
    assert fv.resample_ratio(48000, 44100) == (147, 160)
    up, down = fv.C.c_uint32(7), fv.C.c_uint32(7)
    L = fv.lib()
    assert L.fvad_resample_ratio(44101, 48000, up, down) == INVALID and (up.value, down.value) == (7, 7)   # up would be 48000
    assert L.fvad_resample_ratio(75, 48000, up, down) == OK and (up.value, down.value) == (640, 1)         # the largest up
    assert L.fvad_resample_ratio(74, 48000, up, down) == INVALID
    assert L.fvad_resample_ratio(0, 48000, up, down) == INVALID and L.fvad_resample_ratio(48000, 0, up, down) == INVALID
    assert L.fvad_resample_ratio(44100, 48000, None, down) == INVALID and L.fvad_resample_ratio(44100, 48000, up, None) == INVALID
    assert fv.RESAMPLE_UP_MAX == 640 and fv.RESAMPLE_TAPS_MAX == 2 * 16 * 640 + 1 and fv.RESAMPLE_FIELDS == 11


@pytest.mark.parametrize("up,down,n_taps", [(3, 1, 13), (1, 2, 13), (3, 2, 1), (5, 7, 29), (160, 147, 321), (7, 3, 5), (1, 1, 1), (4, 9, 3)])
def test_out_frames_and_window_against_brute_force(fv, up, down, n_taps):
    K = (n_taps - 1) // 2
    for ff in range(0, 24):
        OF = fv.resample_out_frames(ff, up, down)
        assert OF == rc.out_frames(ff, up, down) == len([o for o in range(10 * ff + 10) if o * down < ff * up])
        # per output: the frames n with a tap index in [0, 2 K], inside the file
        reads = [[n for n in range(ff) if 0 <= K + o * down - n * up <= 2 * K] for o in range(OF)]
        for a in range(OF + 1):
            for n_out in sorted({0, 1, 2, 5, OF - a}):
                if a + n_out > OF:
                    continue
                lo, hi = fv.resample_window(up, down, n_taps, ff, a, n_out)
                assert (lo, hi) == rc.window(up, down, n_taps, ff, a, n_out)
                used = [n for o in range(a, a + n_out) for n in reads[o]]
                if used:
                    assert lo <= min(used) and max(used) < hi <= ff
                    # tight wherever the first and the last output read anything
                    if reads[a]:
                        assert lo == min(reads[a])
                    if reads[a + n_out - 1]:
                        assert hi == max(reads[a + n_out - 1]) + 1
                else:
                    assert lo <= hi <= ff


def test_the_window_is_64_bit(fv):
    # o * down passes 2^32 at o = 29 217 465 of a 44.1 kHz file (10.1 minutes); a window that starts just behind it
    up, down, n_taps = 160, 147, 5121
    o = 29_217_469
    assert (o - 5) * down < 1 << 32 < o * down and (o - 150) * down < 1 << 32
    ff = 100_000_000
    for a, n in ((o, 300), (o - 150, 300), (o * 1000, 7)):
        lo, hi = fv.resample_window(up, down, n_taps, ff * 1000, a, n)
        assert (lo, hi) == rc.window(up, down, n_taps, ff * 1000, a, n)
        assert lo == -(-(a * down - 2560) // up) and hi == ((a + n - 1) * down + 2560) // up + 1
    assert fv.resample_out_frames(1 << 40, 160, 147) == -(-(1 << 40) * 160 // 147)
    assert fv.resample_out_frames(U64_MAX, 640, 1) == U64_MAX                                  # saturated
    assert fv.resample_out_frames(5, 0, 1) == 0 and fv.resample_out_frames(5, 641, 1) == 0 and fv.resample_out_frames(5, 1, 0) == 0
    lo, hi = fv.C.c_uint64(0), fv.C.c_uint64(0)
    L = fv.lib()
    assert L.fvad_resample_window(160, 147, 5120, 10, 0, 1, lo, hi) == INVALID                  # an even count
    assert L.fvad_resample_window(160, 147, 0, 10, 0, 1, lo, hi) == INVALID
    assert L.fvad_resample_window(0, 147, 3, 10, 0, 1, lo, hi) == INVALID and L.fvad_resample_window(160, 0, 3, 10, 0, 1, lo, hi) == INVALID
    assert L.fvad_resample_window(160, 147, 3, 10, U64_MAX, 2, lo, hi) == INVALID               # out_from + n_out wraps
    assert L.fvad_resample_window(160, 147, 3, 10, 0, 1, None, hi) == INVALID


# ---------------------------------------------------------------- the design
@pytest.mark.parametrize("up,down,half,cutoff,beta", [(160, 147, 0, 0.0, 0.0), (3, 1, 0, 0.0, 0.0), (1, 2, 0, 0.0, 0.0), (3, 2, 4, 0.0, 0.0),
                                                       (5, 7, 2, 0.05, 8.5), (640, 147, 0, 0.0, 0.0), (320, 147, 2, 0.0, 3.0)])
def test_the_design_against_numpy(fv, up, down, half, cutoff, beta):
    got = fv.resample_design(up, down, half, cutoff, beta)
    h = half or 16
    want = rc.design(up, down, h, cutoff or None, beta or 6.0)
    assert got.dtype == np.float32 and got.size == 2 * h * max(up, down) + 1 == want.size
    assert np.array_equal(got, want.astype(np.float32))                                      # exact after the rounding to f32
    assert np.array_equal(got, got[::-1])                                                 # symmetric, bit for bit
    assert abs(got.astype(np.float64).sum() - up) < 1e-5 * up                                # sums to up: unit DC gain
    assert got[got.size // 2] == got.max()


def test_the_design_refuses(fv):
    L = fv.lib()
    taps, n = np.zeros(fv.RESAMPLE_TAPS_MAX, np.float32), fv.C.c_uint32(0)
    tp = fv.fptr(taps)
    assert L.fvad_resample_design(640, 147, 16, 0.0, 0.0, tp, n) == OK and n.value == 20481
    assert L.fvad_resample_design(640, 147, 17, 0.0, 0.0, tp, n) == INVALID                   # more than FVAD_RESAMPLE_TAPS_MAX
    assert L.fvad_resample_design(1, 641, 16, 0.0, 0.0, tp, n) == INVALID                     # (m = down counts)
    assert L.fvad_resample_design(0, 1, 1, 0.0, 0.0, tp, n) == INVALID and L.fvad_resample_design(641, 1, 1, 0.0, 0.0, tp, n) == INVALID
    assert L.fvad_resample_design(3, 0, 1, 0.0, 0.0, tp, n) == INVALID
    for cutoff, beta in ((-0.1, 0.0), (0.51, 0.0), (float("nan"), 0.0), (0.0, -1.0), (0.0, float("inf")), (0.0, float("nan")), (0.0, 1e6)):
        assert L.fvad_resample_design(3, 2, 4, cutoff, beta, tp, n) == INVALID, (cutoff, beta)
    assert L.fvad_resample_design(3, 2, 4, 0.0, 0.0, None, n) == INVALID and L.fvad_resample_design(3, 2, 4, 0.0, 0.0, tp, None) == INVALID
    assert L.fvad_resample_design(3, 2, 4, 0.5, 0.0, tp, n) == OK


# ---------------------------------------------------------------- the model against the definition
@pytest.mark.parametrize("up,down,half", rc.CASES[:4] + ((7, 3, 1),))
def test_the_model_is_the_definition(up, down, half):
    rng = np.random.default_rng(up * 100 + down)
    taps = rc.case_taps(up, down, half, "random")
    for ff in (1, 2, 9, 31):
        x = rng.uniform(-1, 1, (ff, 2))
        OF = rc.out_frames(ff, up, down)
        y, B = rc.resample_model(x, taps, up, down, 0, OF)
        for c in range(2):
            want = np.array([rc.brute(x[:, c], taps, up, down, o) for o in range(OF)])
            assert np.allclose(y[c], want, rtol=0, atol=1e-12)
        assert np.all(B >= np.abs(y) - 1e-12)
        # a slice given exactly its window is the file
        a, n = OF // 3, OF - OF // 3 - OF // 4
        lo, hi = rc.window(up, down, taps.size, ff, a, n)
        y2, B2 = rc.resample_model(x[lo:hi], taps, up, down, a, n, frame_base=lo, file_frames=ff)
        assert np.array_equal(y2, y[:, a:a + n]) and np.array_equal(B2, B[:, a:a + n])
        if hi - lo > 1 and n:   # ... and one frame fewer is caught
            with pytest.raises(AssertionError):
                rc.resample_model(x[lo + 1:hi], taps, up, down, a, n, frame_base=lo + 1, file_frames=ff)


def test_identity_and_dc(fv):
    # 1/1 with the single tap 1 is the signal; the default 3/1 design holds a constant to the phases' DC spread
    x = np.random.default_rng(1).uniform(-1, 1, (50, 1))
    y, _ = rc.resample_model(x, [1.0], 1, 1, 0, 50)
    assert np.array_equal(y[0], x[:, 0])
    taps = fv.resample_design(3, 1)
    y, _ = rc.resample_model(np.ones((400, 1)), taps, 3, 1, 0, 1200)
    assert np.all(np.abs(y[0, 100:1100] - 1.0) < 3e-4)
    # zero phase: an impulse at frame 100 of a 16 kHz file peaks at output 300
    x = np.zeros((200, 1))
    x[100] = 1
    y, _ = rc.resample_model(x, taps, 3, 1, 0, 600)
    assert int(np.argmax(y[0])) == 300


# ---------------------------------------------------------------- the tile
def test_the_tile(fv):
    for up, down, half in rc.CASES + ((160, 147, 16), (1, 2, 16), (640, 147, 16)):
        n_taps = 2 * half * max(up, down) + 1
        for C in (1, 2, 3, 64):
            for fmt in (rc.F32, rc.PCM16, rc.PCM24):
                T = fv.ingest_resample_tile(up, down, n_taps, C, fmt)
                fb = C * rc.SAMPLE_BYTES[fmt]
                reach = lambda n: ((n - 1) * down + n_taps - 1) // up + 1
                assert T >= 4 and T % 4 == 0 and T <= 4096 and reach(T) * fb <= 65520, (up, down, C, fmt, T)
                assert T == 4096 or reach(T + 4) * fb > (16384 if reach(64) * fb <= 16384 else 65520)   # the most that fits
                # no window of T outputs is longer than the reach
                for a in (0, 1, 17, 1000, 12345):
                    lo, hi = rc.window(up, down, n_taps, 1 << 40, a, T)
                    assert hi - lo <= reach(T)
    assert fv.ingest_resample_tile(160, 147, 5121, 1, rc.PCM16) == 4096
    assert fv.ingest_resample_tile(1, 1, 20481, 1, rc.PCM16) > 0 and fv.ingest_resample_tile(1, 1, 20481, 64, rc.F32) == 0   # 5 MB of reach
    assert fv.ingest_resample_tile(0, 1, 3, 1, 0) == 0 and fv.ingest_resample_tile(1, 1, 4, 1, 0) == 0
    assert fv.ingest_resample_tile(1, 1, 3, 0, 0) == 0 and fv.ingest_resample_tile(1, 1, 3, 65, 0) == 0 and fv.ingest_resample_tile(1, 1, 3, 1, 3) == 0


# ---------------------------------------------------------------- fvad_ingest_resample_check
# 3/2 with 25 taps (K = 12).  One good source on lanes 2..3 of 6, 100 samples each: a stereo PCM16 file of 40 frames (60
# outputs) whose frames [4, 30) lie at byte 44; outputs [12, 32) -- which read frames [4, 25) -- go to [5, 25), zeros to 30
UP, DOWN, TAPS = 3, 2, np.linspace(0.1, 1.0, 25).astype(np.float32)
GOOD = (44, 26, 2, rc.PCM16, 2, 5, 30, 4, 40, 12, 20)
NAMES = ("byte_offset", "n_frames", "n_channels", "format", "first_lane", "dst_offset", "fill_to", "frame_base", "file_frames", "out_from", "n_out")


def check(fv, sources, raw_bytes=1000, up=UP, down=DOWN, taps=TAPS, n_lanes=6, lane_stride=101, n_samples=100, out_pcm16=False):
    return fv.ingest_resample_check(sources, raw_bytes, up, down, taps, n_lanes, lane_stride, n_samples, out_pcm16)


def edit(**kw):
    return tuple(kw.get(n, v) for n, v in zip(NAMES, GOOD))


def test_check_accepts(fv):
    assert rc.window(UP, DOWN, 25, 40, 12, 20) == (4, 25)
    assert check(fv, [GOOD]) == OK
    assert check(fv, np.zeros((0, 11), np.uint64)) == OK and fv.lib().fvad_ingest_resample_check(None, 0, 0, 1, 1, fv.fptr(TAPS), 25, 0, 0, 0, 0) == OK
    assert check(fv, [edit(n_frames=21)]) == OK                                              # exactly the window
    assert check(fv, [edit(frame_base=0, n_frames=40)]) == OK                                # the whole file
    assert check(fv, [edit(n_out=0, n_frames=0, fill_to=5)]) == OK                           # writes nothing
    assert check(fv, [edit(n_out=0, n_frames=0)]) == OK                                      # only fills
    assert check(fv, [edit(n_out=0, n_frames=0, byte_offset=1000)]) == OK
    assert check(fv, [edit(out_from=40, n_out=20, frame_base=22, n_frames=18)]) == OK        # up to the file's last output
    assert check(fv, [edit(format=rc.PCM24)]) == OK and check(fv, [edit(format=rc.F32)]) == OK
    assert check(fv, [edit(n_channels=64, first_lane=0)], n_lanes=64, raw_bytes=44 + 26 * 128) == OK
    assert check(fv, [edit(byte_offset=1000 - 104)]) == OK and check(fv, [edit(fill_to=100)]) == OK   # both ends exactly
    assert check(fv, [GOOD], raw_bytes=U64_MAX) == OK
    assert check(fv, [edit(file_frames=0, frame_base=0, n_frames=0, out_from=0, n_out=0)]) == OK     # an empty file
    assert check(fv, [GOOD, edit(first_lane=4)]) == OK and check(fv, [GOOD, edit(dst_offset=30, fill_to=50)]) == OK
    assert check(fv, [GOOD], taps=[1.0]) == OK and check(fv, [GOOD], up=640, down=1 << 31, taps=[1.0]) == INVALID   # (60 outputs no more)
    # a phase without taps reads nothing: up 3 with the single tap, an output that is no multiple of 3 needs no frame
    assert check(fv, [edit(out_from=1, n_out=1, n_frames=0, frame_base=40)], up=3, down=1, taps=[1.0]) == OK


def test_check_invalid_arguments_in_order(fv):
    L, u64p = fv.lib(), fv.C.POINTER(fv.C.c_uint64)
    one = np.array([GOOD], np.uint64)
    rows, tp = one.ctypes.data_as(u64p), fv.fptr(TAPS)
    # the call's own arguments, in the documented order: each rule with everything behind it broken as well
    bad_row = np.array([edit(format=9, first_lane=99)], np.uint64).ctypes.data_as(u64p)
    assert L.fvad_ingest_resample_check(rows, 1, 1000, UP, DOWN, tp, 25, 1, 6, 101, 100) == INVALID        # PCM16 lanes: a conversion
    assert L.fvad_ingest_resample_check(rows, 1, 1000, UP, DOWN, tp, 25, 2, 6, 101, 100) == INVALID
    assert L.fvad_ingest_resample_check(None, 0, 0, UP, DOWN, tp, 25, 1, 0, 0, 0) == INVALID               # ... before "no sources"
    assert check(fv, [GOOD], out_pcm16=True) == INVALID
    for up, down in ((0, 2), (641, 2), (3, 0)):
        assert check(fv, [GOOD], up=up, down=down) == INVALID and check(fv, np.zeros((0, 11), np.uint64), up=up, down=down) == INVALID
    assert check(fv, [GOOD], taps=None) == INVALID and check(fv, np.zeros((0, 11), np.uint64), taps=None) == INVALID
    assert check(fv, [GOOD], taps=TAPS[:24]) == INVALID                                      # an even count
    assert check(fv, [GOOD], taps=np.zeros(20483, np.float32)) == INVALID
    for v in (np.nan, np.inf, -np.inf):
        t = TAPS.copy()
        t[7] = v
        assert check(fv, [GOOD], taps=t) == INVALID
    assert L.fvad_ingest_resample_check(None, 1, 1000, UP, DOWN, tp, 25, 0, 6, 101, 100) == INVALID        # NULL sources
    assert check(fv, [GOOD], lane_stride=99) == INVALID
    assert L.fvad_ingest_resample_check(bad_row, 1, 1000, UP, DOWN, tp, 25, 0, 6, 101, 100) == INVALID     # INVALID before RANGE
    # per source
    assert check(fv, [edit(format=3)]) == INVALID
    assert check(fv, [edit(n_channels=0)]) == INVALID and check(fv, [edit(n_channels=65, first_lane=0)], n_lanes=100) == INVALID
    assert check(fv, [edit(file_frames=(1 << 62) // 3 + 1)]) == INVALID                      # file_frames * up >= 2^62
    assert check(fv, [edit(file_frames=(1 << 62) // 3)]) == OK
    assert check(fv, [edit(out_from=41, frame_base=22, n_frames=18)]) == INVALID             # one output past the file's 60
    assert check(fv, [edit(out_from=U64_MAX, n_out=2)]) == INVALID                           # out_from + n_out wraps
    assert check(fv, [edit(fill_to=24)]) == INVALID                                          # below dst_offset + n_out
    assert check(fv, [edit(dst_offset=U64_MAX, fill_to=U64_MAX)]) == INVALID                 # dst_offset + n_out wraps
    assert check(fv, [edit(frame_base=20, n_frames=21)]) == INVALID                          # given frames past the file's end
    assert check(fv, [edit(frame_base=U64_MAX)]) == INVALID                                  # frame_base + n_frames wraps
    assert check(fv, [edit(frame_base=5, n_frames=25)]) == INVALID                           # the window's first frame is missing
    assert check(fv, [edit(n_frames=20)]) == INVALID                                         # ... its last
    assert check(fv, [edit(n_frames=0)]) == INVALID
    assert check(fv, [GOOD, edit(first_lane=4, n_frames=20)]) == INVALID                     # in any row
    assert check(fv, [edit(n_channels=64, first_lane=0, format=rc.F32)], n_lanes=64, raw_bytes=1 << 20, up=1, down=1,
                 taps=np.ones(20481, np.float32)) == INVALID                                 # no tile: the reach is 5 MB
    # the given-frames rule before the ranges: a short slice on lanes that do not exist is INVALID, not RANGE
    assert check(fv, [edit(n_frames=20, first_lane=6)]) == INVALID


def test_check_out_of_range_and_overlap(fv):
    assert check(fv, [edit(first_lane=6)]) == RANGE and check(fv, [edit(first_lane=5)]) == RANGE
    assert check(fv, [edit(first_lane=U64_MAX)]) == RANGE
    assert check(fv, [edit(fill_to=101)]) == RANGE
    assert check(fv, [edit(byte_offset=1000 - 103)]) == RANGE                                # one byte past the raw buffer
    assert check(fv, [edit(byte_offset=1001, n_out=0, n_frames=0, fill_to=5)]) == RANGE
    assert check(fv, [edit(byte_offset=U64_MAX)], raw_bytes=U64_MAX) == RANGE
    assert check(fv, [edit(format=rc.PCM24, byte_offset=1000 - 155)]) == RANGE               # 156 bytes of PCM24
    big = (1 << 62) // 3
    assert check(fv, [edit(frame_base=0, n_frames=big, file_frames=big, n_channels=64, first_lane=0)], n_lanes=64, raw_bytes=U64_MAX) == RANGE   # frames * frame bytes wraps
    assert check(fv, [edit(first_lane=6), edit(fill_to=24)]) == INVALID                      # a later row's own rule before an earlier row's range
    assert check(fv, [GOOD, GOOD]) == INVALID
    assert check(fv, [GOOD, edit(dst_offset=29, fill_to=50)]) == INVALID and check(fv, [edit(dst_offset=29, fill_to=50), GOOD]) == INVALID
    assert check(fv, [GOOD, edit(first_lane=3, n_channels=1)]) == INVALID
    assert check(fv, [GOOD, edit(n_out=0, n_frames=0, dst_offset=10, fill_to=11)]) == INVALID
    assert check(fv, [GOOD, edit(n_out=0, n_frames=0, dst_offset=10, fill_to=10)]) == OK


def test_the_case_tables_pass_the_check_and_bite(fv):
    for up, down, half in rc.CASES:
        taps = rc.case_taps(up, down, half, "design")
        t = rc.case_table(up, down, taps.size, lambda C, fmt: fv.ingest_resample_tile(up, down, taps.size, C, fmt))
        rows = t["rows"].astype(np.int64)
        assert fv.ingest_resample_check(t["rows"], t["raw"].size, up, down, taps, t["n_lanes"], t["lane_stride"], t["n_samples"]) == OK
        assert set(rows[:, 2].tolist()) == {1, 2, 3, 64} and set(rows[:, 3].tolist()) == {0, 1, 2}
        assert {0, 1, 2} <= set(rows[:, 8].tolist())                                         # files of 0, 1 and 2 frames
        for fmt in (0, 1, 2):
            assert {int(b) % 2 for b in rows[rows[:, 3] == fmt, 0]} == {0, 1}                # odd and even byte offsets
        assert {int(d) % 4 for d in rows[:, 5]} == {0, 1, 2, 3} and {0, 1, 7, 9} <= set((rows[:, 6] - rows[:, 5] - rows[:, 10]).tolist())
        for fmt, C in rc.COMBOS:
            T = fv.ingest_resample_tile(up, down, taps.size, C, fmt)
            sel = rows[(rows[:, 3] == fmt) & (rows[:, 2] == C)]
            assert {T - 1, T, T + 1, 2 * T + 1} <= set(sel[:, 10].tolist())
            OF = rc.out_frames(int(sel[0, 8]), up, down)
            assert np.any(sel[:, 9] + sel[:, 10] == OF) and np.any((sel[:, 9] == 0))          # the file's first and last outputs
        assert t["n_lanes"] * t["lane_stride"] < 4_000_000
        tw = rc.twin_f32(t)
        assert fv.ingest_resample_check(tw["rows"], tw["raw"].size, up, down, taps, t["n_lanes"], t["lane_stride"], t["n_samples"]) == OK
        # slices that give exactly their windows pass; one frame fewer does not
        row = t["rows"][3]
        cuts = sorted(int(row[9]) + c for c in (int(row[10]) // 3, int(row[10]) // 3 + 1, int(row[10]) - 2))
        sl = rc.slices(row, cuts, up, down, taps.size)
        assert len(sl) == 4 and fv.ingest_resample_check(sl, t["raw"].size, up, down, taps, t["n_lanes"], t["lane_stride"], t["n_samples"]) == OK
        short = list(sl[1])
        short[1] -= 1
        assert fv.ingest_resample_check([tuple(short)], t["raw"].size, up, down, taps, t["n_lanes"], t["lane_stride"], t["n_samples"]) == INVALID


def test_a_wrong_walk_fails_compare():
    # the bound is tight enough to tell a reversed prototype, a shifted output and an f32 sum with one term dropped apart
    up, down, half = 3, 2, 4
    taps = rc.case_taps(up, down, half, "random")
    x = np.random.default_rng(2).uniform(-1, 1, (200, 1))
    y, B = rc.resample_model(x, taps, up, down, 0, 300)
    rc.compare(y.astype(np.float32), y, B, up, taps.size, "the model itself")
    for wrong in (rc.resample_model(x, taps[::-1], up, down, 0, 300)[0], np.roll(y, 1, axis=1), y + 1e-6 * B):
        with pytest.raises(AssertionError):
            rc.compare(wrong.astype(np.float32), y, B, up, taps.size)


# ---------------------------------------------------------------- the rules fvad_ingest_check and this check share
def _shared_rule_tables(seed, n_tables):
    """seeded random calls -> (sources [n][7], raw_bytes, n_lanes, lane_stride, n_samples): mostly valid layouts (sources on
    lanes of their own, inside the samples and the bytes), each field now and then replaced by a value one of the shared rules
    refuses or that sits near a wrap"""
    rng = np.random.default_rng(seed)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    near_max = lambda: U64_MAX - int(rng.integers(0, 51))
    for _ in range(n_tables):
        n_sources = int(rng.integers(1, 4))
        n_samples = int(rng.integers(8, 200))
        n_lanes = int(rng.integers(1, 10))
        lane_stride = n_samples - 1 if rng.random() < 0.04 else n_samples + int(rng.integers(0, 3))
        raw_bytes = U64_MAX if rng.random() < 0.1 else int(rng.integers(0, 4000))
        rows, lane, at = [], 0, 0
        for _ in range(n_sources):
            ch = int(rng.integers(1, 4))
            fmt = int(rng.integers(0, 3))
            dst = int(rng.integers(0, n_samples))
            n = int(rng.integers(0, n_samples - dst + 1))
            fill = int(rng.integers(0, n_samples - dst - n + 1))
            first_lane = lane if rng.random() < 0.8 else int(rng.integers(0, n_lanes))   # (the others may overlap a neighbour)
            lane += ch
            byte_offset = at + int(rng.integers(0, 5))
            at = byte_offset + n * ch * rc.SAMPLE_BYTES[fmt]
            fill_to = dst + n + fill
            if rng.random() < 0.05:
                ch = pick((0, 65, 64))
            if rng.random() < 0.04:
                fmt = 3
            if rng.random() < 0.05:
                n = pick((1 << 61, int(rng.integers(1 << 32, 1 << 61)), (1 << 61) - 1))
            if rng.random() < 0.05:
                fill_to = (dst + n - 1) % (1 << 64)                       # short by one (n == 0 at 0: wraps)
            if rng.random() < 0.05:
                first_lane = pick((n_lanes, n_lanes + 1, U64_MAX, max(n_lanes - ch + 1, 0)))
            if rng.random() < 0.04:
                dst, fill_to = near_max(), near_max()
            if rng.random() < 0.04:
                byte_offset = near_max()
            if rng.random() < 0.04:
                fill_to = n_samples + 1
            rows.append((byte_offset, n, ch, fmt, first_lane, dst, fill_to))
        if rng.random() < 0.5:
            raw_bytes = max(raw_bytes, at) - (1 if rng.random() < 0.1 else 0)
        yield np.array(rows, np.uint64), raw_bytes, n_lanes, lane_stride, n_samples


def test_the_shared_rules_give_both_checks_one_status(fv):
    # up = down = 1 with the single tap 1.0, a whole-file row (frame_base 0, file_frames = n_out = n_frames, out_from 0): every
    # rule of the resample check that fvad_ingest_check does not have passes (n_frames <= 2^61 keeps file_frames * up below
    # 2^62), so the two checks see the same arguments, rules and order -- and must answer alike, table by table
    seen = {OK: 0, INVALID: 0, RANGE: 0}
    one = np.ones(1, np.float32)
    for sources, raw_bytes, n_lanes, lane_stride, n_samples in _shared_rule_tables(20261021, 4000):
        n = sources[:, 1:2]
        rrows = np.concatenate([sources, np.zeros_like(n), n, np.zeros_like(n), n], axis=1)
        plain = fv.ingest_check(sources, raw_bytes, False, n_lanes, lane_stride, n_samples)
        resampled = fv.ingest_resample_check(rrows, raw_bytes, 1, 1, one, n_lanes, lane_stride, n_samples)
        assert plain == resampled, (sources.tolist(), raw_bytes, n_lanes, lane_stride, n_samples, plain, resampled)
        seen[plain] += 1
    assert min(seen.values()) >= 20, seen
