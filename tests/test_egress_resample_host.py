"""The host side of the resampling egress (fvad_egress_resample_tile / _ready / _check; no GPU), the model of
egress_resample_cases.py against the definition term by term, and the case tables against deliberately wrong models."""
import numpy as np
import pytest

import egress_resample_cases as er
import ingest_resample_cases as rc

OK, INVALID, RANGE = 0, -100, -6
U64_MAX = (1 << 64) - 1


def test_the_exports_exist(fv):
    for name in ("fvad_egress_resample_tile", "fvad_egress_resample_ready", "fvad_egress_resample_check", "fvad_egress_resample_device",
                 "fvad_egress_resample"):
        assert name in fv.SIGNATURES and getattr(fv.lib(), name)
    assert fv.EGRESS_RESAMPLE_FIELDS == er.FIELDS == 10
    assert callable(fv.egress_resample_tile) and callable(fv.egress_resample_ready) and callable(fv.egress_resample_check)
    assert callable(fv.Context.egress_resample)
    assert fv.lib().fvad_abi_version() == 3   # new entry points only


# ---------------------------------------------------------------- the tile and the ready count
def test_the_tile(fv):
    for up, down, half, _ in er.RATIOS + ((147, 640, 16, ""), (640, 1, 16, ""), (1, 1, 16, ""), (3, 1000, 1, "")):
        n_taps = 2 * half * max(up, down) + 1
        if n_taps > fv.RESAMPLE_TAPS_MAX:
            continue
        reach = lambda n: ((n - 1) * down + n_taps - 1) // up + 1
        for C in (1, 2, 3, 5, 64):
            for fmt in (er.F32, er.PCM16, er.PCM24):
                T = fv.egress_resample_tile(up, down, n_taps, C, fmt)
                assert T == er.tile(up, down, n_taps, C, fmt), (up, down, C, fmt)
                most = er.TILE_BYTES // (C * er.SAMPLE_BYTES[fmt]) // 4 * 4
                assert T % 4 == 0 and T <= most
                if T:
                    assert reach(T) <= er.WINDOW and T * C * er.SAMPLE_BYTES[fmt] <= er.TILE_BYTES
                    assert (T - 1) * down + n_taps - 1 < 1 << 23          # the kernel's 32-bit induction
                    assert T == most or reach(T + 4) > er.WINDOW           # the most that fits
                    for a in (0, 1, 17, 12345, (1 << 40) + 3):
                        lo, hi = rc.window(up, down, n_taps, 1 << 50, a, T)
                        assert hi - lo <= reach(T)
                else:
                    assert reach(4) > er.WINDOW
    assert fv.egress_resample_tile(147, 160, 5121, 1, er.F32) == 4096 and fv.egress_resample_tile(147, 160, 5121, 2, er.PCM16) == 4096
    assert fv.egress_resample_tile(147, 160, 5121, 1, er.PCM16) == 7492
    assert fv.egress_resample_tile(1, 1, 20481, 1, er.F32) == 0 and fv.egress_resample_tile(3, 1, 20481, 1, er.F32) == 4096   # a reach of 20481 lane samples
    assert fv.egress_resample_tile(1, 1 << 31, 1, 1, er.F32) == 0                                      # not 4 outputs in 8192 samples
    assert fv.egress_resample_tile(0, 1, 3, 1, 0) == 0 and fv.egress_resample_tile(641, 1, 3, 1, 0) == 0 and fv.egress_resample_tile(1, 0, 3, 1, 0) == 0
    assert fv.egress_resample_tile(1, 1, 4, 1, 0) == 0 and fv.egress_resample_tile(1, 1, 0, 1, 0) == 0 and fv.egress_resample_tile(1, 1, 20483, 1, 0) == 0
    assert fv.egress_resample_tile(1, 1, 3, 0, 0) == 0 and fv.egress_resample_tile(1, 1, 3, 65, 0) == 0 and fv.egress_resample_tile(1, 1, 3, 1, 3) == 0


@pytest.mark.parametrize("up,down,n_taps", [(1, 3, 13), (2, 1, 13), (2, 3, 25), (7, 5, 29), (147, 160, 321), (3, 7, 1), (1, 1, 1), (5, 2, 3)])
def test_ready_against_brute_force(fv, up, down, n_taps):
    K = (n_taps - 1) // 2
    for sf in (0, 1, 2, 7, 23):
        OF = rc.out_frames(sf, up, down)
        for have in range(0, sf + 3):
            got = fv.egress_resample_ready(up, down, n_taps, sf, have)
            assert got == er.ready(up, down, n_taps, sf, have)
            if have >= sf:
                assert got == OF
                continue
            # the leading outputs whose window -- not clipped to the stream -- lies below `have`
            n = 0
            while n < OF and (n * down + K) // up < have:
                n += 1
            assert got == n, (sf, have)
            if got:   # ... so the frames below `have` cover the window of those outputs
                lo, hi = rc.window(up, down, n_taps, sf, 0, got)
                assert hi <= have


def test_ready_is_128_bit(fv):
    up, down, n_taps = 147, 160, 5121
    for sf, have in (((1 << 62) // up, (1 << 62) // up - 5), ((1 << 62) // up, 1 << 40), (U64_MAX, U64_MAX - 1), (U64_MAX, 1 << 63), (1 << 36, (1 << 36) - 1),
                     (U64_MAX // 640 * 640, 17)):
        assert fv.egress_resample_ready(up, down, n_taps, sf, have) == min(er.ready(up, down, n_taps, sf, have), U64_MAX), (sf, have)
    assert fv.egress_resample_ready(640, 1, 1, U64_MAX, U64_MAX - 1) == U64_MAX                # (out_frames saturates)
    assert fv.egress_resample_ready(1, 1 << 31, 1, U64_MAX, U64_MAX - 1) == er.ready(1, 1 << 31, 1, U64_MAX, U64_MAX - 1)
    assert fv.egress_resample_ready(0, 1, 3, 10, 5) == 0 and fv.egress_resample_ready(1, 0, 3, 10, 5) == 0 and fv.egress_resample_ready(1, 1, 4, 10, 5) == 0


# ---------------------------------------------------------------- fvad_egress_resample_check
# 2/3 with 25 taps (K = 12).  One good row on lanes 2..3 of 6, 100 samples each: a stereo PCM16 file of a stream of 60 lane samples
# (40 outputs); outputs [12, 32) -- which read stream samples [12, 53) -- go to byte 44; the lanes hold stream samples [10, 55)
# from lane sample 5 on
UP, DOWN, TAPS = 2, 3, np.linspace(0.1, 1.0, 25).astype(np.float32)
GOOD = (44, 20, 2, er.PCM16, 2, 5, 10, 45, 60, 12)
NAMES = ("byte_offset", "n_out", "n_channels", "format", "first_lane", "src_offset", "frame_base", "n_frames", "stream_frames", "out_from")


def check(fv, sinks, out_bytes=1000, up=UP, down=DOWN, taps=TAPS, n_lanes=6, lane_stride=101, n_samples=100, src_pcm16=False):
    return fv.egress_resample_check(sinks, out_bytes, up, down, taps, n_lanes, lane_stride, n_samples, src_pcm16)


def edit(**kw):
    return tuple(kw.get(n, v) for n, v in zip(NAMES, GOOD))


NONE = np.zeros((0, 10), np.uint64)


def test_check_accepts(fv):
    assert rc.window(UP, DOWN, 25, 60, 12, 20) == (12, 53)
    assert check(fv, [GOOD]) == OK
    assert check(fv, NONE) == OK and fv.lib().fvad_egress_resample_check(None, 0, 0, 1, 1, fv.fptr(TAPS), 25, 0, 0, 0, 0) == OK
    assert check(fv, [edit(frame_base=12, n_frames=41)]) == OK                                  # exactly the window
    assert check(fv, [edit(frame_base=0, n_frames=60)]) == OK                                   # the whole stream
    assert check(fv, [edit(n_out=0, n_frames=0)]) == OK and check(fv, [edit(n_out=0, n_frames=0, byte_offset=1000)]) == OK   # writes nothing
    assert check(fv, [edit(out_from=20, n_out=20, frame_base=24, n_frames=36)]) == OK           # up to the stream's last output
    assert check(fv, [edit(format=er.PCM24)]) == OK and check(fv, [edit(format=er.F32)]) == OK
    assert check(fv, [edit(n_channels=64, first_lane=0)], n_lanes=64, out_bytes=44 + 20 * 128) == OK
    assert check(fv, [edit(byte_offset=1000 - 80)]) == OK and check(fv, [edit(src_offset=55)]) == OK   # both ends exactly
    assert check(fv, [GOOD], out_bytes=U64_MAX) == OK
    assert check(fv, [edit(stream_frames=0, frame_base=0, n_frames=0, out_from=0, n_out=0)]) == OK     # an empty stream
    assert check(fv, [GOOD, edit(byte_offset=124)]) == OK and check(fv, [edit(byte_offset=124), GOOD]) == OK   # the same lanes twice, bytes that touch
    assert check(fv, [GOOD], taps=[1.0]) == OK
    # a phase without taps reads nothing: up 3 with the single tap, an output that is no multiple of 3 needs no frame
    assert check(fv, [edit(out_from=1, n_out=1, n_frames=0, frame_base=60)], up=3, down=1, taps=[1.0]) == OK


def test_check_invalid_arguments_in_order(fv):
    L, u64p = fv.lib(), fv.C.POINTER(fv.C.c_uint64)
    one = np.array([GOOD], np.uint64)
    rows, tp = one.ctypes.data_as(u64p), fv.fptr(TAPS)
    # 1. the lane format, the ratio, the taps -- each before "no sinks", each with everything behind it broken as well
    bad_row = np.array([edit(format=9, first_lane=99)], np.uint64).ctypes.data_as(u64p)
    assert L.fvad_egress_resample_check(rows, 1, 1000, UP, DOWN, tp, 25, 1, 6, 101, 100) == INVALID          # PCM16 lanes: a conversion
    assert L.fvad_egress_resample_check(rows, 1, 1000, UP, DOWN, tp, 25, 2, 6, 101, 100) == INVALID
    assert L.fvad_egress_resample_check(None, 0, 0, UP, DOWN, tp, 25, 1, 0, 0, 0) == INVALID                 # ... before "no sinks"
    assert check(fv, [GOOD], src_pcm16=True) == INVALID
    for up, down in ((0, 3), (641, 3), (2, 0)):
        assert check(fv, [GOOD], up=up, down=down) == INVALID and check(fv, NONE, up=up, down=down) == INVALID
    assert check(fv, [GOOD], taps=None) == INVALID and check(fv, NONE, taps=None) == INVALID
    assert check(fv, [GOOD], taps=TAPS[:24]) == INVALID                                         # an even count
    assert check(fv, [GOOD], taps=np.zeros(20483, np.float32)) == INVALID
    for v in (np.nan, np.inf, -np.inf):
        t = TAPS.copy()
        t[7] = v
        assert check(fv, [GOOD], taps=t) == INVALID and check(fv, NONE, taps=t) == INVALID
    # 2. NULL sinks, the stride
    assert L.fvad_egress_resample_check(None, 1, 1000, UP, DOWN, tp, 25, 0, 6, 101, 100) == INVALID
    assert check(fv, [GOOD], lane_stride=99) == INVALID
    assert check(fv, [edit(first_lane=0, n_channels=1)], n_lanes=1, lane_stride=0) == OK       # (one lane has no stride)
    assert L.fvad_egress_resample_check(bad_row, 1, 1000, UP, DOWN, tp, 25, 0, 6, 101, 100) == INVALID       # INVALID before RANGE
    # 3. per row
    assert check(fv, [edit(format=3)]) == INVALID
    assert check(fv, [edit(n_channels=0)]) == INVALID and check(fv, [edit(n_channels=65, first_lane=0)], n_lanes=100) == INVALID
    assert check(fv, [edit(stream_frames=(1 << 62) // 2)]) == INVALID                           # stream_frames * up >= 2^62
    assert check(fv, [edit(stream_frames=(1 << 62) // 2 - 1)]) == OK
    assert check(fv, [edit(out_from=21, frame_base=24, n_frames=36)]) == INVALID                # one output past the stream's 40
    assert check(fv, [edit(out_from=U64_MAX, n_out=2)]) == INVALID                              # out_from + n_out wraps
    assert check(fv, [edit(frame_base=16, n_frames=45)]) == INVALID                             # given frames past the stream's end
    assert check(fv, [edit(frame_base=U64_MAX)]) == INVALID                                     # frame_base + n_frames wraps
    assert check(fv, [edit(frame_base=13, n_frames=42)]) == INVALID                             # the window's first frame is missing
    assert check(fv, [edit(n_frames=42)]) == INVALID                                            # ... its last
    assert check(fv, [edit(n_frames=0)]) == INVALID
    assert check(fv, [GOOD, edit(byte_offset=200, n_frames=42)]) == INVALID                     # in any row
    assert check(fv, [edit(format=er.F32, frame_base=0, n_frames=60)], up=1, down=1, taps=np.ones(20481, np.float32)) == INVALID   # no tile: 4 outputs reach 20484 lane samples
    # the given-frames rule before the ranges: a short slice on lanes that do not exist is INVALID, not RANGE
    assert check(fv, [edit(n_frames=42, first_lane=6)]) == INVALID
    assert check(fv, [edit(first_lane=6), edit(byte_offset=200, n_frames=42)]) == INVALID       # a later row's own rule before an earlier row's range


def test_check_out_of_range_and_overlap(fv):
    assert check(fv, [edit(first_lane=6)]) == RANGE and check(fv, [edit(first_lane=5)]) == RANGE
    assert check(fv, [edit(first_lane=U64_MAX)]) == RANGE
    assert check(fv, [edit(src_offset=56)]) == RANGE and check(fv, [edit(src_offset=U64_MAX)]) == RANGE
    assert check(fv, [edit(src_offset=101, n_out=0, n_frames=0)]) == RANGE
    assert check(fv, [edit(byte_offset=1000 - 79)]) == RANGE                                    # one byte past the output
    assert check(fv, [edit(byte_offset=1001, n_out=0, n_frames=0)]) == RANGE
    assert check(fv, [edit(byte_offset=U64_MAX)], out_bytes=U64_MAX) == RANGE
    assert check(fv, [edit(format=er.PCM24, byte_offset=1000 - 119)]) == RANGE                  # 120 bytes of PCM24
    big = (1 << 62) // 2 - 1
    assert check(fv, [edit(stream_frames=big, frame_base=0, n_frames=big, out_from=0, n_out=rc.out_frames(big, UP, DOWN), n_channels=64, first_lane=0,
                           format=er.F32, src_offset=0)], n_lanes=64, n_samples=U64_MAX >> 1, lane_stride=U64_MAX >> 1, out_bytes=U64_MAX) == RANGE   # n_out * frame bytes wraps
    # 5. overlapping bytes, after every range
    assert check(fv, [GOOD, GOOD]) == INVALID
    assert check(fv, [GOOD, edit(byte_offset=123)]) == INVALID and check(fv, [edit(byte_offset=123), GOOD]) == INVALID
    assert check(fv, [GOOD, edit(byte_offset=50, n_out=1, format=er.F32)]) == INVALID
    assert check(fv, [GOOD, edit(byte_offset=50, n_out=0, n_frames=0)]) == OK                   # writes nothing
    assert check(fv, [GOOD, GOOD, edit(first_lane=6)]) == RANGE                                 # a range before the overlap


# ---------------------------------------------------------------- the model against the definition
@pytest.mark.parametrize("up,down,half,kind", er.RATIOS[:4] + ((3, 7, 1, "noise"),))
def test_the_model_is_the_definition(fv, up, down, half, kind):
    rng = np.random.default_rng(up * 100 + down)
    taps = rc.case_taps(up, down, half, "noise")
    for sf in (1, 2, 9, 31):
        x = rng.uniform(-1, 1, (sf, 2))
        OF = rc.out_frames(sf, up, down)
        table = {"rows": np.array([(44, OF, 2, er.F32, 1, 0, 0, sf, sf, 0)], np.uint64), "data": [x]}
        (y, B), = er.model(table, taps, up, down)
        for c in range(2):
            want = np.array([rc.brute(x[:, c], taps, up, down, o) for o in range(OF)])
            assert np.allclose(y[c], want, rtol=0, atol=1e-12)
        # a slice given exactly its window, or more, is the stream
        a, n = OF // 3, OF - OF // 3 - OF // 4
        lo, hi = rc.window(up, down, taps.size, sf, a, n)
        for l, h in ((lo, hi), (max(lo - 1, 0), min(hi + 2, sf))):
            piece = {"rows": np.array([(44, n, 2, er.F32, 1, 0, l, h - l, sf, a)], np.uint64), "data": [x[l:h]]}
            assert fv.egress_resample_check(piece["rows"], 44 + n * 8, up, down, taps, 3, sf + 1, sf) == OK   # a row the library takes
            (y2, B2), = er.model(piece, taps, up, down)
            assert np.array_equal(y2, y[:, a:a + n]) and np.array_equal(B2, B[:, a:a + n])


# ---------------------------------------------------------------- the case tables
@pytest.fixture(scope="module", params=er.RATIOS, ids=er.ratio_id)
def table(request, fv):
    up, down, half, kind = request.param
    taps = rc.case_taps(up, down, half, kind)
    t = er.case_table(up, down, taps.size)
    for fmt, C in rc.COMBOS:   # the table is laid out around the library's tile
        assert fv.egress_resample_tile(up, down, taps.size, C, fmt) == er.tile(up, down, taps.size, C, fmt) > 0
    return up, down, kind, taps, t, er.twin_f32(t), er.model(t, taps, up, down)


def test_the_case_tables_pass_the_check_and_bite(fv, table):
    up, down, kind, taps, t, t32, want = table
    assert np.array_equal(taps, fv.resample_design(up, down, (taps.size - 1) // 2 // max(up, down))) or kind == "noise"
    rows = t["rows"].astype(np.int64)
    for tb in (t, t32):
        assert fv.egress_resample_check(tb["rows"], tb["out_bytes"], up, down, taps, t["n_lanes"], t["lane_stride"], t["n_samples"]) == OK
    assert set(rows[:, 2].tolist()) == {1, 2, 3, 64} and set(rows[:, 3].tolist()) == {0, 1, 2}
    assert {0, 1, 5} <= set(rows[:, 8].tolist()) and rows[0, 0] == 44
    assert {int(b) % 2 for b in rows[:, 0]} == {0, 1} and {int(s) % 4 for s in rows[:, 5]} == {0, 1, 2, 3} and t["lane_stride"] > t["n_samples"]
    assert t["lane_stride"] % 2 == 1 and t["n_lanes"] * t["lane_stride"] < 4_000_000
    ends = set((rows[:, 0] + rows[:, 1] * rows[:, 2] * np.array([er.SAMPLE_BYTES[f] for f in rows[:, 3]])).tolist())
    assert sum(int(b) in ends for b in rows[:, 0]) >= 6                                         # rows that touch
    for i in t["big"]:
        _, n_out, C, fmt = rows[i, :4]
        T = fv.egress_resample_tile(up, down, taps.size, int(C), int(fmt))
        assert 2 * T < n_out < 3 * T and n_out % T                                              # two full tiles and a partial one
    assert len(t["big"]) == 6 and np.any((rows[:, 9] > 0) & (rows[:, 6] > 0) & ((rows[:, 9] * down) % up != 0) | (up == 1))
    # NaN everywhere outside the given frames, finite inside
    mask = np.ones(t["lanes"].shape, bool)
    for _, _, C, _, l0, src, _, nf, _, _ in rows.tolist():
        assert np.isfinite(t["lanes"][l0:l0 + C, src:src + nf]).all()
        mask[l0:l0 + C, src:src + nf] = False
    assert np.isnan(t["lanes"][mask]).all() and mask.sum() > t["n_lanes"]
    # a slice one frame short of its window does not pass
    i = t["big"][0]
    sl = er.slices(t["rows"][i], [int(rows[i, 1]) // 3, int(rows[i, 1]) // 3 + 1], up, down, taps.size)
    assert fv.egress_resample_check([s for s, _, _ in sl], t["out_bytes"], up, down, taps, t["n_lanes"], t["lane_stride"], t["n_samples"]) == OK
    short = list(sl[1][0])
    short[7] -= 1
    assert fv.egress_resample_check([tuple(short)], t["out_bytes"], up, down, taps, t["n_lanes"], t["lane_stride"], t["n_samples"]) == INVALID


def test_the_model_passes_its_own_table(table):
    up, down, _, taps, t, t32, want = table
    er.compare_f32(er.model_bytes(t32, want), t32, want, up, taps.size, "the model itself")
    spill = er.model_bytes(t32, want)
    spill[int(t32["rows"][3, 0]) - 1] = 0
    with pytest.raises(AssertionError):
        er.compare_f32(spill, t32, want, up, taps.size, "a byte in front of a row")


@pytest.mark.parametrize("mutation", er.MUTATIONS)
def test_wrong_models_fail_the_case_tables(table, mutation):
    # planar instead of interleaved; the phase counted from the row instead of the stream; a reversed tap walk; the window clipped
    # to the given frames' count instead of the stream.  Two of them cannot show everywhere: with up == 1 every output has the
    # one phase, and a symmetric design reads the same either way -- the ratios with up > 1, and the noise taps, show those.
    up, down, kind, taps, t, t32, want = table
    if (mutation == "row_phase" and up == 1) or (mutation == "reversed" and kind == "design"):
        wrong = er.model(t, taps, up, down, mutation)
        er.compare_f32(er.model_bytes(t32, wrong), t32, want, up, taps.size, "a mutation without effect here")
        return
    wrong = want if mutation == "planar" else er.model(t, taps, up, down, mutation)
    with pytest.raises(AssertionError):
        er.compare_f32(er.model_bytes(t32, wrong, mutation), t32, want, up, taps.size, mutation)
