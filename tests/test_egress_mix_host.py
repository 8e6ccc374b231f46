"""The host side of the two-source egress (fvad_nsnet2_delay, fvad_egress_mix_check; no GPU), the numpy model of
egress_mix_cases.py against the definition written out sample by sample, the proof that its case table bites -- six wrong
versions of the model each fail it -- and run_denoise's refusals of bad kinds, raised before any context is made."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import egress_cases as ec
import egress_mix_cases as mc

OK, INVALID, RANGE, BAD_RATE = 0, -100, -6, -9
U64_MAX = (1 << 64) - 1
EXPORTS = ("fvad_nsnet2_delay", "fvad_egress_mix_check", "fvad_egress_mix_device", "fvad_egress_mix")


def test_the_library_exports_the_mix_calls(fv):
    for name in EXPORTS:
        assert hasattr(fv.lib(), name), name
    assert fv.EGRESS_MIX_FIELDS == 8 == mc.FIELDS
    assert fv.lib().fvad_abi_version() == 3


# ---------------------------------------------------------------- fvad_nsnet2_delay
def test_the_delay(fv):
    assert fv.nsnet2_delay(48000) == 482 == mc.DELAY and fv.nsnet2_delay(16000) == 160 and fv.nsnet2_delay(32000) == 321
    assert fv.nsnet2_delay(96000) == 161 * 6 - 1
    d = C.c_uint64(77)
    for rate in (0, 44100, 8000, 47999, 16001):     # fvad_nsnet2_create's refusals
        assert fv.lib().fvad_nsnet2_delay(rate, C.byref(d)) == BAD_RATE and d.value == 0, rate
        assert fv.lib().fvad_nsnet2_chunk_size(rate) == 0
    assert fv.lib().fvad_nsnet2_delay(48000, None) == INVALID
    with pytest.raises(fv.FvadError):
        fv.nsnet2_delay(44100)


# ---------------------------------------------------------------- fvad_egress_mix_check
# one good sink of lanes 2..3 of 6: 10 stereo PCM16 frames to bytes [44, 84) of 1000, denoised samples 5..14 of 100, three
# leading zeros and then original samples 20..26 of 60
GOOD = (44, 10, 2, ec.PCM16, 2, 5, 20, 3)
NAMES = ("byte_offset", "n_frames", "n_channels", "format", "first_lane", "src_offset", "orig_offset", "orig_zeros")


def check(fv, sinks, out_bytes=1000, w=(1.0, -1.0), n_lanes=6, orig_stride=61, orig_samples=60, den_stride=101, den_samples=100, src_pcm16=False):
    return fv.egress_mix_check(sinks, out_bytes, w[0], w[1], n_lanes, orig_stride, orig_samples, den_stride, den_samples, src_pcm16)


def edit(**kw):
    return tuple(kw.get(n, v) for n, v in zip(NAMES, GOOD))


def test_check_accepts(fv):
    for w in mc.WEIGHTS:
        assert check(fv, [GOOD], w=w) == OK, w
    assert check(fv, np.zeros((0, 8), np.uint64)) == OK                                       # no sinks: nothing to do
    assert fv.lib().fvad_egress_mix_check(None, 0, 0, 0, 1.0, 1.0, 0, 0, 0, 0, 0) == OK
    assert check(fv, [edit(n_frames=0)]) == OK and check(fv, [edit(n_frames=0, byte_offset=1000, src_offset=100, orig_offset=60)]) == OK
    assert check(fv, [edit(byte_offset=1000 - 40)]) == OK and check(fv, [edit(src_offset=90)]) == OK   # both ends exactly
    assert check(fv, [edit(orig_offset=53)]) == OK and check(fv, [edit(orig_offset=50, orig_zeros=0)]) == OK   # 7 (10) samples to the end
    # every frame a zero: nothing of the original is read, wherever orig_offset == orig_samples points
    assert check(fv, [edit(orig_offset=60, orig_zeros=10)]) == OK and check(fv, [edit(orig_offset=60, orig_zeros=U64_MAX)]) == OK
    assert check(fv, [edit(n_channels=64, first_lane=0)], n_lanes=64, out_bytes=44 + 10 * 128) == OK
    assert check(fv, [edit(format=ec.PCM24)]) == OK and check(fv, [edit(format=ec.F32)]) == OK
    assert check(fv, [GOOD], out_bytes=U64_MAX) == OK and check(fv, [edit(byte_offset=U64_MAX - 40)], out_bytes=U64_MAX) == OK
    assert check(fv, [GOOD, edit(byte_offset=84)]) == OK and check(fv, [edit(byte_offset=84), GOOD]) == OK   # ranges that touch
    assert check(fv, [GOOD, edit(n_frames=0, byte_offset=50)]) == OK
    assert check(fv, [edit(first_lane=0, n_channels=1)], n_lanes=1, orig_stride=0, den_stride=0) == OK   # one lane needs no stride


def test_check_weights_come_first(fv):
    bad = [(float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0, float("-inf")), (0.0, 0.0), (-0.0, 0.0), (3.5e38 * 10, 1.0)]
    for w in bad:
        assert check(fv, [GOOD], w=w) == INVALID, w
        assert check(fv, np.zeros((0, 8), np.uint64), w=w) == INVALID, w                       # also without sinks
        assert check(fv, [edit(first_lane=6)], w=w) == INVALID, w                              # before a range
    assert check(fv, [GOOD], src_pcm16=True) == INVALID                                       # PCM16 lanes are refused
    assert check(fv, [GOOD], w=(1e-45, 0.0)) == OK                                            # a subnormal weight is not zero


def test_check_invalid_arguments(fv):
    L, u64p = fv.lib(), C.POINTER(C.c_uint64)
    one = np.array([GOOD], np.uint64)
    assert L.fvad_egress_mix_check(None, 1, 1000, 0, 1.0, -1.0, 6, 61, 60, 101, 100) == INVALID   # NULL sinks
    assert L.fvad_egress_mix_check(one.ctypes.data_as(u64p), 1, 1000, 2, 1.0, -1.0, 6, 61, 60, 101, 100) == INVALID   # no such lanes
    assert check(fv, [GOOD], orig_stride=59) == INVALID and check(fv, [GOOD], den_stride=99) == INVALID   # lanes would overlap
    assert check(fv, [edit(format=3)]) == INVALID and check(fv, [edit(format=U64_MAX)]) == INVALID
    assert check(fv, [edit(n_channels=0)]) == INVALID
    assert check(fv, [edit(n_channels=65, first_lane=0)], n_lanes=100) == INVALID and check(fv, [edit(n_channels=U64_MAX)]) == INVALID
    assert check(fv, [GOOD, edit(byte_offset=200, n_channels=0)]) == INVALID                  # in any row
    # the order: a bad argument before a bad sink before a range; every sink's own rules before any sink's ranges
    assert check(fv, [edit(first_lane=6)], den_stride=99) == INVALID
    assert check(fv, [edit(first_lane=6), edit(byte_offset=200, format=3)]) == INVALID


def test_check_out_of_range(fv):
    assert check(fv, [edit(first_lane=6)]) == RANGE and check(fv, [edit(first_lane=5)]) == RANGE   # lanes past n_lanes
    assert check(fv, [edit(first_lane=U64_MAX)]) == RANGE and check(fv, [edit(first_lane=U64_MAX - 1)]) == RANGE
    assert check(fv, [edit(src_offset=91)]) == RANGE and check(fv, [edit(src_offset=101, n_frames=0)]) == RANGE   # past den_samples
    assert check(fv, [edit(src_offset=U64_MAX)]) == RANGE and check(fv, [edit(n_frames=U64_MAX)]) == RANGE        # the sums wrap
    assert check(fv, [edit(src_offset=U64_MAX - 4)], den_samples=U64_MAX, den_stride=U64_MAX) == RANGE
    assert check(fv, [edit(orig_offset=54)]) == RANGE and check(fv, [edit(orig_offset=51, orig_zeros=0)]) == RANGE   # one past orig_samples
    assert check(fv, [edit(orig_offset=54, orig_zeros=4)]) == OK                              # one more zero, one sample less
    assert check(fv, [edit(orig_offset=61, orig_zeros=10)]) == RANGE and check(fv, [edit(orig_offset=61, n_frames=0)]) == RANGE
    assert check(fv, [edit(orig_offset=U64_MAX)]) == RANGE and check(fv, [edit(orig_offset=U64_MAX - 3)], orig_samples=U64_MAX, orig_stride=U64_MAX) == RANGE
    assert check(fv, [edit(orig_offset=U64_MAX - 7)], orig_samples=U64_MAX, orig_stride=U64_MAX) == OK
    assert check(fv, [edit(byte_offset=1000 - 39)]) == RANGE and check(fv, [edit(byte_offset=1001, n_frames=0)]) == RANGE
    assert check(fv, [edit(byte_offset=U64_MAX)], out_bytes=U64_MAX) == RANGE and check(fv, [edit(byte_offset=U64_MAX - 39)], out_bytes=U64_MAX) == RANGE
    big = dict(den_samples=1 << 62, den_stride=1 << 62, orig_samples=1 << 62, orig_stride=1 << 62, out_bytes=U64_MAX)
    assert check(fv, [edit(n_frames=1 << 62, src_offset=0, orig_offset=0)], **big) == RANGE    # n_frames * frame bytes wraps
    assert check(fv, [edit(format=ec.PCM24, byte_offset=1000 - 59)]) == RANGE                # 60 bytes of PCM24
    assert check(fv, [GOOD, GOOD, edit(first_lane=6)]) == RANGE                              # a range before an overlap


def test_check_skips_the_ranges_of_a_source_whose_weight_is_zero(fv):
    wild = dict(src_offset=U64_MAX, orig_offset=U64_MAX - 1)
    assert check(fv, [edit(src_offset=91)], w=(1.0, 0.0)) == OK and check(fv, [edit(src_offset=U64_MAX)], w=(1.0, 0.0)) == OK
    assert check(fv, [edit(orig_offset=54)], w=(0.0, 1.0)) == OK and check(fv, [edit(orig_offset=U64_MAX)], w=(0.0, 1.0)) == OK
    assert check(fv, [edit(**wild)], w=(1.0, 0.0)) == RANGE and check(fv, [edit(**wild)], w=(0.0, 1.0)) == RANGE   # the other one still counts
    assert check(fv, [GOOD], w=(1.0, 0.0), den_stride=0, den_samples=0) == OK and check(fv, [GOOD], w=(0.0, 1.0), orig_stride=0, orig_samples=0) == OK
    assert check(fv, [GOOD], w=(1.0, 0.0), den_stride=5, den_samples=100) == OK               # nor its stride
    assert check(fv, [GOOD], w=(1.0, 0.0), orig_stride=59) == INVALID and check(fv, [edit(first_lane=6)], w=(1.0, 0.0)) == RANGE


def test_check_overlap(fv):
    assert check(fv, [GOOD, GOOD]) == INVALID                                                # the same bytes twice
    assert check(fv, [GOOD, edit(byte_offset=83)]) == INVALID and check(fv, [edit(byte_offset=83), GOOD]) == INVALID   # one byte, either order
    assert check(fv, [GOOD, edit(byte_offset=60, n_frames=1, first_lane=0)]) == INVALID      # inside, from other lanes
    assert check(fv, [GOOD, edit(byte_offset=400), edit(byte_offset=84, n_frames=79, n_channels=1, format=ec.F32, src_offset=0, orig_offset=0, orig_zeros=79)]) == OK
    assert check(fv, [GOOD, edit(byte_offset=400), edit(byte_offset=83, n_frames=79, n_channels=1, format=ec.F32, src_offset=0, orig_offset=0, orig_zeros=79)]) == INVALID
    assert check(fv, [edit(byte_offset=U64_MAX - 40), edit(byte_offset=U64_MAX - 41)], out_bytes=U64_MAX) == INVALID


# ---------------------------------------------------------------- the case table
@functools.lru_cache(maxsize=None)
def build_table(w):
    t = mc.case_table(*w)
    t["w"] = w
    t["out_in"] = ec.canaries(t["out_bytes"])
    t["want"] = mc.mix_model(t["orig"], t["den"], t["sinks"], w[0], w[1], t["out_in"])
    return t


@pytest.fixture(scope="module", params=mc.WEIGHTS, ids=[f"{a}x{b}" for a, b in mc.WEIGHTS])
def table(request):
    return build_table(request.param)


def test_the_case_table_is_what_the_issue_asks_for(fv, table):
    snk = table["sinks"].astype(object)     # (orig_zeros reaches 2^63)
    formats = {ec.F32, ec.PCM16, ec.PCM24}
    assert set(snk[:, 3].tolist()) == formats and set(snk[:, 2].tolist()) == {1, 2, 3, 5}
    for fmt in formats:
        rows = snk[snk[:, 3] == fmt]
        assert {int(b) % 16 for b in rows[:, 0]} == set(range(16)), fmt                       # every byte alignment, per format
        for Cn in (1, 2, 3, 5):
            assert {0, 1, 3, 4, 5} <= set(rows[rows[:, 2] == Cn, 1].tolist())
        for Cn in ec.BIG[fmt]:
            T = fv.ingest_tile_frames(Cn, fmt)
            assert T == ec.tile_frames(Cn, fmt)
            big = rows[rows[:, 2] == Cn]
            assert {T - 1, T, T + 1, 2 * T + 3} <= set(big[:, 1].tolist())
            assert any(r[7] == T + 5 and r[1] > T + 5 for r in big), (fmt, Cn)               # zeros that end inside the second tile
    # both sources' alignments independently: both, either and neither on a 16-byte boundary (lanes of an odd stride move it again)
    assert {(int(r[5]) % 8, int(r[6]) % 8) for r in snk if r[1] >= mc.ALIGN_FRAMES} >= {(a, b) for a in range(8) for b in range(8)}
    zeros = {int(r[7]) for r in snk if r[1] > r[7]}
    assert {0, 1, 3, mc.DELAY} <= zeros and any(r[7] == r[1] > 0 for r in snk) and any(r[7] > r[1] > 0 for r in snk)
    assert table["orig_stride"] % 2 == 1 and table["den_stride"] % 2 == 0 and table["orig_stride"] != table["den_stride"]
    assert table["orig_stride"] > table["orig_samples"] and table["den_stride"] > table["den_samples"]
    assert not np.all(np.diff(table["sinks"][:, 0].astype(np.int64)) >= 0)                   # shuffled
    a, b = snk[table["names"]["adjacent-a"]], snk[table["names"]["adjacent-b"]]
    assert a[0] + a[1] * a[2] * ec.SAMPLE_BYTES[int(a[3])] == b[0]                            # the touching pair
    w = table["w"]
    assert fv.egress_mix_check(table["sinks"], table["out_bytes"], w[0], w[1], table["n_lanes"], table["orig_stride"], table["orig_samples"],
                               table["den_stride"], table["den_samples"]) == OK
    assert table["orig"].nbytes + table["den"].nbytes < 16_000_000 and table["out_bytes"] < 2_000_000
    # canaries wherever no sink writes, a PAD_BYTE or more around every sink but the touching pair
    written = np.zeros(table["out_bytes"], bool)
    for k in table["names"].values():
        o, n, Cn, fmt = (int(x) for x in snk[k, :4])
        assert not written[o:o + n * Cn * ec.SAMPLE_BYTES[fmt]].any()
        written[o:o + n * Cn * ec.SAMPLE_BYTES[fmt]] = True
    for name, k in table["names"].items():
        o, n, Cn, fmt = (int(x) for x in snk[k, :4])
        end = o + n * Cn * ec.SAMPLE_BYTES[fmt]
        assert name == "adjacent-b" or not written[o - 1], name
        assert name == "adjacent-a" or not written[end], name
    assert np.all(table["want"][~written] == ec.PAD_BYTE)
    # the lanes: NaN outside the ranges a row may read (a source whose weight is zero: +-inf everywhere, and never a NaN)
    for lanes, weight, col, count in ((table["den"], w[1], 5, lambda r: int(r[1])), (table["orig"], w[0], 6, lambda r: int(r[1]) - min(int(r[7]), int(r[1])))):
        if weight == 0:
            assert np.all(np.isinf(lanes)) and (lanes > 0).any() and (lanes < 0).any()
            continue
        inside = np.zeros(lanes.shape, bool)
        for r in snk:
            inside[int(r[4]):int(r[4]) + int(r[2]), int(r[col]):int(r[col]) + count(r)] = True
        assert np.all(np.isnan(lanes[~inside])) and np.abs(lanes[inside & np.isfinite(lanes)]).max() > 1.0   # noise past +-1
    mc.compare(mc.mix_model(table["orig"], table["den"], table["sinks"][::-1], w[0], w[1], table["out_in"]), table["want"], table["sinks"], "the model, sinks reversed")


@pytest.mark.parametrize("w", [w for w in mc.WEIGHTS if 0.0 in w])
def test_a_zero_weight_never_meets_an_infinity(w):
    table = build_table(w)
    one = (1.0, 0.0) if w[1] == 0 else (0.0, 1.0)
    seen = 0
    for row in table["sinks"]:
        if int(row[3]) != ec.F32 or int(row[1]) == 0:
            continue
        o, n, Cn = int(row[0]), int(row[1]), int(row[2])
        got = table["want"][o:o + n * Cn * 4].copy().view("<f4")
        src = mc.mix_values(table["orig"], table["den"], row, one[0], one[1])   # the live source's own samples (a weight of 1)
        assert np.array_equal(np.isnan(got), np.isnan(src))   # a NaN only where the live source holds one
        seen += int(np.isnan(got).sum())
    assert seen > 0   # (the special values hold some)


def test_a_negative_weight_alone_writes_negative_zeros():
    # w = (-1, 0): x = +0.0f for the leading frames, so v = -1 (x) +0 = -0.0f: bits 0x80000000 in an f32 file, 0 in a PCM file
    t = build_table((-1.0, 0.0))
    seen = {ec.F32: 0, ec.PCM16: 0, ec.PCM24: 0}
    for o, n, Cn, fmt, _, _, _, z in t["sinks"].astype(object):
        k = min(z, n)
        if k == 0:
            continue
        B = ec.SAMPLE_BYTES[fmt]
        head = t["want"][o:o + k * Cn * B]
        if fmt == ec.F32:
            assert np.all(head.copy().view("<u4") == 0x80000000)
        else:
            assert not head.any()
        seen[fmt] += k * Cn
    assert all(v > 1000 for v in seen.values()), seen
    # and the same sinks with w = (1, 0) hold +0.0f there
    p = build_table((1.0, 0.0))
    o, n, Cn = next((int(r[0]), int(r[1]), int(r[2])) for r in p["sinks"] if int(r[3]) == ec.F32 and min(int(r[7]), int(r[1])) > 0)
    assert p["want"][o:o + 4].copy().view("<u4")[0] == 0


def test_the_model_is_the_definition_written_out(table):
    w = table["w"]
    snk = table["sinks"]
    few = snk[(snk[:, 1] <= mc.ALIGN_FRAMES) & (snk[:, 7] <= mc.ALIGN_FRAMES + 2)]
    assert len(few) > 60
    want = mc.mix_model(table["orig"], table["den"], few, w[0], w[1], table["out_in"])
    mc.compare(mc.naive_model(table["orig"], table["den"], few, w[0], w[1], table["out_in"]), want, few, "the naive model")


def test_pass_through_is_the_single_source_model():
    # (0, 1) is fvad_egress of the denoised lanes, bit for bit, where no NaN is (and NaN for NaN there)
    t = build_table((0.0, 1.0))
    want = ec.egress_model(t["den"], mc.as_egress_rows(t["sinks"]), False, t["out_in"])
    mc.compare(t["want"], want, t["sinks"], "w = (0, 1) against egress_cases' model")


DISTINGUISHES = {"no_delay": [w for w in mc.WEIGHTS if w[0] != 0], "zeros_read": [w for w in mc.WEIGHTS if w[0] != 0],
                 "swapped": list(mc.WEIGHTS), "single_round": [(0.25, 0.75), (-0.3, 1.7)],
                 "zero_times": [w for w in mc.WEIGHTS if 0.0 in w], "planar": list(mc.WEIGHTS)}


@pytest.mark.parametrize("mutation,w", [(m, w) for m in mc.MUTATIONS for w in DISTINGUISHES[m]])
def test_a_wrong_model_fails_the_case_table(mutation, w):
    # (products by 1 and -1 are exact, so (1, -1) cannot tell one rounding of the sum from three; a weight that is absent cannot
    # tell what its source's zeros were)
    t = build_table(w)
    with pytest.raises(AssertionError):
        mc.compare(mc.mix_model(t["orig"], t["den"], t["sinks"], w[0], w[1], t["out_in"], mutation=mutation), t["want"], t["sinks"], mutation)


def test_the_mutations_are_all_there():
    assert set(DISTINGUISHES) == set(mc.MUTATIONS) and all(DISTINGUISHES[m] for m in mc.MUTATIONS)


# ---------------------------------------------------------------- run_denoise's refusals
def test_run_denoise_refuses_bad_kinds_before_any_work(pkg, tmp_path, monkeypatch):
    sim = pkg.simulator
    made = []
    monkeypatch.setattr(sim, "_make_ctx", lambda *a, **k: made.append(a) or (_ for _ in ()).throw(AssertionError("a context was made")))
    plan = tmp_path / "plan.json"
    plan.write_text(json.dumps({"instances": []}))
    out = tmp_path / "never"
    bad = [dict(kinds=("denoised", "wet")), dict(kinds="residual"), dict(kinds=()), dict(kinds=("mix",)), dict(kinds=("mix",), mix=0.0),
           dict(kinds=("mix",), mix=1.0), dict(kinds=("mix",), mix=float("nan")), dict(kinds=("mix",), mix="0.5"), dict(kinds=("mix",), mix=True),
           dict(kinds=("residual",), mix=0.5), dict(mix=0.5), dict(kinds=("denoised", "denoised")),
           dict(kinds=("original",), rate=44100), dict(kinds=("denoised", "residual"), rate="source"), dict(kinds=("residual",), fmt="flac")]
    for kw in bad:
        with pytest.raises(ValueError):
            sim.run_denoise(str(plan), str(out), **kw)
    for argv in (["--denoised-kinds", "residual"], ["--denoised-mix", "0.5"]):
        with pytest.raises(ValueError, match="--export-denoised"):
            sim.main(["-i", str(plan)] + argv)
    with pytest.raises(ValueError):
        sim.main(["-i", str(plan), "--export-denoised", str(out), "--denoised-kinds", "residual,wet"])
    with pytest.raises(ValueError):
        sim.main(["-i", str(plan), "--export-denoised", str(out), "--denoised-kinds", "original", "--denoised-rate", "16000"])
    assert not made and not out.exists()
    assert sim.DENOISED_KINDS == ("denoised", "original", "residual", "mix")
