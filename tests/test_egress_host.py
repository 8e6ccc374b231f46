"""The host side of the device-side egress (fvad_wav_header, fvad_egress_check; no GPU), and the proof that the case table of
egress_cases.py bites: six wrong versions of the numpy model each fail it."""
import ctypes as C
import functools

import numpy as np
import pytest

import egress_cases as ec

OK, INVALID, RANGE, TOO_SMALL = 0, -100, -6, -106
U64_MAX = (1 << 64) - 1
EXPORTS = ("fvad_wav_header", "fvad_egress_check", "fvad_egress_device", "fvad_egress")


def test_the_library_exports_the_egress_calls(fv):
    for name in EXPORTS:
        assert hasattr(fv.lib(), name), name
    assert fv.EGRESS_FIELDS == 6 and fv.WAV_HEADER_BYTES == 44


# ---------------------------------------------------------------- fvad_wav_header
@pytest.mark.parametrize("frames", [0, 1, 1001])
@pytest.mark.parametrize("channels,rate", [(1, 48000), (2, 44100), (5, 16000), (64, 8000)])
def test_the_header_is_what_the_writers_write(fv, tmp_path, channels, rate, frames):
    p = str(tmp_path / "w.wav")
    fv.wav_write(p, np.zeros((channels, frames), np.float32), sample_rate=rate)
    with open(p, "rb") as f:
        assert f.read(44) == fv.wav_header(fv.INGEST_F32, channels, rate, frames)
    fv.wav_write_i16(p, np.zeros((channels, frames), np.int16), sample_rate=rate)
    with open(p, "rb") as f:
        assert f.read(44) == fv.wav_header(fv.INGEST_PCM16, channels, rate, frames)


@pytest.mark.parametrize("fmt,bits", [(ec.F32, 32), (ec.PCM16, 16), (ec.PCM24, 24)])
@pytest.mark.parametrize("channels,rate,frames", [(1, 48000, 0), (2, 44100, 7), (3, 16000, 1000), (64, 48000, 3)])
def test_probe_returns_the_headers_arguments(fv, tmp_path, fmt, bits, channels, rate, frames):
    p = tmp_path / "h.wav"
    head = fv.wav_header(fmt, channels, rate, frames)
    assert len(head) == 44
    p.write_bytes(head + bytes(frames * channels * ec.SAMPLE_BYTES[fmt]))
    assert fv.wav_probe(str(p)) == {"format": fmt, "n_channels": channels, "sample_rate": rate, "data_offset": 44, "n_frames": frames, "bits": bits}


def test_the_24_bit_header(fv):
    h = fv.wav_header(fv.INGEST_PCM24, 2, 48000, 10)
    assert h[:4] == b"RIFF" and int.from_bytes(h[4:8], "little") == 36 + 60 and h[8:16] == b"WAVEfmt " and int.from_bytes(h[16:20], "little") == 16
    assert [int.from_bytes(h[a:b], "little") for a, b in ((20, 22), (22, 24), (24, 28), (28, 32), (32, 34), (34, 36))] == [1, 2, 48000, 288000, 6, 24]
    assert h[36:40] == b"data" and int.from_bytes(h[40:44], "little") == 60


def test_the_header_refuses_what_the_writers_refuse(fv):
    L = fv.lib()
    buf, n = np.full(64, 0xEE, np.uint8), C.c_size_t(99)

    def status(fmt, channels, rate, frames, out="own", cap=64, n_bytes="own"):
        return L.fvad_wav_header(fmt, channels, rate, frames, buf.ctypes.data if out == "own" else out, cap, C.byref(n) if n_bytes == "own" else n_bytes)

    for args in ((3, 1, 48000, 1), (-1, 1, 48000, 1), (0, 0, 48000, 1), (0, 65536, 48000, 1), (0, 1, 0, 1),
                 (0, 1, 48000, 0xFFFFFF00 // 4 + 1), (1, 2, 48000, 0xFFFFFF00 // 4 + 1), (2, 1, 48000, 0xFFFFFF00 // 3 + 1),
                 (0, 1, 48000, U64_MAX), (2, 65535, 48000, U64_MAX // 3)):
        assert status(*args) == INVALID and n.value == 0, args
    assert status(0, 1, 48000, 1, out=None) == INVALID and status(0, 1, 48000, 1, n_bytes=None) == INVALID
    assert np.all(buf == 0xEE)
    assert status(0, 1, 48000, 1, cap=43) == TOO_SMALL and n.value == 44 and np.all(buf == 0xEE)
    assert status(0, 1, 48000, 0xFFFFFF00 // 4) == OK and status(2, 65535, 48000, 1) == OK and n.value == 44   # the largest that fit
    assert status(1, 2, 48000, 5, cap=44) == OK and np.all(buf[44:] == 0xEE)
    with pytest.raises(fv.FvadError):
        fv.wav_header(fv.INGEST_F32, 0, 48000, 1)


# ---------------------------------------------------------------- fvad_egress_check
# one good sink of lanes 2..3 of 6, 100 samples each: 10 stereo PCM16 frames from sample 5 to bytes [44, 84) of 1000
GOOD = (44, 10, 2, ec.PCM16, 2, 5)


def check(fv, sinks, out_bytes=1000, src_pcm16=False, n_lanes=6, lane_stride=101, n_samples=100):
    return fv.egress_check(sinks, out_bytes, src_pcm16, n_lanes, lane_stride, n_samples)


def edit(**kw):
    names = ("byte_offset", "n_frames", "n_channels", "format", "first_lane", "src_offset")
    return tuple(kw.get(n, v) for n, v in zip(names, GOOD))


def test_check_accepts(fv):
    assert check(fv, [GOOD]) == OK and check(fv, [GOOD], src_pcm16=True) == OK
    assert check(fv, np.zeros((0, 6), np.uint64)) == OK                                      # no sinks: nothing to do
    assert fv.lib().fvad_egress_check(None, 0, 0, 0, 0, 0, 0) == OK
    assert check(fv, [edit(n_frames=0)]) == OK and check(fv, [edit(n_frames=0, byte_offset=1000, src_offset=100)]) == OK   # writes nothing
    assert check(fv, [edit(byte_offset=1000 - 40)]) == OK and check(fv, [edit(src_offset=90)]) == OK   # both ends exactly
    assert check(fv, [edit(n_channels=64, first_lane=0)], n_lanes=64, out_bytes=44 + 10 * 128) == OK
    assert check(fv, [edit(format=ec.PCM24)]) == OK and check(fv, [edit(format=ec.F32)]) == OK
    assert check(fv, [GOOD], out_bytes=U64_MAX) == OK and check(fv, [edit(byte_offset=U64_MAX - 40)], out_bytes=U64_MAX) == OK
    # the same lanes twice (reading is shared), ranges that touch in either order, an empty sink inside another
    assert check(fv, [GOOD, edit(byte_offset=84)]) == OK and check(fv, [edit(byte_offset=84), GOOD]) == OK
    assert check(fv, [GOOD, edit(byte_offset=4)]) == OK
    assert check(fv, [GOOD, edit(n_frames=0, byte_offset=50)]) == OK
    assert check(fv, [GOOD], n_lanes=4, lane_stride=100) == OK and check(fv, [edit(first_lane=0, n_channels=1)], n_lanes=1, lane_stride=0) == OK


def test_check_invalid_arguments(fv):
    L, u64p = fv.lib(), C.POINTER(C.c_uint64)
    one = np.array([GOOD], np.uint64)
    assert L.fvad_egress_check(None, 1, 1000, 0, 6, 101, 100) == INVALID                      # NULL sinks
    assert L.fvad_egress_check(one.ctypes.data_as(u64p), 1, 1000, 2, 6, 101, 100) == INVALID   # PCM24 lanes do not exist
    assert L.fvad_egress_check(one.ctypes.data_as(u64p), 1, 1000, -1, 6, 101, 100) == INVALID
    assert check(fv, [GOOD], lane_stride=99) == INVALID                                       # lanes would overlap
    assert check(fv, [edit(format=3)]) == INVALID and check(fv, [edit(format=U64_MAX)]) == INVALID   # no such format
    assert check(fv, [edit(format=ec.F32)], src_pcm16=True) == INVALID                        # conversions, not egress
    assert check(fv, [edit(format=ec.PCM24)], src_pcm16=True) == INVALID
    assert check(fv, [edit(n_channels=0)]) == INVALID
    assert check(fv, [edit(n_channels=65, first_lane=0)], n_lanes=100) == INVALID and check(fv, [edit(n_channels=U64_MAX)]) == INVALID
    assert check(fv, [GOOD, edit(byte_offset=200, n_channels=0)]) == INVALID                  # in any row
    # the order: a bad argument before a bad sink before a range; every sink's own rules before any sink's ranges
    assert check(fv, [edit(first_lane=6)], lane_stride=99) == INVALID
    assert check(fv, [edit(first_lane=6), edit(byte_offset=200, format=3)]) == INVALID
    assert L.fvad_egress_check(None, 1, 1000, 2, 6, 101, 100) == INVALID


def test_check_out_of_range(fv):
    assert check(fv, [edit(first_lane=6)]) == RANGE and check(fv, [edit(first_lane=5)]) == RANGE   # lanes past n_lanes
    assert check(fv, [edit(first_lane=U64_MAX)]) == RANGE and check(fv, [edit(first_lane=U64_MAX - 1)]) == RANGE
    assert check(fv, [edit(src_offset=91)]) == RANGE and check(fv, [edit(src_offset=101, n_frames=0)]) == RANGE   # past n_samples
    assert check(fv, [edit(src_offset=U64_MAX)]) == RANGE and check(fv, [edit(n_frames=U64_MAX)]) == RANGE        # src_offset + n_frames wraps
    assert check(fv, [edit(src_offset=U64_MAX - 4)], n_samples=U64_MAX, lane_stride=U64_MAX) == RANGE
    assert check(fv, [edit(byte_offset=1000 - 39)]) == RANGE                                 # one byte past the output
    assert check(fv, [edit(byte_offset=1001, n_frames=0)]) == RANGE
    assert check(fv, [edit(byte_offset=U64_MAX)], out_bytes=U64_MAX) == RANGE and check(fv, [edit(byte_offset=U64_MAX - 39)], out_bytes=U64_MAX) == RANGE
    assert check(fv, [edit(n_frames=1 << 62, src_offset=0)], n_samples=1 << 62, lane_stride=1 << 62, out_bytes=U64_MAX) == RANGE   # n_frames * frame bytes wraps
    assert check(fv, [edit(format=ec.PCM24, byte_offset=1000 - 59)]) == RANGE                # 60 bytes of PCM24
    assert check(fv, [GOOD, GOOD, edit(first_lane=6)]) == RANGE                              # a range before an overlap


def test_check_overlap(fv):
    assert check(fv, [GOOD, GOOD]) == INVALID                                                # the same bytes twice
    assert check(fv, [GOOD, edit(byte_offset=83)]) == INVALID and check(fv, [edit(byte_offset=83), GOOD]) == INVALID   # one byte, either order
    assert check(fv, [GOOD, edit(byte_offset=5)]) == INVALID
    assert check(fv, [GOOD, edit(byte_offset=60, n_frames=1, first_lane=0)]) == INVALID      # inside, from other lanes
    assert check(fv, [GOOD, edit(byte_offset=400), edit(byte_offset=0, n_frames=100, n_channels=1, format=ec.F32, src_offset=0)]) == INVALID   # a long range over a short one
    assert check(fv, [GOOD, edit(byte_offset=400), edit(byte_offset=84, n_frames=79, n_channels=1, format=ec.F32, src_offset=0)]) == OK        # [84, 400) between the two
    assert check(fv, [edit(byte_offset=U64_MAX - 40), edit(byte_offset=U64_MAX - 41)], out_bytes=U64_MAX) == INVALID


# ---------------------------------------------------------------- the case table
@functools.lru_cache(maxsize=None)
def build_table(src_pcm16):
    t = ec.case_table(src_pcm16)
    t["src_pcm16"] = src_pcm16
    t["out_in"] = ec.canaries(t["out_bytes"])
    t["want"] = ec.egress_model(t["lanes"], t["sinks"], src_pcm16, t["out_in"])
    return t


@pytest.fixture(scope="module", params=[False, True], ids=["from-f32", "from-pcm16"])
def table(request):
    return build_table(request.param)


def test_the_case_table_is_what_the_issue_asks_for(fv, table):
    snk, src_pcm16 = table["sinks"].astype(np.int64), table["src_pcm16"]
    formats = {ec.PCM16} if src_pcm16 else {ec.F32, ec.PCM16, ec.PCM24}
    assert set(snk[:, 3].tolist()) == formats and set(snk[:, 2].tolist()) == {1, 2, 3, 5}
    for fmt in formats:
        rows = snk[snk[:, 3] == fmt]
        assert {int(b) % 16 for b in rows[:, 0]} == set(range(16)), fmt                       # every byte alignment, per format
        for Cn in (1, 2, 3, 5):
            assert {0, 1, 3, 4, 5} <= set(rows[rows[:, 2] == Cn, 1].tolist())
            T = fv.ingest_tile_frames(Cn, fmt)
            assert T == ec.tile_frames(Cn, fmt) and T % 4 == 0 and T * Cn * ec.SAMPLE_BYTES[fmt] <= fv.INGEST_TILE_BYTES
        for Cn in ec.BIG[fmt]:
            T = ec.tile_frames(Cn, fmt)
            assert {T - 1, T, T + 1, 2 * T + 3} <= set(rows[rows[:, 2] == Cn, 1].tolist())
    assert {int(d) % 8 for d in snk[:, 5]} == set(range(8))
    assert table["lane_stride"] % 2 == 1 and table["lane_stride"] > table["n_samples"]
    assert not np.all(np.diff(snk[:, 0]) >= 0)                                               # shuffled
    a, b = snk[table["names"]["adjacent-a"]], snk[table["names"]["adjacent-b"]]
    assert a[0] + a[1] * a[2] * ec.SAMPLE_BYTES[int(a[3])] == b[0]                            # the touching pair
    assert fv.egress_check(table["sinks"], table["out_bytes"], src_pcm16, table["n_lanes"], table["lane_stride"], table["n_samples"]) == OK
    assert table["n_lanes"] * table["lane_stride"] < 4_000_000 and table["out_bytes"] < 2_000_000
    # a PAD_BYTE or more in front of and behind every sink but the touching pair; canaries wherever no sink writes
    written = np.zeros(table["out_bytes"], bool)
    for name, k in table["names"].items():
        o, n, Cn, fmt = snk[k, :4].tolist()
        end = o + n * Cn * ec.SAMPLE_BYTES[fmt]
        assert not written[o:end].any()
        written[o:end] = True
    for name, k in table["names"].items():
        o, n, Cn, fmt = snk[k, :4].tolist()
        end = o + n * Cn * ec.SAMPLE_BYTES[fmt]
        assert name == "adjacent-b" or not written[o - 1], name
        assert name == "adjacent-a" or not written[end], name
    want = table["want"]
    assert np.all(want[~written] == ec.PAD_BYTE) and want.size == table["out_bytes"]
    ec.compare(ec.egress_model(table["lanes"], table["sinks"][::-1], src_pcm16, table["out_in"]), want, "the model, sinks reversed")


def test_the_model_on_the_special_values():
    t = build_table(False)
    snk = t["sinks"].astype(np.int64)
    n = len(ec.F32_FIRST)

    def first(name, B):
        o = int(snk[t["names"][name], 0])
        return t["want"][o:o + n * B].reshape(n, B).astype(np.int64)

    b = first(f"big-{ec.PCM16}-1-3", 2)
    got16 = ((b[:, 0] | (b[:, 1] << 8)) ^ 0x8000) - 0x8000
    #       +-1            +-(1 - 2^-15)   +-(1 - 2^-23)   ties k + 0.5 to even    the 24-bit ties   +-1.5        +-inf        NaNs            -0, subnormal
    assert got16.tolist() == [32767, -32768, 32767, -32767, 32767, -32768, 0, 2, 2, 0, -2, -2, 0, 0, 0, 0, 0, 0, 32767, -32768, 32767, -32768, -32768, -32768, 0, 0]
    b = first(f"big-{ec.PCM24}-2-3", 3)
    got24 = ((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) ^ 0x800000) - 0x800000
    M = 1 << 23
    assert got24.tolist() == [M - 1, -M, M - 256, -(M - 256), M - 1, -(M - 1), 128, 384, 640, -128, -384, -640, 0, 2, 2, 0, -2, -2,
                              M - 1, -M, M - 1, -M, -M, -M, 0, 0]
    b = first(f"big-{ec.F32}-5-3", 4)
    assert (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24)).tolist() == ec.F32_FIRST   # the bits, NaN payloads and -0 included
    # the PCM16 lanes' extremes go out as they are
    t16 = build_table(True)
    o = int(t16["sinks"][t16["names"][f"big-{ec.PCM16}-5-3"], 0])
    assert t16["want"][o:o + 10].view("<i2").tolist() == ec.PCM16_EXTREMES


@pytest.mark.parametrize("src_pcm16,mutation", [(False, m) for m in ec.MUTATIONS] + [(True, "planar"), (True, "spill")])
def test_a_wrong_model_fails_the_case_table(src_pcm16, mutation):
    # (PCM16 lanes are moved, not converted: the four conversion mutations are told apart by the f32 table alone)
    t = build_table(src_pcm16)
    with pytest.raises(AssertionError):
        ec.compare(ec.egress_model(t["lanes"], t["sinks"], src_pcm16, t["out_in"], mutation=mutation), t["want"], mutation)


def test_each_conversion_mutation_is_told_apart_per_format():
    # the PCM16 sinks alone and the PCM24 sinks alone each fail trunc, wrap and scale32767; be24 is PCM24's
    t = build_table(False)
    for fmt in (ec.PCM16, ec.PCM24):
        sinks = t["sinks"][t["sinks"][:, 3] == fmt]
        want = ec.egress_model(t["lanes"], sinks, False, t["out_in"])
        for mutation in ("trunc", "wrap", "scale32767") + (("be24",) if fmt == ec.PCM24 else ()):
            with pytest.raises(AssertionError):
                ec.compare(ec.egress_model(t["lanes"], sinks, False, t["out_in"], mutation=mutation), want, mutation)
