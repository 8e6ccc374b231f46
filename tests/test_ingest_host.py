"""The host side of the device-side ingest (fvad_wav_probe, wav_map_raw, fvad_ingest_check; no GPU), and the proof that the case
table of ingest_cases.py bites: three wrong versions of the numpy model each fail it."""
import functools
import struct

import numpy as np
import pytest

import ingest_cases as ic

OK, INVALID, RANGE, FORMAT = 0, -100, -6, -104
U64_MAX = (1 << 64) - 1


def riff(chunks):
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def fmt_chunk(tag, channels, bits, extensible=False, rate=48000):
    block = channels * bits // 8
    if not extensible:
        return b"fmt " + struct.pack("<IHHIIHH", 16, tag, channels, rate, rate * block, block, bits)
    guid = struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    return b"fmt " + struct.pack("<IHHIIHHHHI", 40, 0xFFFE, channels, rate, rate * block, block, bits, 22, bits, 0) + guid


def data_chunk(payload, length=None):
    return b"data" + struct.pack("<I", len(payload) if length is None else length) + payload


def samples(fmt, channels, frames, seed=3):
    return ic.sample_bytes(np.random.default_rng(seed), fmt, frames * channels).tobytes()


FORMATS = {"pcm16": (ic.PCM16, 1, 16), "pcm24": (ic.PCM24, 1, 24), "f32": (ic.F32, 3, 32)}


@pytest.mark.parametrize("extensible", [False, True], ids=["plain", "extensible"])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("kind", list(FORMATS))
def test_probe_and_map_raw_agree_with_the_reader(fv, tmp_path, kind, channels, extensible):
    fmt, tag, bits = FORMATS[kind]
    payload = samples(fmt, channels, 37)
    # an odd-sized chunk (with its pad byte) and a LIST chunk in front of "fmt ": the data chunk starts at an odd place
    blob = riff(b"junk" + struct.pack("<I", 3) + b"abc\0" + b"LIST" + struct.pack("<I", 4) + b"INFO" + fmt_chunk(tag, channels, bits, extensible)
                + data_chunk(payload))
    p = tmp_path / "a.wav"
    p.write_bytes(blob)
    info = fv.wav_probe(str(p))
    assert info == {"format": fmt, "n_channels": channels, "sample_rate": 48000, "data_offset": blob.index(b"data") + 8,
                    "n_frames": 37, "bits": bits}
    raw, info2 = fv.wav_map_raw(str(p))
    assert info2 == info and raw.dtype == np.uint8 and raw.tobytes() == payload
    src = [(0, 37, channels, fmt, 0, 0, 37)]
    got = ic.ingest_model(raw, src, False, ic.canaries(channels, 37, False))
    if kind == "pcm24":   # the readers refuse it; the model against plain arithmetic
        with pytest.raises(fv.FvadError):
            fv.wav_read(str(p))
        with pytest.raises(fv.FvadError):
            fv.wav_map(str(p))
        b = np.frombuffer(payload, np.uint8).reshape(-1, 3).astype(np.int64)
        s = b[:, 0] + (b[:, 1] << 8) + (b[:, 2] << 16)
        s = np.where(s >= 1 << 23, s - (1 << 24), s).reshape(37, channels)
        assert np.array_equal(got.astype(np.float64), s.T / 8388608.0)
        return
    want, rate = fv.wav_read(str(p))
    assert rate == 48000 and np.array_equal(ic.bits(got), ic.bits(want))   # the model on the mapped bytes == fvad_wav_read, bit for bit
    mapped, _ = fv.wav_map(str(p))
    assert mapped.shape == (37, channels) and mapped.tobytes() == raw.tobytes()
    if kind == "pcm16":
        got16 = ic.ingest_model(raw, [(0, 37, channels, fmt, 0, 0, 37)], True, ic.canaries(channels, 37, True))
        assert np.array_equal(got16, fv.wav_read_i16(str(p))[0])


def test_probe_edge_cases(fv, tmp_path):
    fmt16 = fmt_chunk(1, 2, 16)
    data = np.arange(-10, 10, dtype="<i2").tobytes()              # 10 stereo frames
    # a data length past the end of the file is cut to the file; a partial frame at the end is dropped
    p = tmp_path / "long.wav"
    p.write_bytes(riff(fmt16 + data_chunk(data + b"\x01", 1 << 30)))
    raw, info = fv.wav_map_raw(str(p))
    assert info["n_frames"] == 10 and raw.tobytes() == data
    assert np.array_equal(raw.view("<i2").reshape(10, 2), fv.wav_map(str(p))[0])
    # the same for 24-bit: 7 bytes of stereo PCM24 are one frame
    p = tmp_path / "long24.wav"
    p.write_bytes(riff(fmt_chunk(1, 2, 24) + data_chunk(b"\1\2\3\4\5\6\7", 1 << 30)))
    raw, info = fv.wav_map_raw(str(p))
    assert info["n_frames"] == 1 and info["format"] == ic.PCM24 and raw.tobytes() == b"\1\2\3\4\5\6"
    # an empty data chunk
    p = tmp_path / "empty.wav"
    p.write_bytes(riff(fmt16 + data_chunk(b"")))
    raw, info = fv.wav_map_raw(str(p))
    assert info["n_frames"] == 0 and raw.shape == (0,) and fv.wav_map(str(p))[0].shape == (0, 2)
    # the first "fmt " and the first "data" chunk count
    p = tmp_path / "two.wav"
    p.write_bytes(riff(fmt16 + data_chunk(data) + data_chunk(b"\0" * 8)))
    assert fv.wav_probe(str(p))["n_frames"] == 10


def test_probe_refuses_what_the_reader_refuses(fv, tmp_path):
    data = np.arange(-10, 10, dtype="<i2").tobytes()
    fmt16 = fmt_chunk(1, 2, 16)
    bad = {"pcm8": riff(fmt_chunk(1, 1, 8) + data_chunk(b"\0" * 6)),
           "pcm32": riff(fmt_chunk(1, 1, 32) + data_chunk(b"\0" * 8)),
           "f64": riff(fmt_chunk(3, 1, 64) + data_chunk(b"\0" * 8)),
           "f24": riff(fmt_chunk(3, 1, 24) + data_chunk(b"\0" * 6)),
           "alaw": riff(fmt_chunk(6, 1, 16) + data_chunk(b"\0" * 6)),
           "nofmt": riff(data_chunk(data) + fmt16),
           "notriff": b"RIFX" + riff(fmt16 + data_chunk(data))[4:],
           "nodata": riff(fmt16),
           "nochannels": riff(fmt_chunk(1, 0, 16) + data_chunk(data)),
           "norate": riff(fmt_chunk(1, 2, 16, rate=0) + data_chunk(data)),
           "short": b"RIFF\0\0\0\0WAV"}
    for name, blob in bad.items():
        p = tmp_path / f"{name}.wav"
        p.write_bytes(blob)
        with pytest.raises(fv.FvadError) as e:
            fv.wav_read(str(p))
        status = e.value.status
        with pytest.raises(fv.FvadError) as e:
            fv.wav_probe(str(p))
        assert e.value.status == status == FORMAT, name
        with pytest.raises(fv.FvadError):
            fv.wav_map_raw(str(p))
    with pytest.raises(fv.FvadError) as e:
        fv.wav_probe(str(tmp_path / "absent.wav"))
    assert e.value.status == -105
    info = (fv.C.c_uint64 * 6)()
    assert fv.lib().fvad_wav_probe(None, info) == INVALID and fv.lib().fvad_wav_probe(b"x", None) == INVALID


# ---------------------------------------------------------------- fvad_ingest_check
# one good source on lanes 2..3 of 6, 100 samples each: byte_offset 44, 10 stereo PCM16 frames to [5, 15), zeros to 20
GOOD = (44, 10, 2, ic.PCM16, 2, 5, 20)


def check(fv, sources, raw_bytes=1000, out_pcm16=False, n_lanes=6, lane_stride=101, n_samples=100):
    return fv.ingest_check(sources, raw_bytes, out_pcm16, n_lanes, lane_stride, n_samples)


def edit(**kw):
    names = ("byte_offset", "n_frames", "n_channels", "format", "first_lane", "dst_offset", "fill_to")
    return tuple(kw.get(n, v) for n, v in zip(names, GOOD))


def test_check_accepts(fv):
    assert check(fv, [GOOD]) == OK and check(fv, [GOOD], out_pcm16=True) == OK
    assert check(fv, np.zeros((0, 7), np.uint64)) == OK                                      # no sources: nothing to do
    assert fv.lib().fvad_ingest_check(None, 0, 0, 0, 0, 0, 0) == OK
    assert check(fv, [edit(n_frames=0, fill_to=5)]) == OK                                    # writes nothing
    assert check(fv, [edit(n_frames=0)]) == OK                                               # only fills
    assert check(fv, [edit(byte_offset=1000 - 40)]) == OK and check(fv, [edit(fill_to=100)]) == OK   # both ends exactly
    assert check(fv, [edit(n_channels=64, first_lane=0)], n_lanes=64, raw_bytes=44 + 10 * 128) == OK
    assert check(fv, [edit(format=ic.PCM24)]) == OK and check(fv, [edit(format=ic.F32)]) == OK
    assert check(fv, [GOOD], raw_bytes=U64_MAX) == OK                                        # the host form's raw_bytes
    # the same sample range on different lanes, adjacent ranges on the same lanes, an empty range inside another
    assert check(fv, [GOOD, edit(first_lane=4)]) == OK and check(fv, [GOOD, edit(first_lane=0)]) == OK
    assert check(fv, [GOOD, edit(dst_offset=20, fill_to=30)]) == OK and check(fv, [edit(dst_offset=20, fill_to=30), GOOD]) == OK
    assert check(fv, [GOOD, edit(n_frames=0, dst_offset=10, fill_to=10)]) == OK


def test_check_invalid_arguments(fv):
    L, u64p = fv.lib(), fv.C.POINTER(fv.C.c_uint64)
    one = np.array([GOOD], np.uint64)
    assert L.fvad_ingest_check(None, 1, 1000, 0, 6, 101, 100) == INVALID                     # NULL sources
    assert L.fvad_ingest_check(one.ctypes.data_as(u64p), 1, 1000, 2, 6, 101, 100) == INVALID   # PCM24 lanes do not exist
    assert L.fvad_ingest_check(one.ctypes.data_as(u64p), 1, 1000, -1, 6, 101, 100) == INVALID
    assert check(fv, [GOOD], lane_stride=99) == INVALID                                      # lanes would overlap
    assert check(fv, [edit(format=3)]) == INVALID                                            # no such format
    assert check(fv, [edit(format=ic.PCM24)], out_pcm16=True) == INVALID                     # conversions, not ingest
    assert check(fv, [edit(format=ic.F32)], out_pcm16=True) == INVALID
    assert check(fv, [edit(n_channels=0)]) == INVALID
    assert check(fv, [edit(n_channels=65, first_lane=0)], n_lanes=100) == INVALID
    assert check(fv, [edit(fill_to=14)]) == INVALID                                          # below dst_offset + n_frames
    assert check(fv, [edit(n_frames=U64_MAX, fill_to=U64_MAX)]) == INVALID                   # dst_offset + n_frames wraps
    assert check(fv, [GOOD, edit(fill_to=14)]) == INVALID                                    # in any row


def test_check_out_of_range(fv):
    assert check(fv, [edit(first_lane=6)]) == RANGE and check(fv, [edit(first_lane=5)]) == RANGE   # lanes past n_lanes
    assert check(fv, [edit(first_lane=U64_MAX)]) == RANGE
    assert check(fv, [edit(fill_to=101)]) == RANGE                                           # past n_samples
    assert check(fv, [edit(byte_offset=1000 - 39)]) == RANGE                                 # one byte past the raw buffer
    assert check(fv, [edit(byte_offset=1001, n_frames=0, fill_to=5)]) == RANGE
    assert check(fv, [edit(byte_offset=U64_MAX)], raw_bytes=U64_MAX) == RANGE                # byte_offset + bytes wraps
    assert check(fv, [edit(n_frames=1 << 62, dst_offset=0, fill_to=1 << 62)], n_samples=1 << 62, lane_stride=1 << 62,
                 raw_bytes=U64_MAX) == RANGE                                                 # n_frames * frame bytes wraps
    assert check(fv, [edit(format=ic.PCM24, byte_offset=1000 - 59)]) == RANGE                # 60 bytes of PCM24


def test_check_overlap(fv):
    assert check(fv, [GOOD, GOOD]) == INVALID                                                # the same range twice
    assert check(fv, [GOOD, edit(dst_offset=19, fill_to=30)]) == INVALID                     # one sample of the fill
    assert check(fv, [edit(dst_offset=19, fill_to=30), GOOD]) == INVALID                     # in either order
    assert check(fv, [GOOD, edit(first_lane=3, n_channels=1)]) == INVALID                    # partial lane overlap: lane 3 alone
    assert check(fv, [GOOD, edit(first_lane=1)]) == INVALID                                  # lanes 1..2 against 2..3
    assert check(fv, [GOOD, edit(first_lane=4), edit(first_lane=0, n_channels=3, dst_offset=0, fill_to=6)]) == INVALID
    assert check(fv, [GOOD, edit(first_lane=4), edit(first_lane=0, n_channels=3, dst_offset=0, fill_to=5, n_frames=5)]) == OK
    assert check(fv, [GOOD, edit(n_frames=0, dst_offset=10, fill_to=11)]) == INVALID         # a fill inside another's frames


# ---------------------------------------------------------------- the case table
@functools.lru_cache(maxsize=None)
def build_table(out_pcm16):
    t = ic.case_table(out_pcm16)
    t["out_pcm16"] = out_pcm16
    t["lanes_in"] = ic.canaries(t["n_lanes"], t["lane_stride"], out_pcm16)
    t["want"] = ic.ingest_model(t["raw"], t["sources"], out_pcm16, t["lanes_in"])
    return t


@pytest.fixture(scope="module", params=[False, True], ids=["to-f32", "to-pcm16"])
def table(request):
    return build_table(request.param)


def test_the_case_table_is_what_the_issue_asks_for(fv, table):
    src, out_pcm16 = table["sources"].astype(np.int64), table["out_pcm16"]
    formats = {ic.PCM16} if out_pcm16 else {ic.F32, ic.PCM16, ic.PCM24}
    assert set(src[:, 3].tolist()) == formats and set(src[:, 2].tolist()) == {1, 2, 3, 5}
    fills = src[:, 6] - src[:, 5] - src[:, 1]
    for fmt in formats:
        rows = src[src[:, 3] == fmt]
        assert {int(b) % 16 for b in rows[:, 0]} == set(range(16)), fmt                       # every byte alignment, per format
        for C in {int(c) for c in rows[:, 2]}:
            T = fv.ingest_tile_frames(C, fmt)
            assert T == ic.tile_frames(C, fmt) and T % 4 == 0 and T * C * ic.SAMPLE_BYTES[fmt] <= fv.INGEST_TILE_BYTES
        for C in ic.BIG[fmt]:
            T = ic.tile_frames(C, fmt)
            sel = (src[:, 3] == fmt) & (src[:, 2] == C)
            assert {0, 1, 3, 4, 5, T - 1, T, T + 1, 2 * T + 3} <= set(src[sel, 1].tolist())
            assert T + 1 in set(fills[sel].tolist())
    assert {0, 1, 7} <= set(fills.tolist())
    assert {int(d) % 8 for d in src[:, 5]} == set(range(8))
    assert table["lane_stride"] % 2 == 1 and table["lane_stride"] > table["n_samples"]
    a, b = src[table["names"]["adjacent-a"]], src[table["names"]["adjacent-b"]]
    assert a[4] == b[4] and a[2] == b[2] and a[6] == b[5]                                    # adjacent on the same lanes
    assert not np.all(np.diff(src[:, 4]) >= 0)                                               # not in lane order
    assert fv.ingest_check(table["sources"], table["raw"].size, out_pcm16, table["n_lanes"], table["lane_stride"], table["n_samples"]) == OK
    assert table["n_lanes"] * table["lane_stride"] < 4_000_000
    # the model on the table: the extremes decode to what they are, canaries stand outside the sources
    want = table["want"]
    written = np.zeros(want.shape, bool)
    for _, n, C, _, l0, d, f in src.tolist():
        written[l0:l0 + C, d:f] = True
    canary = ic.CANARY_I16 if out_pcm16 else ic.CANARY_F32
    assert np.all(ic.bits(want)[~written] == canary) and not np.any(ic.bits(want)[written] == canary)
    if not out_pcm16:
        r = src[table["names"][f"big-{ic.PCM24}-2-3"]]
        got = want[r[4]:r[4] + 2, r[5]:r[5] + 3].T.reshape(-1)[:5]
        assert got.tolist() == [-1.0, (2 ** 23 - 1) / 2 ** 23, -(2.0 ** -23), 2.0 ** -23, 0.0]
        r = src[table["names"][f"big-{ic.F32}-5-3"]]
        got = ic.bits(want[r[4]:r[4] + 5, r[5]:r[5] + 2]).T.reshape(-1)[:9]
        assert got.tolist() == ic.F32_SPECIALS
    ic.compare(ic.ingest_model(table["raw"], table["sources"][::-1], out_pcm16, table["lanes_in"]), want, "the model, sources reversed")


# (PCM16 lanes take no PCM24 source: the sign extension is told apart by the f32 table alone)
@pytest.mark.parametrize("out_pcm16,mutation", [(False, "nosign"), (False, "swap"), (False, "late"), (True, "swap"), (True, "late")])
def test_a_wrong_model_fails_the_case_table(out_pcm16, mutation):
    t = build_table(out_pcm16)
    with pytest.raises(AssertionError):
        ic.compare(ic.ingest_model(t["raw"], t["sources"], out_pcm16, t["lanes_in"], mutation=mutation), t["want"], mutation)


def test_a_slice_behind_a_files_end_is_a_row_that_only_fills(pkg, fv, tmp_path):
    # the sliced grid keeps a channel-count group's short files until the longest ends: their rows then have no frames, and
    # must read no byte of the mapped file, wherever the slice starts
    p = tmp_path / "short.wav"
    p.write_bytes(riff(fmt_chunk(1, 2, 16) + data_chunk(samples(ic.PCM16, 2, 50))))
    raw, info = fv.wav_map_raw(str(p))
    sim = pkg.simulator
    a = sim._RawAudio(raw, info)
    assert (a.n_channels, a.n_frames) == (2, 50) and sim._dims(a) == sim._dims(a, mapped=True) == (2, 50)
    assert sim._dims(fv.wav_map(str(p))[0], mapped=True) == sim._dims(fv.wav_read(str(p))[0]) == (2, 50)
    assert a.source(10, 50, 4, 0, 64) == (40, 40, 2, ic.PCM16, 4, 0, 64)
    assert a.source(10, 70, 4, 0, 64)[:2] == (40, 60)                     # (the caller clamps frame_to to n_frames)
    for lo, hi in ((50, 50), (78, 50), (1 << 40, 50)):
        row = a.source(lo, hi, 4, 0, 64)
        assert row == (0, 0, 2, ic.PCM16, 4, 0, 64)
        assert fv.ingest_check([row], raw.size, False, 6, 64, 64) == OK
