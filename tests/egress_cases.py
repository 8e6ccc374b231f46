"""The numpy model and the case table of the device-side egress tests (fvad_egress*; test_egress_host.py, test_egress_gpu.py),
the mirror of ingest_cases.py.

The model is the statement of what fvad_egress_device computes:
  * a sink (byte_offset, n_frames, n_channels, format, first_lane, src_offset) takes sample src_offset + f of lane first_lane + c
    and writes it, little-endian in the FILE's format, to out[byte_offset + (f * n_channels + c) * bytes_per_sample ...];
  * f32 -> f32 and PCM16 -> PCM16 are the lane's bits; f32 -> PCM16 is rint(min(max(f32(y) * f32(32768), -32768), 32767)),
    f32 -> PCM24 the same with 8388608 and 8388607 (the product and the clamp in float32, ties to even, NaN the minimum), the
    low three bytes written;
  * nothing else of the output changes.
`egress_model(..., mutation=...)` states six wrong versions; test_egress_host.py shows that the case table fails each of them.
All comparisons are of bytes."""
import numpy as np

F32, PCM16, PCM24 = 0, 1, 2
SAMPLE_BYTES = {F32: 4, PCM16: 2, PCM24: 3}
TILE_BYTES = 16384       # kIngestTileBytes of csrc/kernels.h: the DESTINATION bytes a workgroup takes ...
PAD_BYTE = 0xA5          # the canary of the output buffer: between the sinks, written by nobody
MUTATIONS = ("planar", "trunc", "wrap", "scale32767", "be24", "spill")
SCALE = {PCM16: 32768.0, PCM24: 8388608.0}


def tile_frames(n_channels, fmt):
    """... rounded down to whole frames, in fours (binding.ingest_tile_frames states the same rule)"""
    return TILE_BYTES // (n_channels * SAMPLE_BYTES[fmt]) // 4 * 4


def quantise(y, fmt, mutation=None):
    """float32 samples -> the integers of a PCM16 / PCM24 file (int64)"""
    y = np.asarray(y, np.float32)
    scale = np.float32(SCALE[fmt])
    lo, hi = np.float32(-SCALE[fmt]), np.float32(SCALE[fmt] - 1.0)
    with np.errstate(all="ignore"):
        if mutation == "scale32767":   # libsndfile's rule, fvad_wav_write's: clip to [-1, 1], scale by the largest positive value
            p = np.where(np.isnan(y), np.float32(-1.0), np.minimum(np.maximum(y, np.float32(-1.0)), np.float32(1.0))) * hi
        else:
            p = y * scale                                   # a float32 product
        if mutation == "wrap":                              # no clamp: what does not fit wraps (non-finite: 0)
            p = np.where(np.isfinite(p), p, np.float32(0.0))
        else:
            p = np.where(np.isnan(p), lo, np.minimum(np.maximum(p, lo), hi)).astype(np.float32)   # the clamp in f32, NaN the minimum
        q = (np.trunc(p) if mutation == "trunc" else np.rint(p)).astype(np.float64)
    return q.astype(np.int64)


def encode(v, fmt, src_pcm16, mutation=None):
    """lane samples v [n] (uint32 bits of f32 lanes, or int16) -> the file's bytes [n][bytes_per_sample]"""
    if src_pcm16:
        assert fmt == PCM16
        u = v.view(np.uint16).astype(np.uint32)
    elif fmt == F32:
        u = v.astype(np.uint32)
    else:
        u = (quantise(v.view(np.float32), fmt, mutation) & 0xFFFFFFFF).astype(np.uint32)
    B = SAMPLE_BYTES[fmt]
    b = np.stack([(u >> (8 * k)) & 0xFF for k in range(B)], axis=1).astype(np.uint8)
    if mutation == "be24" and fmt == PCM24:
        b = b[:, ::-1]
    return b


def lane_bits(lanes):
    return lanes.view(np.uint32 if lanes.dtype == np.float32 else np.int16)


def egress_model(lanes, sinks, src_pcm16, out_in, mutation=None):
    """lanes [n_lanes][lane_stride] (float32, or int16 with src_pcm16), out_in [bytes] uint8 -> the bytes after the sinks, a new array"""
    out = out_in.copy()
    lb = lane_bits(lanes)
    for byte_offset, n_frames, n_channels, fmt, first_lane, src_offset in np.asarray(sinks, np.uint64).reshape(-1, 6).tolist():
        v = lb[first_lane:first_lane + n_channels, src_offset:src_offset + n_frames]       # [c][f]
        v = v.reshape(-1) if mutation == "planar" else np.ascontiguousarray(v.T).reshape(-1)   # planar: channel and frame swapped
        b = encode(v, fmt, src_pcm16, mutation).reshape(-1)
        out[byte_offset:byte_offset + b.size] = b
        if mutation == "spill" and n_frames:
            out[byte_offset + b.size] = 0   # one byte past the sink's end
    return out


# ---------------------------------------------------------------- the case table
PCM16_EXTREMES = [-32768, 32767, -1, 1, 0]


def _f32_bits(x):
    return np.asarray(x, np.float64).astype(np.float32).view(np.uint32).tolist()


TIE_K = (0, 1, 2, -1, -2, -3)
F32_FIRST = (_f32_bits([1.0, -1.0, 1 - 2.0 ** -15, -(1 - 2.0 ** -15), 1 - 2.0 ** -23, -(1 - 2.0 ** -23)])
             + _f32_bits([(k + 0.5) / 32768.0 for k in TIE_K]) + _f32_bits([(k + 0.5) / 8388608.0 for k in TIE_K])   # exact in f32
             + _f32_bits([1.5, -1.5])
             + [0x7F800000, 0xFF800000, 0x7FC12345, 0xFFA00001, 0x80000000, 0x00000001])   # +-inf, two NaNs (one signalling), -0, a subnormal


def lane_samples(rng, src_pcm16, n):
    """n lane samples: the extremes / special values first (as many as fit), seeded noise for the rest -> int16 or uint32 (f32 bits)"""
    if src_pcm16:
        v = rng.integers(-32768, 32768, n).astype(np.int16)
        v[:len(PCM16_EXTREMES)] = PCM16_EXTREMES[:n]
        return v
    v = rng.uniform(-1.2, 1.2, n).astype(np.float32).view(np.uint32)   # (past +-1: the clamp)
    v[:len(F32_FIRST)] = F32_FIRST[:n]
    return v


SMALL_FRAMES = (0, 1, 3, 4, 5)
CHANNELS = (1, 2, 3, 5)
BIG = {F32: (2, 5), PCM16: (1, 5), PCM24: (2, 3)}   # the channel counts that get the sizes around the tile


def case_table(src_pcm16, seed=12):
    """-> dict(lanes [n_lanes][lane_stride] (float32 or int16), sinks [n][6] uint64, out_bytes, n_lanes, lane_stride (odd),
    n_samples, names {name: row}).
    Every sink has lane samples of its own (its flat [frame][channel] samples begin with the special values): the small sinks
    (0 .. 5 frames, every file format and channel count) one behind the other on a track of lanes per channel count, the sinks
    around the tile size on lanes of their own.  In the output the sinks lie one behind the other with a PAD_BYTE or more
    between them -- except the pair "adjacent-a" / "adjacent-b", whose byte ranges touch.  byte_offset runs through every
    residue modulo 16 per format, src_offset through every residue modulo 8.  The rows are then shuffled."""
    rng = np.random.default_rng(seed)
    formats = (PCM16,) if src_pcm16 else (PCM16, PCM24, F32)
    specs = []   # (name, fmt, C, n_frames)
    for fmt in formats:
        for C in CHANNELS:
            for n in SMALL_FRAMES:
                specs.append((f"small-{fmt}-{C}-{n}", fmt, C, n))
    for fmt in formats:
        for C in BIG[fmt]:
            T = tile_frames(C, fmt)
            for i, n in enumerate((T - 1, T, T + 1, 2 * T + 3)):
                specs.append((f"big-{fmt}-{C}-{i}", fmt, C, n))
    fmt0 = formats[-1]
    specs.append(("adjacent-a", fmt0, 2, 9))
    specs.append(("adjacent-b", fmt0, 3, 6))

    rows, names, data = [], {}, []
    at = 0
    byte_res = {f: 0 for f in formats}
    src_res = 0
    track = {C: None for C in CHANNELS}   # (first_lane, cursor) of the small sinks per channel count
    n_lanes = 1                           # lane 0 belongs to no sink
    for name, fmt, C, n in specs:
        if name == "adjacent-b":
            byte_offset = at                              # touches adjacent-a's last byte
        else:   # at the next offset with the format's next residue, at least one pad byte after the previous sink
            want = byte_res[fmt]
            byte_res[fmt] = (want + 1) % 16
            byte_offset = at + 1 + (want - (at + 1)) % 16
        at = byte_offset + n * C * SAMPLE_BYTES[fmt]
        if name.startswith("big"):
            first_lane, src = n_lanes, src_res
            n_lanes += C
        else:
            if track[C] is None:
                track[C] = [n_lanes, 0]
                n_lanes += C
            first_lane, cur = track[C]
            src = cur + (src_res - cur) % 8
            track[C][1] = src + n
        src_res = (src_res + 1) % 8
        names[name] = len(rows)
        rows.append((byte_offset, n, C, fmt, first_lane, src))
        data.append(lane_samples(rng, src_pcm16, n * C).reshape(n, C))
    out_bytes = at + 3
    rows = np.asarray(rows, np.uint64)
    n_samples = int((rows[:, 5] + rows[:, 1]).max()) + 2
    lane_stride = n_samples + 1 + (n_samples % 2)   # odd
    lanes = lane_samples(rng, src_pcm16, (n_lanes + 1) * lane_stride).reshape(n_lanes + 1, lane_stride)
    for (_, n, C, _, first_lane, src), v in zip(rows.tolist(), data):
        lanes[first_lane:first_lane + C, src:src + n] = v.T
    order = rng.permutation(len(rows))
    names = {k: int(np.nonzero(order == v)[0][0]) for k, v in names.items()}
    return {"lanes": lanes if src_pcm16 else lanes.view(np.float32), "sinks": np.ascontiguousarray(rows[order]), "out_bytes": out_bytes,
            "n_lanes": n_lanes + 1, "lane_stride": lane_stride, "n_samples": n_samples, "names": names}


def canaries(out_bytes):
    return np.full(out_bytes, PAD_BYTE, np.uint8)


def compare(got, want, what):
    got, want = np.asarray(got, np.uint8), np.asarray(want, np.uint8)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at byte {bad[0]}: {got[bad[0]]:#x} != {want[bad[0]]:#x}"
