"""The numpy model and the case table of the device-side ingest tests (fvad_ingest*; test_ingest_host.py, test_ingest_gpu.py).

The model is the statement of what fvad_ingest_device computes:
  * a source (byte_offset, n_frames, n_channels, format, first_lane, dst_offset, fill_to) reads the interleaved little-endian
    samples raw[byte_offset + (f * n_channels + c) * bytes_per_sample ...] and writes sample f of channel c to lane
    first_lane + c at dst_offset + f;
  * PCM16 -> f32 is f32(s) * f32(1 / 32768), PCM24 (sign-extended) -> f32 is f32(s) * f32(1 / 8388608), both exact; PCM16 ->
    PCM16 and f32 -> f32 are the source's bits;
  * [dst_offset + n_frames, fill_to) of the source's lanes becomes zeros; nothing else of the lanes changes.
`ingest_model(..., mutation=...)` states three wrong versions; test_ingest_host.py shows that the case table fails each of
them.  All comparisons are of bits: f32 lanes are compared as uint32 (NaN payloads, -0)."""
import numpy as np

F32, PCM16, PCM24 = 0, 1, 2
SAMPLE_BYTES = {F32: 4, PCM16: 2, PCM24: 3}
TILE_BYTES = 16384       # kIngestTileBytes of csrc/kernels.h: the source bytes a workgroup takes ...
CANARY_F32 = 0x7FC5A5A5  # a NaN pattern no source holds
CANARY_I16 = 0x5A5A       # (the PCM16 noise skips it)
PAD_BYTE = 0xA5          # between the sources of the raw buffer: read by nobody


def tile_frames(n_channels, fmt):
    """... rounded down to whole frames, in fours (binding.ingest_tile_frames states the same rule)"""
    return TILE_BYTES // (n_channels * SAMPLE_BYTES[fmt]) // 4 * 4


def bits(lanes):
    return lanes.view(np.uint32 if lanes.dtype == np.float32 else np.uint16)


def canaries(n_lanes, lane_stride, out_pcm16):
    if out_pcm16:
        return np.full((n_lanes, lane_stride), CANARY_I16, np.int16)
    return np.full((n_lanes, lane_stride), CANARY_F32, np.uint32).view(np.float32)


def decode(raw, byte_offset, n_frames, n_channels, fmt, mutation=None):
    """the source's samples as [n_frames][n_channels]: int16, int32 (PCM24) or uint32 (the f32 bits)"""
    B = SAMPLE_BYTES[fmt]
    b = np.asarray(raw[byte_offset:byte_offset + n_frames * n_channels * B], np.uint8).reshape(n_frames * n_channels, B).astype(np.uint32)
    if fmt == PCM16:
        v = (b[:, 0] | (b[:, 1] << 8)).astype(np.uint16).view(np.int16)
    elif fmt == PCM24:
        u = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = u.astype(np.int32) if mutation == "nosign" else ((u << 8).astype(np.uint32).view(np.int32) >> 8)
    else:
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24)
    if mutation == "swap":   # channel and frame index swapped: the bytes taken as planar
        return np.ascontiguousarray(v.reshape(n_channels, n_frames).T)
    return v.reshape(n_frames, n_channels)


def ingest_model(raw_bytes, sources, out_pcm16, lanes_in, mutation=None):
    """lanes_in [n_lanes][lane_stride] (float32, or int16 with out_pcm16) -> the lanes after the sources, a new array"""
    lanes = lanes_in.copy()
    lb = bits(lanes)
    for byte_offset, n_frames, n_channels, fmt, first_lane, dst_offset, fill_to in np.asarray(sources, np.uint64).reshape(-1, 7).tolist():
        v = decode(raw_bytes, byte_offset, n_frames, n_channels, fmt, mutation)
        if out_pcm16:
            assert fmt == PCM16
            out = v.view(np.uint16)
        elif fmt == F32:
            out = v
        else:
            out = (v.astype(np.float32) * np.float32(1.0 / (32768.0 if fmt == PCM16 else 8388608.0))).view(np.uint32)
        end = dst_offset + n_frames
        for c in range(n_channels):
            lb[first_lane + c, dst_offset:end] = out[:, c]
            lb[first_lane + c, end + (1 if mutation == "late" else 0):fill_to] = 0
    return lanes


# ---------------------------------------------------------------- the case table
PCM16_EXTREMES = [-32768, 32767, -1, 1, 0]
PCM24_EXTREMES = [-(1 << 23), (1 << 23) - 1, -1, 1, 0]
F32_SPECIALS = [0x7FC12345, 0xFFA00001, 0x7F800001, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000]


def sample_bytes(rng, fmt, n):
    """n samples of the format as bytes: the extremes / special values first (as many as fit), seeded noise for the rest"""
    if fmt == PCM16:
        v = rng.integers(-32768, 32768, n).astype(np.int16)
        v[v == CANARY_I16] += 1   # no source holds the canary
        v[:len(PCM16_EXTREMES)] = PCM16_EXTREMES[:n]
        return v.astype("<i2").view(np.uint8)
    if fmt == PCM24:
        v = rng.integers(-(1 << 23), 1 << 23, n).astype(np.int32)
        v[:len(PCM24_EXTREMES)] = PCM24_EXTREMES[:n]
        return v.astype("<i4").view(np.uint8).reshape(n, 4)[:, :3].reshape(-1)
    v = rng.uniform(-1.0, 1.0, n).astype(np.float32).view(np.uint32)
    v[:len(F32_SPECIALS)] = F32_SPECIALS[:n]
    return v.astype("<u4").view(np.uint8)


SMALL_FRAMES = (0, 1, 3, 4, 5)
CHANNELS = (1, 2, 3, 5)
BIG = {F32: (2, 5), PCM16: (1, 5), PCM24: (2, 3)}   # the channel counts that get the sizes around the tile


def case_table(out_pcm16, seed=11):
    """-> dict(raw [bytes] uint8, sources [n][7] uint64, n_lanes, lane_stride (odd), n_samples, names {name: row}).
    Small sources (0 .. 5 frames, every format and channel count) lie one behind the other on a track of lanes per channel
    count, a canary sample or more between them -- except the pair "adjacent-a" / "adjacent-b", whose ranges touch.  The
    sources around the tile size have lanes of their own.  byte_offset runs through every residue modulo 16 per format,
    dst_offset through every residue modulo 8, the fills through 0, 1, 7 and T + 1.  The rows are then shuffled, so that
    their order is not the lanes' order."""
    rng = np.random.default_rng(seed)
    formats = (PCM16,) if out_pcm16 else (PCM16, PCM24, F32)
    specs = []   # (name, fmt, C, n_frames, fill)
    small_fill = (0, 1, 7)
    k = 0
    for fmt in formats:
        for C in CHANNELS:
            for n in SMALL_FRAMES:
                specs.append((f"small-{fmt}-{C}-{n}", fmt, C, n, small_fill[k % 3]))
                k += 1
    for fmt in formats:
        for j, C in enumerate(BIG[fmt]):
            T = tile_frames(C, fmt)
            for i, n in enumerate((T - 1, T, T + 1, 2 * T + 3)):
                specs.append((f"big-{fmt}-{C}-{i}", fmt, C, n, (0, 1, 7, T + 1)[(i + j + 1) % 4]))
    fmt0 = formats[0]
    specs.append(("adjacent-a", fmt0, 2, 9, 3))
    specs.append(("adjacent-b", fmt0, 2, 6, 0))
    specs.append(("fill-only", fmt0, 3, 0, tile_frames(3, fmt0) + 1))   # no frames at all: zeros alone

    rows, names, chunks = [], {}, []
    at = 0
    byte_res = {f: 0 for f in formats}
    dst_res = 0
    track = {C: None for C in CHANNELS}   # (first_lane, cursor) of the small sources per channel count
    n_lanes = 1                           # lane 0 belongs to no source
    for name, fmt, C, n, fill in specs:
        # the bytes: at the next offset with the format's next residue, at least one pad byte after the previous source
        want = byte_res[fmt]
        byte_res[fmt] = (want + 1) % 16
        pad = 1 + (want - (at + 1)) % 16
        chunks.append(np.full(pad, PAD_BYTE, np.uint8))
        at += pad
        data = sample_bytes(rng, fmt, n * C)
        chunks.append(data)
        byte_offset = at
        at += data.size
        # the lanes
        if name.startswith("big") or name == "fill-only":
            first_lane, dst = n_lanes, dst_res
            n_lanes += C
        else:
            if track[C] is None:
                track[C] = [n_lanes, 0]
                n_lanes += C
            first_lane, cur = track[C]
            if name == "adjacent-b":
                dst = cur                                 # touches adjacent-a's fill_to
            else:
                dst = cur + 1 + (dst_res - (cur + 1)) % 8  # a canary or more in front
            track[C][1] = dst + n + fill
        if name != "adjacent-b":
            dst_res = (dst_res + 1) % 8
        names[name] = len(rows)
        rows.append((byte_offset, n, C, fmt, first_lane, dst, dst + n + fill))
    chunks.append(np.full(3, PAD_BYTE, np.uint8))
    raw = np.concatenate(chunks)
    rows = np.asarray(rows, np.uint64)
    n_samples = int(rows[:, 6].max()) + 2
    lane_stride = n_samples + 1 + (n_samples % 2)   # odd, and a canary or more between the lanes
    order = rng.permutation(len(rows))
    names = {k: int(np.nonzero(order == v)[0][0]) for k, v in names.items()}
    return {"raw": raw, "sources": np.ascontiguousarray(rows[order]), "n_lanes": n_lanes + 1, "lane_stride": lane_stride,
            "n_samples": n_samples, "names": names}


def compare(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} samples differ, the first at lane {bad[0][0]} sample {bad[0][1]}: {g[tuple(bad[0])]:#x} != {w[tuple(bad[0])]:#x}"
