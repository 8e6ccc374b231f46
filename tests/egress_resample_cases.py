"""The model, the bound and the case tables of the resampling egress tests (fvad_egress_resample*; test_egress_resample_host.py,
test_egress_resample_gpu.py).

The float64 model is ingest_resample_cases.resample_model -- the arithmetic is the same definition, with the lanes' samples in
the place of a file's decoded frames -- and the bound is ingest_resample_cases.compare's: gamma(up, n_taps) * B plus one f32 ulp,
computed, not measured.  Only an F32 file is held against the model.  The PCM16 and PCM24 bytes of a row are compared EXACTLY
against egress_cases.quantise of the f32 values the library itself wrote for the same row as an f32 file (`twin_f32` is the table
with every row an f32 file): that is the invariant of include/fvad.h, so no rounding-boundary slack is needed.

A row of a table is (byte_offset, n_out, n_channels, format, first_lane, src_offset, frame_base, n_frames, stream_frames,
out_from).  The lanes are NaN everywhere outside the given frames of the rows (finite inside): a NaN in the output shows a read
that should not count.  `model(..., mutation=...)` states four wrong versions; test_egress_resample_host.py shows that the case
tables fail each of them."""
import numpy as np

import egress_cases as ec
import ingest_resample_cases as rc

F32, PCM16, PCM24 = rc.F32, rc.PCM16, rc.PCM24
SAMPLE_BYTES = rc.SAMPLE_BYTES
FIELDS = 10
PAD_BYTE = ec.PAD_BYTE
TILE_BYTES, WINDOW = 16384, 8192   # kIngestTileBytes and kClipTile of csrc/kernels.h: a tile's destination bytes and staged lane samples
# (up, down, half, taps): 16 kHz, 96 kHz and 32 kHz out, a ratio with up > down > 1 and asymmetric taps, 44.1 kHz at the default
# length (5121 taps: the table in LDS), 22.05 kHz at the default length (10241 taps: the table in global memory)
RATIOS = ((1, 3, 2, "design"), (2, 1, 3, "noise"), (2, 3, 4, "design"), (7, 5, 2, "noise"), (147, 160, 16, "design"), (147, 320, 16, "design"))
MUTATIONS = ("planar", "row_phase", "reversed", "given")


def ratio_id(r):
    return f"{r[0]}-{r[1]}"


def tile(up, down, n_taps, n_channels, fmt):
    """fvad_egress_resample_tile restated in python integers"""
    most = TILE_BYTES // (n_channels * SAMPLE_BYTES[fmt]) // 4 * 4
    if WINDOW * up <= n_taps - 1:
        return 0
    return min((WINDOW * up - (n_taps - 1) - 1) // down + 1, most) // 4 * 4


def ready(up, down, n_taps, stream_frames, frames_have):
    """fvad_egress_resample_ready restated in python integers"""
    OF = rc.out_frames(stream_frames, up, down)
    if frames_have >= stream_frames:
        return OF
    K = (n_taps - 1) // 2
    return max(0, min(OF, -(-(frames_have * up - K) // down)))


def lane_data(rng, n, C):
    """n frames of C finite f32 samples, past +-1 (the clamp), a few edge values first"""
    v = rng.uniform(-1.2, 1.2, (n, C)).astype(np.float32)
    edge = np.array([1.0, -1.0, 0.0, -0.0, 1 - 2.0 ** -15, 0.5 / 32768.0, 1.5 / 8388608.0, -1.5], np.float32)
    flat = v.reshape(-1)
    flat[:edge.size] = edge[:flat.size]
    return v


def case_table(up, down, n_taps, seed=31):
    """-> dict(lanes float32 [n_lanes][lane_stride] (NaN outside the rows' given frames), rows [n][10] uint64, data [row] float64
    [n_frames][C], out_bytes, n_lanes, lane_stride (odd, > n_samples), n_samples, big [row indices]).
    Per (format, channels) of ingest_resample_cases.COMBOS whole streams of 0, 1, 5 and about the filter's reach in lane samples;
    for the combos below 64 channels a stream of two full tiles and a partial one, whole, and a SLICE of a stream of that length:
    37 outputs from an odd output in its middle, given three frames more than their window in front and two behind.  Rows of
    one channel count lie one behind the other on their lanes, NaN between them; src_offset runs through the 4 alignments (the
    odd lane_stride moves them again lane by lane).  In the output the first row lies at byte 44, the others behind it with a
    canary or more between, byte_offset running through every residue modulo 16 per format -- except each slice, which touches
    the row in front of it."""
    rng = np.random.default_rng(seed)
    K = (n_taps - 1) // 2
    specs = []   # (fmt, C, stream_frames, out_from, n_out, frame_base, n_frames, touch, big)
    for fmt, C in rc.COMBOS:
        for sf in (0, 1, 5, max(6, K // up + 2)):
            specs.append((fmt, C, sf, 0, rc.out_frames(sf, up, down), 0, sf, False, False))
        if C == 64:
            continue
        T = tile(up, down, n_taps, C, fmt)
        sf = -(-(2 * T + T // 3 + 1) * down // up)
        OF = rc.out_frames(sf, up, down)
        assert OF > 2 * T
        specs.append((fmt, C, sf, 0, OF, 0, sf, False, True))
        a = (OF // 2) | 1
        lo, hi = rc.window(up, down, n_taps, sf, a, 37)
        lo, hi = max(lo - 3, 0), min(hi + 2, sf)
        specs.append((fmt, C, sf, a, 37, lo, hi - lo, True, False))
    rows, data, big = [], [], []
    at, byte_res, track, n_lanes, k = 44, {F32: 0, PCM16: 0, PCM24: 0}, {}, 1, 0   # lane 0 belongs to no row
    for i, (fmt, C, sf, out_from, n_out, fb, nf, touch, is_big) in enumerate(specs):
        if i and not touch:
            want = byte_res[fmt]
            byte_res[fmt] = (want + 1) % 16
            at = at + 1 + (want - (at + 1)) % 16
        if C not in track:
            track[C] = [n_lanes, 0]
            n_lanes += C
        first_lane, cur = track[C]
        src = cur + 1 + (k - (cur + 1)) % 4
        k += 1
        track[C][1] = src + nf
        if is_big:
            big.append(len(rows))
        rows.append((at, n_out, C, fmt, first_lane, src, fb, nf, sf, out_from))
        data.append(lane_data(rng, nf, C))
        at += n_out * C * SAMPLE_BYTES[fmt]
    out_bytes = at + 3
    rows = np.asarray(rows, np.uint64)
    n_samples = int((rows[:, 5] + rows[:, 7]).max()) + 2
    lane_stride = n_samples + 1 + (n_samples % 2)
    lanes = np.full((n_lanes + 1, lane_stride), np.nan, np.float32)
    for (_, _, C, _, l0, src, _, nf, _, _), v in zip(rows.tolist(), data):
        lanes[l0:l0 + C, src:src + nf] = v.T
    return {"lanes": lanes, "rows": rows, "data": [v.astype(np.float64) for v in data], "out_bytes": out_bytes, "n_lanes": n_lanes + 1,
            "lane_stride": lane_stride, "n_samples": n_samples, "big": big}


def twin_f32(table):
    """the table with every row an f32 file: other bytes (the offsets run through the residues modulo 16 again), same lanes"""
    rows = table["rows"].copy()
    at = 44
    for i in range(len(rows)):
        if i:
            at = at + 1 + (i - (at + 1)) % 16
        rows[i, 0], rows[i, 3] = at, F32
        at += int(rows[i, 1]) * int(rows[i, 2]) * 4
    return dict(table, rows=rows, out_bytes=at + 3)


def canaries(out_bytes):
    return np.full(out_bytes, PAD_BYTE, np.uint8)


def model(table, taps, up, down, mutation=None):
    """-> [row] = (y, B) float64 [C][n_out].  Mutations: "row_phase": the output index counted from the row's first output, not
    the stream's (the row taken for a stream of its own that begins at sample floor(out_from down / up)); "reversed": the taps
    walked from the other end; "given": the stream's length taken to be the COUNT of the given frames (a clip's len), so the sums
    are clipped to [0, n_frames) instead of [0, stream_frames); "planar" is model_bytes'."""
    t = np.asarray(taps, np.float64)
    if mutation == "reversed":
        t = t[::-1]
    out = []
    for (_, n_out, C, _, _, _, fb, nf, sf, out_from), x in zip(table["rows"].tolist(), table["data"]):
        if mutation == "row_phase":
            # output o - out_from of a stream whose sample 0 is the stream's sample `shift`; M up outputs further on the phase is
            # the same and no index is negative; zeros around x for the terms a right model does not have
            shift, M, P = out_from * down // up, 1 << 20, 64 + t.size // up
            out.append(rc.resample_model(_padded(x, P), t, up, down, M * up, n_out, fb - shift + M * down - P, 1 << 61))
        elif mutation == "given":
            keep = max(0, min(nf, nf - fb))   # the given frames that lie below stream sample n_frames
            out.append(rc.resample_model(x[:keep], t, up, down, out_from, n_out, fb, nf))
        else:
            out.append(rc.resample_model(x, t, up, down, out_from, n_out, fb, sf))
    return out


def _padded(x, n):
    """x with n zero frames in front and behind (a wrong model may reach past what a right one reads)"""
    z = np.zeros((n, x.shape[1]))
    return np.concatenate([z, x, z])


def row_f32(out, row):
    """the samples an F32 row wrote -> float32 [C][n_out]"""
    at, n_out, C = int(row[0]), int(row[1]), int(row[2])
    return np.ascontiguousarray(out[at:at + n_out * C * 4].copy().view("<f4").reshape(n_out, C).T)


def model_bytes(table_f32, want, mutation=None):
    """the bytes of an all-f32 table as the model's f32(y) gives them ("planar": channel and frame swapped)"""
    out = canaries(table_f32["out_bytes"])
    for row, (y, _) in zip(table_f32["rows"].tolist(), want):
        v = y.astype(np.float32)
        v = v.reshape(-1) if mutation == "planar" else np.ascontiguousarray(v.T).reshape(-1)
        out[row[0]:row[0] + v.size * 4] = v.view(np.uint8)
    return out


def compare_f32(out, table_f32, want, up, n_taps, what):
    """an all-f32 table's bytes: every row's samples within the bound of the model, every other byte the canary"""
    rest = np.asarray(out, np.uint8).copy()
    assert rest.size == table_f32["out_bytes"], what
    for i, (row, (y, B)) in enumerate(zip(table_f32["rows"].tolist(), want)):
        got = row_f32(out, row)
        assert not np.isnan(got).any(), f"{what}: row {i} holds a NaN: a lane sample outside the given frames was read"
        rc.compare(got, y, B, up, n_taps, f"{what}: row {i}")
        rest[row[0]:row[0] + got.size * 4] = PAD_BYTE
    bad = np.flatnonzero(rest != PAD_BYTE)
    assert bad.size == 0, f"{what}: {bad.size} bytes outside the rows were written, the first at byte {bad[0]}"


def bytes_from_f32(table, table_f32, out_f32):
    """the table's expected bytes: every row the conversion (egress_cases.encode: quantise, little-endian) of the f32 values
    the same row gave in the all-f32 table's output out_f32"""
    out = canaries(table["out_bytes"])
    for row, row32 in zip(table["rows"].tolist(), table_f32["rows"].tolist()):
        v = np.ascontiguousarray(row_f32(out_f32, row32).T).reshape(-1)
        b = ec.encode(v.view(np.uint32), row[3], False).reshape(-1)
        out[row[0]:row[0] + b.size] = b
    return out


def slices(row, cuts, up, down, n_taps):
    """a whole-stream row cut at the outputs `cuts` (ascending, inside the row) -> [(row with src_offset 0, lo, hi)]: each piece
    asks for its outputs and is given exactly its window [lo, hi) of the stream"""
    at, n_out, C, fmt, l0, _, _, _, sf, out_from = (int(v) for v in row)
    fb = C * SAMPLE_BYTES[fmt]
    edges = [out_from] + [int(c) for c in cuts] + [out_from + n_out]
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        lo, hi = rc.window(up, down, n_taps, sf, a, b - a)
        out.append(((at + (a - out_from) * fb, b - a, C, fmt, l0, 0, lo, hi - lo, sf, a), lo, hi))
    return out
