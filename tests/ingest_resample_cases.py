"""The float64 model, the bound and the case tables of the resampling ingest tests (fvad_ingest_resample*;
test_ingest_resample_host.py, test_ingest_resample_gpu.py).

The model is the definition of include/fvad.h in plain numpy float64: with K = (n_taps - 1) / 2 and x the file's decoded samples
of one channel (fvad_ingest's rules; 0 outside [0, file_frames)),
    y[o] = sum over n of x[n] * taps[K + o * down - n * up],   over every n whose tap index lies in [0, 2 K].
`resample_model` walks it phase-wise (P = K + o down = q up + r: taps r + j up against frames q - j) and `brute` states it term
by term, for the host test that holds one against the other.

The library sums in f32: beside every y[o] the model gives B[o] = sum |taps[k]| |x[n]| over the same terms, and a device output
may differ from y[o] by g B[o] plus one f32 ulp of y[o], g = n u / (1 - n u), u = 2^-24, n = ceil(n_taps / up), the most terms of
a phase -- the bound of an n-term fma chain in any order (taps and samples are f32 exactly, so there is no other error).
`compare` holds a result against that; it is computed, not measured."""
import numpy as np

import ingest_cases as ic

F32, PCM16, PCM24 = ic.F32, ic.PCM16, ic.PCM24
SAMPLE_BYTES = ic.SAMPLE_BYTES
FIELDS = 11
U = 2.0 ** -24
# (up, down, half): 16 kHz, 96 kHz and 32 kHz in, a ratio with down > up > 1, 44.1 kHz at the default length, 22.05 kHz short
CASES = ((3, 1, 2), (1, 2, 3), (3, 2, 4), (5, 7, 2), (160, 147, 16), (320, 147, 2))


def gamma(up, n_taps):
    n = -(-n_taps // up)
    return n * U / (1 - n * U)


def out_frames(file_frames, up, down):
    return -(-file_frames * up // down)


def window(up, down, n_taps, file_frames, out_from, n_out):
    """the frames outputs [out_from, out_from + n_out) read, clipped to the file, by the definition (python integers)"""
    if n_out == 0:
        return 0, 0
    K = (n_taps - 1) // 2
    lo = max(0, -(-(out_from * down - K) // up))            # ceil((o down - K) / up)
    hi = ((out_from + n_out - 1) * down + K) // up + 1      # floor((o down + K) / up) + 1
    lo, hi = min(lo, file_frames), min(hi, file_frames)
    return lo, max(lo, hi)


def design(up, down, half=16, cutoff=None, beta=6.0):
    """fvad_resample_design restated: float64 taps (round to float32 to compare)"""
    m = max(up, down)
    K = half * m
    fc = 0.45 / m if cutoff is None else cutoff
    h = 2 * fc * np.sinc(2 * fc * (np.arange(2 * K + 1) - K)) * np.kaiser(2 * K + 1, beta)
    return h / h.sum() * up


def decode_f64(raw, byte_offset, n_frames, n_channels, fmt):
    """the samples [n_frames][n_channels] as float64, by fvad_ingest's rules"""
    v = ic.decode(raw, byte_offset, n_frames, n_channels, fmt)
    if fmt == F32:
        return v.astype(np.uint32).view(np.float32).astype(np.float64)
    return v.astype(np.float64) / (32768.0 if fmt == PCM16 else 8388608.0)


def resample_model(x, taps, up, down, out_from, n_out, frame_base=0, file_frames=None):
    """x float64 [n_frames][C]: frames [frame_base, frame_base + n_frames) of a file of file_frames -> (y, B) float64
    [C][n_out] for outputs [out_from, out_from + n_out).  A needed frame inside the file that x does not hold is an error."""
    t = np.asarray(taps, np.float64)
    n_taps = t.size
    K = (n_taps - 1) // 2
    ff = frame_base + x.shape[0] if file_frames is None else file_frames
    C = x.shape[1]
    y, Bd = np.zeros((C, n_out)), np.zeros((C, n_out))
    if n_out == 0:
        return y, Bd
    # P = K + o down = q up + r.  The first output's P in python integers (no width to get wrong), the others relative to it;
    # frames relative to frame_base, so that the arrays hold small numbers wherever in the file the row lies
    q0, r0 = divmod(K + int(out_from) * down, up)
    rel = r0 + np.arange(n_out, dtype=np.int64) * down
    q_rel, r = rel // up, rel % up
    clip = lambda v: int(max(-(1 << 62), min(1 << 62, v)))
    shift, first, end = clip(q0 - frame_base), clip(-frame_base), clip(ff - frame_base)
    J = -(-n_taps // up)
    for j in range(J):
        k = r + j * up
        idx_all = q_rel + (shift - j)                                  # frame q - j, counted from frame_base
        ok = (k < n_taps) & (idx_all >= first) & (idx_all < end)
        if not ok.any():
            continue
        idx = idx_all[ok]
        assert idx.min() >= 0 and idx.max() < x.shape[0], "the given frames do not cover the window"
        xs = x[idx].T                                                  # [C][sel]
        y[:, ok] += t[k[ok]] * xs
        Bd[:, ok] += np.abs(t[k[ok]]) * np.abs(xs)
    return y, Bd


def brute(x, taps, up, down, o):
    """y[o] of a whole file x [n_frames] term by term, straight from the definition"""
    K = (len(taps) - 1) // 2
    acc = 0.0
    for n in range(len(x)):
        k = K + o * down - n * up
        if 0 <= k <= 2 * K:
            acc += float(x[n]) * float(taps[k])
    return acc


def compare(got, y, B, up, n_taps, what=""):
    """got float32 against the model's y and bound B (same shape)"""
    assert got.dtype == np.float32 and got.shape == y.shape, (what, got.shape, y.shape)
    tol = gamma(up, n_taps) * B + np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - y)
    assert np.all(err <= tol), (what, "at", np.unravel_index(int(np.argmax(err - tol)), err.shape), float(np.max(err - tol)))


# ---------------------------------------------------------------- the case table
def case_taps(up, down, half, kind, seed=5):
    """float32 taps: the library's design rule restated, or finite noise of the same length (asymmetric: a reversed walk shows)"""
    if kind == "design":
        return design(up, down, half).astype(np.float32)
    n = 2 * half * max(up, down) + 1
    return np.random.default_rng(seed).normal(0.0, 0.5, n).astype(np.float32)


def file_bytes(rng, fmt, n):
    """n samples as bytes: PCM with its extremes first (ingest_cases), f32 finite with a few edge values first"""
    if fmt != F32:
        return ic.sample_bytes(rng, fmt, n)
    v = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    edge = np.array([1.0, -1.0, 0.0, -0.0, 1e-38, -3e-39], np.float32)
    v[:edge.size] = edge[:n]
    return v.view(np.uint8)


# (format, channels): every format with 1 .. 3 channels, 64 channels of the widest and of the narrowest sample
COMBOS = ((PCM16, 1), (PCM24, 2), (F32, 3), (F32, 64), (PCM16, 3), (PCM24, 1), (F32, 2), (PCM16, 64))
SHORT_COMBOS = ((PCM16, 1), (PCM24, 2), (F32, 3), (F32, 64))


def case_table(up, down, n_taps, tile_of, seed=23):
    """-> dict(raw, files [(byte_offset, fmt, C, file_frames)], rows [n][11] uint64 (each a whole-file source: frame_base 0, all
    frames given), file_of [row -> file], n_lanes, lane_stride (odd), n_samples).  tile_of(C, fmt) is the kernel's tile T.
    Per (format, channels) a file of a little more than 2 T + 1 outputs with rows of T - 1, T, T + 1 and 2 T + 1 outputs from
    the file's first, T + 1 outputs up to its last, and 5 outputs from the middle; files of 0, 1, 2 frames and of about half
    the filter's reach, whole.  Rows of one channel count lie one behind the other on their lanes, a canary or more between
    them; dst_offset runs through the 4 alignments (the odd lane_stride moves them again lane by lane), the fills through 0, 1,
    7 and 9; byte offsets run through the residues modulo 4 per format."""
    rng = np.random.default_rng(seed)
    K = (n_taps - 1) // 2
    files, rows, file_of, chunks = [], [], [], []
    at = 0
    byte_res = {F32: 0, PCM16: 0, PCM24: 0}
    track = {}
    n_lanes = 1   # lane 0 belongs to no source
    k = 0

    def add_file(fmt, C, ff):
        nonlocal at
        want = byte_res[fmt]
        byte_res[fmt] = (want + 1) % 4
        pad = 1 + (want - (at + 1)) % 4
        chunks.append(np.full(pad, ic.PAD_BYTE, np.uint8))
        at += pad
        data = file_bytes(rng, fmt, ff * C)
        chunks.append(data)
        files.append((at, fmt, C, ff))
        at += data.size
        return len(files) - 1

    def add_row(fi, out_from, n_out):
        nonlocal n_lanes, k
        byte_offset, fmt, C, ff = files[fi]
        if C not in track:
            track[C] = [n_lanes, 0]
            n_lanes += C
        first_lane, cur = track[C]
        dst = cur + 1 + (k - (cur + 1)) % 4
        fill = (0, 1, 7, 9)[(k // 4 + k) % 4]
        track[C][1] = dst + n_out + fill
        k += 1
        rows.append((byte_offset, ff, C, fmt, first_lane, dst, dst + n_out + fill, 0, ff, out_from, n_out))
        file_of.append(fi)

    for fmt, C in COMBOS:
        T = tile_of(C, fmt)
        ff = -(-(2 * T + 1) * down // up) + 5
        fi = add_file(fmt, C, ff)
        OF = out_frames(ff, up, down)
        assert OF >= 2 * T + 1
        for n_out in (T - 1, T, T + 1, 2 * T + 1):
            add_row(fi, 0, n_out)
        add_row(fi, OF - (T + 1), T + 1)
        add_row(fi, OF // 2, 5)
    for fmt, C in SHORT_COMBOS:
        for ff in (0, 1, 2, max(3, K // up)):
            fi = add_file(fmt, C, ff)
            add_row(fi, 0, out_frames(ff, up, down))
    chunks.append(np.full(3, ic.PAD_BYTE, np.uint8))
    rows = np.asarray(rows, np.uint64)
    n_samples = int(rows[:, 6].max()) + 2
    return {"raw": np.concatenate(chunks), "files": files, "rows": rows, "file_of": file_of, "n_lanes": n_lanes + 1,
            "lane_stride": n_samples + 1 + (n_samples % 2), "n_samples": n_samples}


def twin_f32(table):
    """the table with every PCM file replaced by the f32 file holding s / 32768 (PCM24: s / 8388608): other bytes, same lanes"""
    chunks, files, new_at, at = [], [], {}, 0
    for fi, (byte_offset, fmt, C, ff) in enumerate(table["files"]):
        pad = 1 + (fi % 4)
        chunks.append(np.full(pad, ic.PAD_BYTE, np.uint8))
        at += pad
        data = decode_f64(table["raw"], byte_offset, ff, C, fmt).astype(np.float32).reshape(-1).view(np.uint8)   # (exact: 24 bits at most)
        chunks.append(data)
        files.append((at, F32, C, ff))
        new_at[fi] = at
        at += data.size
    chunks.append(np.full(3, ic.PAD_BYTE, np.uint8))
    rows = table["rows"].copy()
    for i, fi in enumerate(table["file_of"]):
        rows[i, 0], rows[i, 3] = new_at[fi], F32
    return dict(table, raw=np.concatenate(chunks), files=files, rows=rows)


def model_lanes(table, taps, up, down, lanes_in):
    """-> (want [row] = (y, B) of the row's outputs, lanes: lanes_in with every row's fill zeroed and its outputs as f32(y) --
    the exact part of the expectation is the zeros and the canaries)"""
    lanes = lanes_in.copy()
    lb = ic.bits(lanes)
    want, cache = [], {}
    for row, fi in zip(table["rows"].tolist(), table["file_of"]):
        byte_offset, ff, C, fmt, l0, dst, fill_to, _, _, out_from, n_out = row
        if fi not in cache:
            cache[fi] = decode_f64(table["raw"], byte_offset, ff, C, fmt)
        y, B = resample_model(cache[fi], taps, up, down, out_from, n_out)
        want.append((y, B))
        lanes[l0:l0 + C, dst:dst + n_out] = y.astype(np.float32)
        lb[l0:l0 + C, dst + n_out:fill_to] = 0
    return want, lanes


def compare_lanes(got, table, want, lanes_want, up, n_taps, what):
    """the rows' outputs within the bound; everything else (zeros, canaries) bit for bit"""
    g, w = ic.bits(got).copy(), ic.bits(lanes_want).copy()
    for row, (y, B) in zip(table["rows"].tolist(), want):
        _, _, C, _, l0, dst, _, _, _, _, n_out = row
        compare(got[l0:l0 + C, dst:dst + n_out], y, B, up, n_taps, what)
        g[l0:l0 + C, dst:dst + n_out] = 0
        w[l0:l0 + C, dst:dst + n_out] = 0
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} samples outside the outputs differ, the first at lane {bad[0][0]} sample {bad[0][1]}"


def slices(row, cuts, up, down, n_taps):
    """a whole-file row cut at the outputs `cuts` (ascending, inside the row) -> rows that each give exactly their window"""
    byte_offset, _, C, fmt, l0, dst, fill_to, _, ff, out_from, n_out = [int(v) for v in row]
    fb = C * SAMPLE_BYTES[fmt]
    edges = [out_from] + [int(c) for c in cuts] + [out_from + n_out]
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        lo, hi = window(up, down, n_taps, ff, a, b - a)
        d = dst + (a - out_from)
        out.append((byte_offset + lo * fb, hi - lo, C, fmt, l0, d, fill_to if b == out_from + n_out else d + (b - a), lo, ff, a, b - a))
    return out
