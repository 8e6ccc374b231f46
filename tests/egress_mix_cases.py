"""The numpy model and the case table of the two-source egress tests (fvad_egress_mix*; test_egress_mix_host.py,
test_egress_mix_gpu.py, test_egress_mix_harness_gpu.py), beside egress_cases.py, whose conversion they import.

The model is the statement of what fvad_egress_mix_device computes.  A sink (byte_offset, n_frames, n_channels, format,
first_lane, src_offset, orig_offset, orig_zeros) takes for frame f and channel c
    y = den[first_lane + c][src_offset + f],   x = +0 for f < orig_zeros, else orig[first_lane + c][orig_offset + f - orig_zeros],
    v = w_den * y when w_orig == 0 (the original is not read), w_orig * x when w_den == 0 (the denoised is not read),
        else w_orig * x + w_den * y: float32 products and a float32 sum, each rounded,
and writes v as egress_cases.encode writes an f32 lane sample.  Nothing else of the output changes.
`mix_model(..., mutation=...)` states six wrong versions; test_egress_mix_host.py shows that the case table fails each of them.
Comparisons are of bytes -- but for a NaN in an f32 file, whose payload the library does not promise: `compare` takes any NaN for
any NaN there."""
import numpy as np

import egress_cases as ec

F32, PCM16, PCM24 = ec.F32, ec.PCM16, ec.PCM24
FIELDS = 8
DELAY = 482                  # fvad_nsnet2_delay(48000)
# the five pairs the feature was specified with, and (-1, 0): a negative weight alone, whose leading zeros are -0.0 in an f32 file
WEIGHTS = ((1.0, 0.0), (0.0, 1.0), (1.0, -1.0), (0.25, 0.75), (-0.3, 1.7), (-1.0, 0.0))
MUTATIONS = ("no_delay", "zeros_read", "swapped", "single_round", "zero_times", "planar")


def _take(lanes, first_lane, n_channels, index):
    """lanes[first_lane + c][index[f]] as [c][f]; an index outside the lane (a wrong model's) is clipped into it"""
    return lanes[first_lane:first_lane + n_channels][:, np.clip(index, 0, lanes.shape[1] - 1)]


def mix_values(orig, den, row, w_orig, w_den, mutation=None):
    """the float32 values v of one sink, [frame][channel] (planar: [channel][frame]) flattened"""
    _, n, C, _, l0, src, oo, z = (int(x) for x in row)
    wo, wd = np.float32(w_orig), np.float32(w_den)
    if mutation == "swapped":
        wo, wd = wd, wo
    f = np.arange(n, dtype=np.int64)
    k = 0 if mutation == "no_delay" else min(z, n)
    with np.errstate(all="ignore"):
        x = y = None
        if wo != 0 or mutation == "zero_times":
            x = _take(orig, l0, C, oo + f - k).astype(np.float32)
            if mutation != "zeros_read":
                x[:, :k] = np.float32(0.0)
        if wd != 0 or mutation == "zero_times":
            y = _take(den, l0, C, src + f).astype(np.float32)
        if x is None:
            v = wd * y
        elif y is None:
            v = wo * x
        elif mutation == "single_round":
            v = (np.float64(wo) * x.astype(np.float64) + np.float64(wd) * y.astype(np.float64)).astype(np.float32)
        else:
            v = (wo * x).astype(np.float32) + (wd * y).astype(np.float32)
    v = np.asarray(v, np.float32)
    return v.reshape(-1) if mutation == "planar" else np.ascontiguousarray(v.T).reshape(-1)


def mix_model(orig, den, sinks, w_orig, w_den, out_in, mutation=None):
    """orig [n_lanes][orig_stride], den [n_lanes][den_stride] float32, out_in [bytes] uint8 -> the bytes after the sinks, a new array"""
    out = out_in.copy()
    for row in np.asarray(sinks, np.uint64).reshape(-1, FIELDS).tolist():
        v = mix_values(orig, den, row, w_orig, w_den, mutation)
        b = ec.encode(v.view(np.uint32), int(row[3]), False).reshape(-1)
        out[int(row[0]):int(row[0]) + b.size] = b
    return out


def naive_model(orig, den, sinks, w_orig, w_den, out_in):
    """the definition written out sample by sample (for a few small sinks)"""
    out = out_in.copy()
    wo, wd = np.float32(w_orig), np.float32(w_den)
    for o, n, C, fmt, l0, src, oo, z in np.asarray(sinks, np.uint64).reshape(-1, FIELDS).tolist():
        B = ec.SAMPLE_BYTES[fmt]
        for f in range(n):
            for c in range(C):
                with np.errstate(all="ignore"):
                    if wo == 0:
                        v = np.float32(wd * den[l0 + c, src + f])
                    else:
                        x = np.float32(0.0) if f < z else orig[l0 + c, oo + f - z]
                        v = np.float32(wo * x) if wd == 0 else np.float32(np.float32(wo * x) + np.float32(wd * den[l0 + c, src + f]))
                at = o + (f * C + c) * B
                out[at:at + B] = ec.encode(np.array([v], np.float32).view(np.uint32), fmt, False).reshape(-1)
    return out


def canonical(buf, sinks):
    """buf with every NaN of an f32 sink replaced by one NaN (the payload is not promised)"""
    buf = np.array(buf, np.uint8)
    for o, n, C, fmt in np.asarray(sinks, np.uint64).reshape(-1, FIELDS)[:, :4].tolist():
        if fmt != F32 or n == 0:
            continue
        u = buf[o:o + n * C * 4].copy().view("<u4")
        u[np.isnan(u.view("<f4"))] = 0x7FC00000
        buf[o:o + n * C * 4] = u.view(np.uint8)
    return buf


def compare(got, want, sinks, what):
    ec.compare(canonical(got, sinks), canonical(want, sinks), what)


# ---------------------------------------------------------------- the case table
SMALL_FRAMES = ec.SMALL_FRAMES
CHANNELS = ec.CHANNELS
BIG = ec.BIG
ALIGN_FRAMES = 37            # several whole 16-byte groups and a ragged end, whatever the two alignments


def _lane_data(rng, n, C, reverse):
    """[C][n] lane samples of one range: egress_cases' special values first in the flat [frame][channel] order (reverse: in
    reverse order, so that the two sources meet with different partners), noise past +-1 behind them"""
    v = ec.lane_samples(rng, False, n * C)
    if reverse:
        k = min(len(ec.F32_FIRST), n * C)
        v[:k] = v[:k][::-1].copy()
    return v.reshape(n, C).T.view(np.float32)


def case_table(w_orig, w_den, seed=21):
    """-> dict(orig [n_lanes][orig_stride], den [n_lanes][den_stride] float32, sinks [n][8] uint64, out_bytes, n_lanes,
    orig_stride (odd), orig_samples, den_stride (even, another value), den_samples, names {name: row}).
    The rows, their ranges and the live sources' contents do not depend on the weights.  Every sink has lane samples of its own in
    both sources (each range begins with the special values); every sample outside the ranges is NaN.  A source whose weight is
    zero holds +-inf everywhere instead: it must not be read, and must not be multiplied by its zero.
    Rows: the small sinks (0 .. 5 frames, every file format and channel count) and the 64 "align" sinks (src_offset modulo 8 x
    orig_offset modulo 8) one behind the other on a track of lanes per channel count, the sinks around the tile size on lanes
    of their own; orig_zeros runs through 0, 1, 3, 482, T + 5, n_frames, past n_frames and 2^63.  In the output the sinks lie one
    behind the other with a PAD_BYTE or more between them -- except "adjacent-a" / "adjacent-b", whose byte ranges touch --,
    byte_offset through every residue modulo 16 per format.  The rows are then shuffled."""
    rng = np.random.default_rng(seed)
    formats = (PCM16, PCM24, F32)
    specs = []   # (name, fmt, C, n_frames, orig_zeros, want src residue, want orig residue)
    k = 0
    for fmt in formats:
        for C in CHANNELS:
            for n in SMALL_FRAMES:
                specs.append((f"small-{fmt}-{C}-{n}", fmt, C, n, (0, 1, 3, n, n + 2, DELAY, 1 << 63)[k % 7], k % 8, (k // 8 + k) % 8))
                k += 1
    pair = 0
    for fmt in formats:
        for C in BIG[fmt]:
            T = ec.tile_frames(C, fmt)
            for i, n in enumerate((T - 1, T, T + 1, 2 * T + 3, 2 * T + 3)):
                # the two longest: the delay, and zeros that end inside the second tile; the others in turn
                z = DELAY if i == 3 else T + 5 if i == 4 else ((0, n, 3), (1, n + 9, 0), (3, 1, n))[pair % 3][i]
                specs.append((f"big-{fmt}-{C}-{i}", fmt, C, n, z, k % 8, (3 * k + 1) % 8))
                k += 1
            pair += 1
    for a in range(8):
        for b in range(8):
            q = a * 8 + b
            specs.append((f"align-{a}-{b}", formats[q % 3], (1, 2)[(q // 3) % 2], ALIGN_FRAMES, (0, 1, 3, 5, 0, 2)[q % 6], a, b))
    specs.append(("adjacent-a", F32, 2, 9, 4, 1, 6))
    specs.append(("adjacent-b", F32, 3, 6, 0, 3, 2))

    rows, names, data = [], {}, []
    at = 0
    byte_res = {f: 0 for f in formats}
    track = {C: None for C in CHANNELS}   # [first_lane, denoised cursor, original cursor] of the tracked sinks per channel count
    n_lanes = 1                           # lane 0 belongs to no sink
    for name, fmt, C, n, z, res_d, res_o in specs:
        if name == "adjacent-b":
            byte_offset = at                              # touches adjacent-a's last byte
        else:   # at the next offset with the format's next residue, at least one pad byte after the previous sink
            want = byte_res[fmt]
            byte_res[fmt] = (want + 1) % 16
            byte_offset = at + 1 + (want - (at + 1)) % 16
        at = byte_offset + n * C * ec.SAMPLE_BYTES[fmt]
        n_read = n - min(z, n)
        if name.startswith("big"):
            first_lane, src, oo = n_lanes, res_d, res_o
            n_lanes += C
        else:
            if track[C] is None:
                track[C] = [n_lanes, 0, 0]
                n_lanes += C
            first_lane, cur_d, cur_o = track[C]
            src, oo = cur_d + (res_d - cur_d) % 8, cur_o + (res_o - cur_o) % 8
            track[C][1], track[C][2] = src + n, oo + n_read
        names[name] = len(rows)
        rows.append((byte_offset, n, C, fmt, first_lane, src, oo, z))
        data.append((_lane_data(rng, n, C, False), _lane_data(rng, n_read, C, True)))
    out_bytes = at + 3
    rows = np.asarray(rows, np.uint64)
    n_read = rows[:, 1] - np.minimum(rows[:, 7], rows[:, 1])
    den_samples, orig_samples = int((rows[:, 5] + rows[:, 1]).max()) + 2, int((rows[:, 6] + n_read).max()) + 5
    den_stride = den_samples + 2 + (den_samples % 2)       # even
    orig_stride = orig_samples + 1 + (orig_samples % 2)    # odd
    n_lanes += 1
    den, orig = np.full((n_lanes, den_stride), np.nan, np.float32), np.full((n_lanes, orig_stride), np.nan, np.float32)
    for (_, n, C, _, first_lane, src, oo, z), (vd, vo) in zip(rows.tolist(), data):
        den[first_lane:first_lane + C, src:src + n] = vd
        orig[first_lane:first_lane + C, oo:oo + vo.shape[1]] = vo
    for lanes, w in ((orig, w_orig), (den, w_den)):
        if w == 0:
            lanes[:] = np.where((np.arange(lanes.size).reshape(lanes.shape) % 3) == 0, -np.inf, np.inf)
    order = rng.permutation(len(rows))
    names = {k: int(np.nonzero(order == v)[0][0]) for k, v in names.items()}
    return {"orig": orig, "den": den, "sinks": np.ascontiguousarray(rows[order]), "out_bytes": out_bytes, "n_lanes": n_lanes,
            "orig_stride": orig_stride, "orig_samples": orig_samples, "den_stride": den_stride, "den_samples": den_samples, "names": names}


def unit_gain_weights(fv):
    """NSNet2-shaped weights whose every gain is exactly 1.0f: the library's seeded synthetic model with its last layer zeroed and
    a bias of +30 (sigmoid(30) rounds to 1.0f), so that the denoiser is its analysis, synthesis and resamplers alone"""
    wd = fv.synth_weights(7)
    wd["fc4_w"] = np.zeros_like(wd["fc4_w"])
    wd["fc4_b"] = np.full_like(wd["fc4_b"], 30.0)
    return wd


def as_egress_rows(sinks):
    """the fvad_egress rows of the same sinks (the first six fields)"""
    return np.ascontiguousarray(np.asarray(sinks, np.uint64).reshape(-1, FIELDS)[:, :6])
