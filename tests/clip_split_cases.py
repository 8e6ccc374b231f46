"""The split-source tables and model of the batch Recorder tests (fvad_clips_export_split*; test_clips_split_host.py,
test_clips_split_gpu.py), on top of clip_cases.py's case table, sources and float64 model.

Every clip of the case table is cut at the seams
    sigma in {0, 1, 3, len // 2, len - 3, len - 1, len, T - 1, T, T + 1, 2 T} & [0, len],   T = 8192,
its first sigma samples laid into buffer A and the rest into buffer B.  A and B are separate arrays with different lane counts,
strides and lane order (a stream's first lane differs between the two and from the contiguous source), every piece at its own
place with at least one sentinel / NaN sample around it, as everything else in both buffers is.  One case (`ALL_PAIRS`) is laid
out at every pair of (a_from, b_from) offsets within 16 bytes, the others rotate through a few pairs.

What a split export has to give is what the contiguous clip gives (`expected_rows` maps the base clips' results to the rows).
Beyond clip_cases.compare's rules (picks, offsets and sample bits exact, RMS within one f32 ulp of the f64 model) the split
form promises the contiguous form's bits, sums included: `sum_sq` restates the kernels' sum in numpy float64 -- lane t of 256
adds the squares of samples t, t + 256, ... of a tile of T, a shuffle tree adds the 64 lanes of a wave, then ((w0 + w1) + w2) +
w3, tiles in order -- which is exact IEEE arithmetic on both sides, so a model that tiles from the seam instead of from the
clip's first sample gives other bits.  `model_export_split(..., mutation=...)` states three wrong versions; test_clips_split_host.py
shows that `compare_split` over the table fails each of them."""
import numpy as np

import clip_cases as cc

T = cc.TILE
FIELDS = 7                       # n_channels, a_lane, a_from, a_len, b_lane, b_from, b_len
# a stream's first lane in A and in B (clip_cases.STREAMS has A 1, B 2, C 4, D 7 of 12 lanes)
A_LANES, A_FIRST = 11, {"D": 0, "C": 5, "B": 8, "A": 10}
B_LANES, B_FIRST = 15, {"A": 2, "B": 3, "C": 6, "D": 10}
ALL_PAIRS = "dup"                # the clip laid out at every pair of offsets (stream C: three channels, 8995 samples)
FEW_PAIRS = ((0, 0), (1, 3), (3, 1), (2, 2), (0, 1), (3, 0))    # in elements; the rest of the rows rotate through these


def seams(n):
    return sorted({s for s in (0, 1, 3, n // 2, n - 3, n - 1, n, T - 1, T, T + 1, 2 * T) if 0 <= s <= n})


def _stream_of(l0):
    return next(s for s, (first, _) in cc.STREAMS.items() if first == l0)


class SplitTable:
    """rows [n][7] uint64 over A [A_LANES][a_stride] and B [B_LANES][b_stride] (numpy, the source's dtype; a_samples /
    b_samples of each lane are in use), base[n] = the row's clip in the case table, sigma[n] = its seam"""

    def __init__(self, pcm16, seed=5):
        self.pcm16 = pcm16
        self.clips, self.names = cc.case_table()
        self.src = cc.mask_outside(cc.make_source(pcm16, seed), self.clips)
        per16 = 8 if pcm16 else 4
        plan = []                                   # (base, sigma, (a offset, b offset) within 16 bytes, in elements)
        k = 0
        for i, (l0, C_, a, b) in enumerate(self.clips.astype(np.int64)):
            for s in seams(int(b - a)):
                plan.append((i, s, FEW_PAIRS[k % len(FEW_PAIRS)]))
                k += 1
        i = self.names[ALL_PAIRS]
        n = int(self.clips[i, 3] - self.clips[i, 2])
        plan += [(i, n // 2, (x, y)) for x in range(per16) for y in range(per16)]
        # odd strides, so that the lanes of a stream start at different offsets within 16 bytes; the buffers themselves are
        # 16-byte aligned on the device, so an element index's offset is its address's
        need_a, need_b = {s: 1 for s in cc.STREAMS}, {s: 1 for s in cc.STREAMS}
        places = []
        for i, s, (x, y) in plan:
            l0, C_, a, b = (int(v) for v in self.clips[i])
            st = _stream_of(l0)
            n = b - a
            places.append((st, need_a[st], need_b[st]))
            need_a[st] += s + per16 + 1             # room to move the piece to its offset, and a sentinel behind it
            need_b[st] += n - s + per16 + 1
        self.a_samples, self.b_samples = max(need_a.values()) + per16, max(need_b.values()) + per16
        self.a_stride, self.b_stride = self.a_samples + 3 | 1, self.b_samples + 7 | 1
        fill = cc.SENTINEL if pcm16 else np.nan
        self.A = np.full((A_LANES, self.a_stride), fill, self.src.dtype)
        self.B = np.full((B_LANES, self.b_stride), fill, self.src.dtype)
        rows, self.base, self.sigma = [], [], []
        for (i, s, (x, y)), (st, ca, cb) in zip(plan, places):
            l0, C_, a, b = (int(v) for v in self.clips[i])
            la, lb = A_FIRST[st], B_FIRST[st]
            # the first channel's address offset: (lane * stride + from) mod per16 == the wanted offset
            fa = ca + (x - (la * self.a_stride + ca)) % per16
            fb = cb + (y - (lb * self.b_stride + cb)) % per16
            self.A[la:la + C_, fa:fa + s] = self.src[l0:l0 + C_, a:a + s]
            self.B[lb:lb + C_, fb:fb + b - a - s] = self.src[l0:l0 + C_, a + s:b]
            rows.append((C_, la if s else 0, fa if s else 0, s, lb if s < b - a else 0, fb if s < b - a else 0, b - a - s))
            self.base.append(i)
            self.sigma.append(s)
        self.rows = np.array(rows, np.uint64)
        self.base, self.sigma = np.array(self.base), np.array(self.sigma)

    def a(self, address=None):
        return (address, A_LANES, self.a_stride, self.a_samples)

    def b(self, address=None):
        return (address, B_LANES, self.b_stride, self.b_samples)

    def offsets_mod16(self):
        """{(a_from's, b_from's address offset within 16 bytes)} of the rows that have both pieces, first channel"""
        by = 2 if self.pcm16 else 4
        r = self.rows.astype(np.int64)
        both = (r[:, 3] > 0) & (r[:, 6] > 0)
        return {(int((la * self.a_stride + fa) * by % 16), int((lb * self.b_stride + fb) * by % 16))
                for _, la, fa, _, lb, fb, _ in r[both]}


def plan_rows(rows, out_pcm16):
    return cc.plan([(0, 1, 0, int(r[3] + r[6])) for r in np.asarray(rows, np.int64)], out_pcm16)


def _tile_sum(x):
    """one tile's partial as rms_tile adds it: x float64, at most T of them"""
    pad = np.zeros(-len(x) % 256)                    # (a lane without a sample adds nothing: s + 0 = s for s >= 0)
    sq = np.concatenate([x * x, pad]).reshape(-1, 256)
    lane = np.zeros(256)
    for row in sq:
        lane = lane + row
    w = lane.reshape(4, 64).copy()
    o = 32
    while o:
        w[:, :o] = w[:, :o] + w[:, o:2 * o]
        o //= 2
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def sum_sq(x, starts=None):
    """the f64 sum of squares of a channel's samples (any dtype of the tables) as the kernels add it; starts: where the tiles
    begin (None: every T from the first sample -- the rule)"""
    v = cc.as_f32(x).astype(np.float64)
    cuts = list(range(0, len(v), T)) if starts is None else starts
    s = 0.0
    for k, at in enumerate(cuts):
        s = s + _tile_sum(v[at:cuts[k + 1] if k + 1 < len(cuts) else len(v)])
    return s


def _rms_of_sum(s, n):
    return np.float32(np.sqrt(s / float(n)))


def _pick(r):
    pick, vol = 0, np.float32(9999.0)
    for c in range(len(r)):
        if r[c] < vol:
            pick, vol = c, r[c]
    others = [r[c] for c in range(len(r)) if c != pick]
    return pick, r[pick], (min(others) if others else r[pick])


def model_export_contiguous(src, clips, out_pcm16):
    """clip_cases.model_export with the kernels' own sums beside it: sums[i][c] (f64) and the RMS taken from them (rms_k,
    runner_k) -- what both device forms give bit for bit"""
    m = cc.model_export(src, clips, out_pcm16)
    m["sums"], m["rms_k"], m["runner_k"] = [], [], []
    for l0, C_, a, b in np.asarray(clips, np.int64):
        s = [sum_sq(src[l0 + c, a:b]) for c in range(C_)]
        _, best, runner = _pick([_rms_of_sum(x, b - a) for x in s])
        m["sums"].append(s)
        m["rms_k"].append(best)
        m["runner_k"].append(runner)
    return m


def model_export_split(t, rows, out_pcm16, mutation=None):
    """the statement of fvad_clips_export_split in numpy over t.A / t.B.  mutation: None | "seam" (the seam one sample late:
    A gives a_len + 1 samples, B starts one later) | "tiles" (the tiles counted from the seam) | "swapped" (B's piece first)"""
    rows = np.asarray(rows, np.int64)
    offsets, total = plan_rows(rows, out_pcm16)
    out = {k: [] for k in ("best_channel", "best_rms", "runner_up_rms", "samples", "sums", "rms_k", "runner_k")}
    for C_, la, fa, na, lb, fb, nb in rows:
        chans, sums = [], []
        for c in range(C_):
            d = 1 if mutation == "seam" and na and nb else 0
            pa, pb = t.A[la + c, fa:fa + na + d], t.B[lb + c, fb + d:fb + nb]
            x = np.concatenate([pb, pa] if mutation == "swapped" else [pa, pb])
            starts = None
            if mutation == "tiles":
                starts = list(range(0, na, T)) + list(range(na, na + nb, T))
            chans.append(x)
            sums.append(sum_sq(x, starts))
        pick, best, runner = _pick([cc.rms_f32(x) for x in chans])
        _, best_k, runner_k = _pick([_rms_of_sum(s, na + nb) for s in sums])
        out["best_channel"].append(pick)
        out["best_rms"].append(best)
        out["runner_up_rms"].append(runner)
        out["samples"].append(cc.convert(chans[pick], out_pcm16))
        out["sums"].append(sums)
        out["rms_k"].append(best_k)
        out["runner_k"].append(runner_k)
    return {"best_channel": np.array(out["best_channel"], np.int32), "best_rms": np.array(out["best_rms"], np.float32),
            "runner_up_rms": np.array(out["runner_up_rms"], np.float32), "offsets": offsets, "total": total,
            "samples": out["samples"], "sums": out["sums"], "rms_k": out["rms_k"], "runner_k": out["runner_k"]}


def expected_rows(want, base, rows, out_pcm16):
    """the base clips' results (a model's dict or the library's, with `samples`) as the rows' results: row r is clip base[r]"""
    offsets, total = plan_rows(rows, out_pcm16)
    res = {k: np.asarray(want[k])[base] for k in ("best_channel", "best_rms", "runner_up_rms")}
    res.update(offsets=offsets, total=total, samples=[want["samples"][i] for i in base])
    for k in ("sums", "rms_k", "runner_k"):
        if k in want:
            res[k] = [want[k][i] for i in base]
    return res


def compare_split(got, want, what=""):
    """clip_cases.compare, and where both sides carry the kernels' sums: those, and the RMS values they give, bit for bit"""
    cc.compare(got, want, what)
    if "sums" in got and "sums" in want:
        for i, (g, w) in enumerate(zip(got["sums"], want["sums"])):
            assert np.array(g).tobytes() == np.array(w).tobytes(), (what, "the f64 sums of row", i)
        for k in ("rms_k", "runner_k"):
            assert np.array(got[k], np.float32).tobytes() == np.array(want[k], np.float32).tobytes(), (what, k)
