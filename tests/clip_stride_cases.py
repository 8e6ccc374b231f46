"""The model and the case tables of the strided Recorder tests (fvad_clips_export*_strided; test_clips_stride_host.py,
test_clips_stride_gpu.py), on top of clip_cases.py's sources and float64 model and clip_split_cases.py's split model.

The rule, in numpy: a strided export of a clip with `skip` < `step` is the full-rate export's pick and RMS values -- taken over
EVERY sample of the clip -- and its samples[skip::step]; slots are 16-byte aligned, in clip order, sized by
out_len = ceil((len - skip) / step).  skip = (phase + step - sample_from mod step) mod step keeps the lane indices = phase
(mod step).  For a split clip the stride runs through the seam.

The table (`Table`): every clip of clip_cases.case_table(), and per (step, phase) of STEPS x 0..step-1 the clips whose out_len
is T_o - 1, T_o, T_o + 1, 2 T_o + 1 and 1 (T_o = tile_out(step), the gather's tile in output samples), each starting at each of
the 8 sample alignments, with 0..step-1 samples behind the last kept one.  A case is (step, phase, the indices of its clips):
the base clips and the case's own edge clips; base clips with len <= skip keep no sample and are on the case's `refused` list.
For the split form (`cuts`, `SplitLayout`) the case's edge clips are cut at clip_split_cases.seams and at skip - 1, skip,
skip + 1 and directly before and after a kept sample in the middle.

`model_export_strided` / `model_export_split_strided` state four wrong versions; test_clips_stride_host.py shows that the table
fails each of them."""
import numpy as np

import clip_cases as cc
import clip_split_cases as sc

TILE = cc.TILE                   # kClipTile: the source samples a workgroup stages
STEPS = (2, 3, 6)
STEP_MAX = 16                    # FVAD_CLIP_STEP_MAX
EDGE_STREAM, EDGE_ZONE = "B", 1  # the edge clips: stereo, channel 1 the quietest


def tile_out(step):
    """the strided gathers' tile in OUTPUT samples: floor(TILE / step) rounded down to a multiple of 8"""
    return TILE // step // 8 * 8


TILE_OUT_3 = 2728                # tile_out(3): 8182 source samples staged
assert tile_out(3) == TILE_OUT_3 and tile_out(1) == TILE


def phase_skip(sample_from, step, phase):
    return (phase + step - int(sample_from) % step) % step


def out_len(n, skip, step):
    return -(-(int(n) - int(skip)) // step)


def plan_strided(lens, skips, step, out_pcm16):
    """-> (out_lens, offsets, total) in samples of the output format; skips None: all 0"""
    per16 = 8 if out_pcm16 else 4
    outs, offsets, at = [], [], 0
    for i, n in enumerate(lens):
        k = 0 if skips is None else int(skips[i])
        assert k < step and int(n) > k
        outs.append(out_len(n, k, step))
        offsets.append(at)
        at += (outs[-1] + per16 - 1) // per16 * per16
    return np.array(outs, np.uint64), np.array(offsets, np.uint64), at


class Case:
    def __init__(self, step, phase, idx, refused, edge):
        self.step, self.phase, self.idx, self.refused, self.edge = step, phase, idx, refused, edge

    def __repr__(self):
        return f"step{self.step}-phase{self.phase}"


class Table:
    """clips [n][4] uint64 (the base table, then every case's edge clips), skips-free: a case computes its own"""

    def __init__(self):
        base, self.names = cc.case_table()
        self.n_base = len(base)
        clips = [tuple(int(v) for v in c) for c in base]
        l0, C_ = cc.STREAMS[EDGE_STREAM]
        z0 = cc.zones(EDGE_STREAM)[EDGE_ZONE][0]
        self.cases = []
        for step in STEPS:
            To = tile_out(step)
            for phase in range(step):
                edge = []
                for j, target in enumerate((To - 1, To, To + 1, 2 * To + 1, 1)):
                    for i in range(8):
                        a = z0 + 16 * j + i
                        n = phase_skip(a, step, phase) + (target - 1) * step + 1 + (i + j) % step
                        edge.append(len(clips))
                        clips.append((l0, C_, a, a + n))
                ok = [k for k in range(self.n_base) if clips[k][3] - clips[k][2] > phase_skip(clips[k][2], step, phase)]
                refused = [k for k in range(self.n_base) if k not in ok]
                self.cases.append(Case(step, phase, np.array(ok + edge), np.array(refused, int), np.array(edge)))
        self.clips = np.array(clips, np.uint64)
        assert int(self.clips[:, 3].max()) <= cc.N_SAMPLES

    def source(self, pcm16, seed=5):
        return cc.mask_outside(cc.make_source(pcm16, seed), self.clips)

    def skips(self, case, idx=None):
        idx = case.idx if idx is None else idx
        return np.array([phase_skip(self.clips[k, 2], case.step, case.phase) for k in idx], np.uint32)


def strided_of(full, idx, skips, step, out_pcm16, lens, mutation=None):
    """what a strided export of clips idx has to give, from a full-rate result `full` (the model's dict or the library's with
    `samples`) over the whole table.  mutation: None | "skip0" (the phase counted from the clip's first sample) | "floor" (out_len
    by floor: the last kept sample dropped where the stride does not end on it)"""
    eff = [0 if mutation == "skip0" else int(k) for k in skips]
    samples = [full["samples"][i][k::step] for i, k in zip(idx, eff)]
    if mutation == "floor":
        samples = [s[:max((int(n) - k) // step, 1)] for s, n, k in zip(samples, lens, eff)]
    per16 = 8 if out_pcm16 else 4
    offsets, at = [], 0
    for s in samples:
        offsets.append(at)
        at += (len(s) + per16 - 1) // per16 * per16
    res = {k: np.asarray(full[k])[idx] for k in ("best_channel", "best_rms", "runner_up_rms")}
    res.update(offsets=np.array(offsets, np.uint64), total=at, samples=samples)
    return res


def model_export_strided(src, clips, skips, step, out_pcm16, mutation=None):
    """the statement of fvad_clips_export_strided in numpy.  mutation: strided_of's, or "kept" (RMS and pick over the kept
    samples only)"""
    clips = np.asarray(clips, np.int64)
    lens = clips[:, 3] - clips[:, 2]
    full = cc.model_export(src, clips, out_pcm16)
    res = strided_of(full, np.arange(len(clips)), skips, step, out_pcm16, lens, mutation)
    if mutation == "kept":
        for i, ((l0, C_, a, b), k) in enumerate(zip(clips, skips)):
            pick, best, runner = sc._pick([cc.rms_f32(src[l0 + c, a + int(k):b:step]) for c in range(C_)])
            res["best_channel"][i], res["best_rms"][i], res["runner_up_rms"][i] = pick, best, runner
            res["samples"][i] = cc.convert(src[l0 + pick, a + int(k):b:step], out_pcm16)
    return res


# ------------------------------------------------------------------ the split form
def cuts_of(n, skip, step):
    """the seams of a clip of n samples: clip_split_cases', around the first kept sample, and directly before and after a kept
    sample in the middle"""
    mid = skip + (n // 2 - skip) // step * step
    return sorted({s for s in sc.seams(n) + [skip - 1, skip, skip + 1, mid, mid + 1] if 0 <= s <= n})


class SplitLayout:
    """rows [n][7] uint64 for cuts [(clip index, sigma)] of clips of one stream: the first sigma samples of every channel in A
    [C + 1 lanes], the rest in B [C + 3 lanes], at lanes 1.. and 2.., every piece at its own place with sentinels / NaN around
    it and its first byte rotating through clip_split_cases.FEW_PAIRS' offsets within 16 bytes"""

    def __init__(self, src, clips, cuts):
        pcm16 = src.dtype == np.int16
        per16 = 8 if pcm16 else 4
        C_ = int(clips[cuts[0][0]][1])
        self.a_lanes, self.b_lanes, la, lb = C_ + 1, C_ + 3, 1, 2
        at_a, at_b, places = 1, 1, []
        for i, s in cuts:
            n = int(clips[i][3] - clips[i][2])
            places.append((at_a, at_b))
            at_a += s + per16 + 1
            at_b += n - s + per16 + 1
        self.a_samples, self.b_samples = at_a + per16, at_b + per16
        self.a_stride, self.b_stride = self.a_samples + 3 | 1, self.b_samples + 7 | 1
        fill = cc.SENTINEL if pcm16 else np.nan
        self.A = np.full((self.a_lanes, self.a_stride), fill, src.dtype)
        self.B = np.full((self.b_lanes, self.b_stride), fill, src.dtype)
        rows = []
        for k, ((i, s), (ca, cb)) in enumerate(zip(cuts, places)):
            l0, c_, a, b = (int(v) for v in clips[i])
            assert c_ == C_
            x, y = sc.FEW_PAIRS[k % len(sc.FEW_PAIRS)]
            fa = ca + (x - (la * self.a_stride + ca)) % per16
            fb = cb + (y - (lb * self.b_stride + cb)) % per16
            self.A[la:la + C_, fa:fa + s] = src[l0:l0 + C_, a:a + s]
            self.B[lb:lb + C_, fb:fb + b - a - s] = src[l0:l0 + C_, a + s:b]
            rows.append((C_, la if s else 0, fa if s else 0, s, lb if s < b - a else 0, fb if s < b - a else 0, b - a - s))
        self.rows = np.array(rows, np.uint64)
        self.base = np.array([i for i, _ in cuts])
        self.sigma = np.array([s for _, s in cuts])

    def a(self, address=None):
        return (address, self.a_lanes, self.a_stride, self.a_samples)

    def b(self, address=None):
        return (address, self.b_lanes, self.b_stride, self.b_samples)


def split_case(table, case, src):
    """the case's edge clips at every seam of cuts_of -> (SplitLayout, skips per row)"""
    cuts, skips = [], []
    for i in case.edge:
        a, b = int(table.clips[i, 2]), int(table.clips[i, 3])
        k = phase_skip(a, case.step, case.phase)
        for s in cuts_of(b - a, k, case.step):
            cuts.append((int(i), s))
            skips.append(k)
    return SplitLayout(src, table.clips, cuts), np.array(skips, np.uint32)


def model_export_split_strided(layout, skips, step, out_pcm16, mutation=None):
    """the statement of fvad_clips_export_split_strided in numpy over layout.A / layout.B.  mutation: None | "restart" (the
    stride restarted at the seam: B's piece kept from its own first sample)"""
    full = sc.model_export_split(layout, layout.rows, out_pcm16)
    rows = layout.rows.astype(np.int64)
    res = strided_of(full, np.arange(len(rows)), skips, step, out_pcm16, rows[:, 3] + rows[:, 6])
    if mutation == "restart":
        for i, (r, k) in enumerate(zip(rows, skips)):
            s, na = full["samples"][i], int(r[3])
            if 0 < na < len(s):
                res["samples"][i] = np.concatenate([s[:na][int(k)::step], s[na:][::step]])
    return res
