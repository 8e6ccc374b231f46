"""The model and the case tables of the filtered Recorder tests (fvad_clips_export*_fir; test_clips_fir_host.py,
test_clips_fir_gpu.py), on top of clip_cases.py's sources and float64 model and clip_stride_cases.py's slots and split layout.

The rule, in numpy float64: a filtered export of a clip with `skip` < `step` and an odd number of taps (H = (n_taps - 1) / 2) is
the full-rate export's pick and RMS values -- taken over EVERY sample of the UNFILTERED clip -- and, of the picked channel x as
f32, zero-extended on both sides,
    y[q] = sum_k taps[k] * x[c + k - H],   c = skip + q * step,   q = 0 .. ceil((len - skip) / step) - 1,
i.e. the centres [skip::step] of the full-rate clip filtered as a finite signal (`fir_centres` computes only those centres).
Slots are the strided export's.  For a split clip the filter runs through the seam.

The library sums in f32: beside every y[q] the model gives B[q] = sum_k |taps[k]| |x[c + k - H]|, and a device output may differ
from y[q] by g B[q] plus one f32 ulp of y[q], g = n u / (1 - n u), u = 2^-24, n = n_taps -- the bound of an n-term fma chain in
any order (taps and samples are f32 exactly, so there is no other error).  `compare` holds a result against that.

The table (`Table`): per (step, H) of CASES and per phase 0 .. step - 1 a `Case` with asymmetric taps and
- the clips whose out_len is T_o - 1, T_o, T_o + 1, 2 T_o + 1 and 1 (T_o = tile_out(step, H), the gather's tile in output samples),
  each starting at each of the 8 sample alignments, with 0 .. step - 1 samples behind the last kept one (`edge`),
- clips of 1, 2, H - 1, H, H + 1 and 2 H + 1 samples (`short`); those with len <= skip keep no sample: the `refused` list,
- five clips of clip_cases.case_table(): the source's first and last samples, three and five channels, a tie, silence (`named`).
For the split form (`split_case`) one 2 T_o + 1 clip and two short ones per case are cut 1, H - 1, H, H + 1 samples from either
end, directly before, at and after a kept sample, inside the left halo, the body and the right halo of the second tile, and
where a_len < H and where b_len < H.

`model_export_fir` / `model_export_split_fir` state five wrong versions; test_clips_fir_host.py shows that the table fails each."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import clip_cases as cc
import clip_split_cases as sc
import clip_stride_cases as st

TILE = cc.TILE
TAPS_MAX = 513                   # FVAD_CLIP_FIR_TAPS_MAX
CASES = ((1, 2), (2, 5), (3, 48), (6, 7), (16, 256))
NAMED = ("first", "last", "dup", "tie-D", "silence")
U = 2.0 ** -24


def tile_out(step, H):
    """the filtered gathers' tile in OUTPUT samples: its (T_o - 1) step + 1 + 2 H source samples fit TILE"""
    return ((TILE - 2 * H - 1) // step + 1) // 8 * 8


assert tile_out(3, 48) == 2696 and tile_out(16, 256) == 480


def design(step, half=0, cutoff=0.0, beta=0.0):
    """fvad_clips_fir_design's statement in numpy float64 (np.kaiser, np.sinc) -> float64 taps of unit sum, before the rounding"""
    half = half or 16 * step
    cutoff = cutoff or 0.45 / step
    beta = beta or 6.0
    k = np.arange(2 * half + 1, dtype=np.float64) - half
    h = 2 * cutoff * np.sinc(2 * cutoff * k) * np.kaiser(2 * half + 1, beta)
    return h / h.sum()


def response(taps, f):
    """|H(f)| of the taps in float64, f in cycles per input sample"""
    t = np.asarray(taps, np.float64)
    k = np.arange(len(t), dtype=np.float64)
    return np.abs(np.exp(-2j * np.pi * np.outer(np.atleast_1d(f), k)) @ t)


def case_taps(step, H):
    """float32 taps of the table's cases: a windowed sinc tilted to one side, so that reversing them shows"""
    h = design(step, half=H, cutoff=0.45 / step) * (1.0 + 0.5 * np.linspace(-1.0, 1.0, 2 * H + 1))
    return h.astype(np.float32)


def gamma(n_taps):
    return n_taps * U / (1 - n_taps * U)


def fir_centres(x, taps, skip, step, replicate=False):
    """x float64 [len], taps [n] -> (y, B) float64 at the centres skip, skip + step, ... of the zero-extended clip"""
    t = np.asarray(taps, np.float64)
    H = (len(t) - 1) // 2
    xp = np.pad(np.asarray(x, np.float64), H, mode="edge" if replicate else "constant")
    win = sliding_window_view(xp, len(t))[int(skip)::step]      # the window of centre c is xp[c : c + n] = x[c - H : c + H + 1]
    return win @ t, np.abs(win) @ np.abs(t)


class Case:
    def __init__(self, step, H, phase, idx, refused, edge, short, named):
        self.step, self.H, self.phase, self.idx, self.refused, self.edge, self.short, self.named = step, H, phase, idx, refused, edge, short, named
        self.taps = case_taps(step, H)

    def __repr__(self):
        return f"step{self.step}-H{self.H}-phase{self.phase}"


class Table:
    """clips [n][4] uint64: the named clips of clip_cases.case_table(), then every case's own; a case computes its skips"""

    def __init__(self):
        base, names = cc.case_table()
        clips = [tuple(int(v) for v in base[names[k]]) for k in NAMED]
        named = list(range(len(clips)))
        l0, C_ = cc.STREAMS[st.EDGE_STREAM]
        z0 = cc.zones(st.EDGE_STREAM)[st.EDGE_ZONE][0]
        self.cases = []
        for step, H in CASES:
            To = tile_out(step, H)
            for phase in range(step):
                edge, short = [], []
                for j, target in enumerate((To - 1, To, To + 1, 2 * To + 1, 1)):
                    for i in range(8):
                        a = z0 + 16 * j + i
                        n = st.phase_skip(a, step, phase) + (target - 1) * step + 1 + (i + j) % step
                        edge.append(len(clips))
                        clips.append((l0, C_, a, a + n))
                for j, n in enumerate(sorted({n for n in (1, 2, H - 1, H, H + 1, 2 * H + 1) if n > 0})):
                    a = z0 + 20000 + 37 * j + j % 8
                    short.append(len(clips))
                    clips.append((l0, C_, a, a + n))
                mine = named + edge + short
                ok = [k for k in mine if clips[k][3] - clips[k][2] > st.phase_skip(clips[k][2], step, phase)]
                refused = [k for k in mine if k not in ok]
                self.cases.append(Case(step, H, phase, np.array(ok), np.array(refused, int), np.array(edge),
                                       np.array([k for k in short if k in ok]), np.array([k for k in named if k in ok])))
        self.clips = np.array(clips, np.uint64)
        assert int(self.clips[:, 3].max()) <= cc.N_SAMPLES

    def source(self, pcm16, seed=5):
        return cc.mask_outside(cc.make_source(pcm16, seed), self.clips)

    def skips(self, case, idx=None):
        idx = case.idx if idx is None else idx
        return np.array([st.phase_skip(self.clips[k, 2], case.step, case.phase) for k in idx], np.uint32)


def _slots(lens_out, out_pcm16):
    per16 = 8 if out_pcm16 else 4
    offsets, at = [], 0
    for n in lens_out:
        offsets.append(at)
        at += (int(n) + per16 - 1) // per16 * per16
    return np.array(offsets, np.uint64), at


def fir_of(full, channels, skips, step, taps, out_pcm16=False, mutation=None):
    """what a filtered export has to give, from the full-rate model result `full` (picks and RMS) and the picked channels' f32
    samples `channels` [per clip].  mutation: None | "reversed" (the taps applied back to front) | "skip0" (the centres counted
    from the clip's first sample) | "replicate" (the edge samples repeated in place of the zeros)"""
    t = np.asarray(taps, np.float32)[::-1] if mutation == "reversed" else np.asarray(taps, np.float32)
    ys, bs = [], []
    for x, k in zip(channels, skips):
        y, b = fir_centres(cc.as_f32(x), t, 0 if mutation == "skip0" else int(k), step, replicate=mutation == "replicate")
        if mutation == "skip0":
            y, b = y[:st.out_len(len(x), k, step)], b[:st.out_len(len(x), k, step)]
        ys.append(y)
        bs.append(b)
    offsets, total = _slots([len(y) for y in ys], out_pcm16)
    res = {k: np.asarray(full[k]).copy() for k in ("best_channel", "best_rms", "runner_up_rms")}
    res.update(offsets=offsets, total=total, y=ys, bound=bs, n_taps=len(t), samples=[cc.convert(y.astype(np.float32), out_pcm16) for y in ys])
    return res


def model_export_fir(src, clips, skips, step, taps, mutation=None):
    """the statement of fvad_clips_export_fir (f32 output) in numpy float64.  mutation: fir_of's, or "filtered" (RMS and pick
    over the filtered samples)"""
    clips = np.asarray(clips, np.int64)
    full = cc.model_export(src, clips, False)
    res = fir_of(full, [src[l0 + p, a:b] for (l0, _, a, b), p in zip(clips, full["best_channel"])], skips, step, taps,
                 mutation=None if mutation == "filtered" else mutation)
    if mutation == "filtered":
        for i, ((l0, C_, a, b), k) in enumerate(zip(clips, skips)):
            r = [cc.rms_f32(fir_centres(cc.as_f32(src[l0 + c, a:b]), taps, k, step)[0].astype(np.float32)) for c in range(C_)]
            res["best_channel"][i], res["best_rms"][i], res["runner_up_rms"][i] = sc._pick(r)
            res["y"][i], res["bound"][i] = fir_centres(cc.as_f32(src[l0 + res["best_channel"][i], a:b]), taps, k, step)
            res["samples"][i] = res["y"][i].astype(np.float32)
    return res


def compare(got, want, what=""):
    """a result with f32 `samples` (the library's, cut from its output, or a model's) against the model's `want`: picks and
    offsets exact, both RMS within one f32 ulp, every sample within g B[q] + ulp_f32(y[q]) of y[q]"""
    assert np.array_equal(got["best_channel"], want["best_channel"]), (what, "best_channel", np.flatnonzero(got["best_channel"] != want["best_channel"]))
    assert np.array_equal(got["offsets"], want["offsets"]) and got["total"] == want["total"], (what, "offsets")
    for k in ("best_rms", "runner_up_rms"):
        assert cc.within_one_ulp(got[k], want[k]), (what, k)
    g = gamma(want["n_taps"])
    for i, (s, y, b) in enumerate(zip(got["samples"], want["y"], want["bound"])):
        assert s.dtype == np.float32 and s.shape == y.shape, (what, "samples of clip", i, s.shape, y.shape)
        tol = g * b + np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
        err = np.abs(s.astype(np.float64) - y)
        assert np.all(err <= tol), (what, "samples of clip", i, "at", int(np.argmax(err - tol)), float(np.max(err - tol)))


# ------------------------------------------------------------------ the split form
def cuts_of(n, skip, step, H, To):
    """the seams of a clip of n samples"""
    mid = skip + (n // 2 - skip) // step * step                  # a kept sample in the middle
    c2 = skip + To * step                                         # the centre of the second tile's first output
    s = [0, n, 1, H - 1, H, H + 1, n - 1, n - H + 1, n - H, n - H - 1, mid - 1, mid, mid + 1, skip, skip + 1,
         c2 - H + H // 2, c2 - H, c2, c2 + 5 * step + 1, c2 + (To // 2) * step, n - H // 2 - 1, max(H // 2, 1), n - max(H // 2, 1)]
    return sorted({int(v) for v in s if 0 <= v <= n})


def split_case(table, case, src):
    """one 2 T_o + 1 clip (its alignment rotates with the phase) and the case's two longest short clips at every seam of cuts_of
    -> (SplitLayout, skips per row)"""
    To = tile_out(case.step, case.H)
    picks = [int(case.edge[24 + case.phase % 8])] + [int(k) for k in case.short[-2:]]
    cuts, skips = [], []
    for i in picks:
        a, b = int(table.clips[i, 2]), int(table.clips[i, 3])
        k = st.phase_skip(a, case.step, case.phase)
        for s in cuts_of(b - a, k, case.step, case.H, To):
            cuts.append((i, s))
            skips.append(k)
    return st.SplitLayout(src, table.clips, cuts), np.array(skips, np.uint32)


def model_export_split_fir(layout, skips, step, taps, mutation=None):
    """the statement of fvad_clips_export_split_fir (f32 output) in numpy over layout.A / layout.B.  mutation: None | "restart"
    (the filter restarted at the seam: each piece filtered as a finite signal of its own)"""
    full = sc.model_export_split(layout, layout.rows, False)
    chans = [cc.as_f32(s) for s in full["samples"]]                # the picked channel, A's piece then B's
    res = fir_of(full, chans, skips, step, taps)
    if mutation == "restart":
        for i, (r, k) in enumerate(zip(layout.rows.astype(np.int64), skips)):
            x, na = chans[i], int(r[3])
            if 0 < na < len(x):
                ya = fir_centres(x[:na], taps, 0, 1)[0]
                yb = fir_centres(x[na:], taps, 0, 1)[0]
                res["y"][i] = np.concatenate([ya, yb])[int(k)::step]
                res["samples"][i] = res["y"][i].astype(np.float32)
    return res
