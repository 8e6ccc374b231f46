"""The model and the case tables of the resampled Recorder tests (fvad_clips_export*_resampled; test_clips_resample_host.py,
test_clips_resample_gpu.py), on top of clip_cases.py's sources and float64 model, clip_split_cases.py's split model,
clip_stride_cases.py's split layout and ingest_resample_cases.py's float64 resampler and bound.

The rule, in numpy float64: a resampled export of a clip at up/down with an odd number of taps (K = (n_taps - 1) / 2) is the
full-rate export's pick and RMS values -- taken over EVERY sample of the UNRESAMPLED clip -- and, of the picked channel x as f32,
zero outside the clip,
    y[o] = sum over n of x[n] * taps[K + o * down - n * up],   o = 0 .. ceil(len * up / down) - 1,
over every n whose tap index lies in [0, 2 K]: ingest_resample_cases.resample_model of the clip as a whole file.  o counts from
the clip's first sample.  Slots are 16-byte aligned, in clip order, sized by out_len.  For a split clip the filter runs through
the seam.

The library sums in f32: beside every y[o] the model gives B[o] = sum |tap| |x| over the same terms, and a device output may
differ from y[o] by g B[o] plus one f32 ulp of y[o], g = n u / (1 - n u), u = 2^-24, n = ceil(n_taps / up)
(ingest_resample_cases.gamma) -- computed, not measured.  `compare` holds a result against that.

The table (`Table`, one per (up, down, half, taps) of CASES): a source of clip_cases' 12 lanes plus a stereo stream E of its own
(channel 1 the quieter), in which the case's own clips lie one behind the other with 1 .. 8 samples of NaN (PCM16: the
sentinel) between them, so that a read outside a clip poisons an output:
- `edge`: clips whose out_len is T_o - 1, T_o, T_o + 1, 2 T_o + 1 and 1 (T_o = tile_out(...), the gather's tile in output samples;
  where up > down leaves no clip of exactly that out_len, the next one above), each starting at each of the 8 sample alignments,
- `short`: clips of 1, 2, R - 1, R, R + 1 and 2 R + 1 samples, R = ceil(K / up) the filter's reach in clip samples, and one of
  R / 2 samples, shorter than the reach on both sides,
- `named`: five clips of clip_cases.case_table(): the source's first and last samples, three and five channels, a tie, silence.
For the split form (`split_case`) one 2 T_o + 1 clip and two short ones are cut 1, R - 1, R, R + 1 samples from either end, inside
the left halo, the body and the right halo of the second tile, and so that a_len, then b_len, is below the reach.

`resampled_of` / `model_export_split` state five wrong versions; test_clips_resample_host.py shows which rows tell each."""
import numpy as np

import clip_cases as cc
import clip_split_cases as sc
import clip_stride_cases as st
import ingest_resample_cases as rr

WINDOW = cc.TILE                 # the clip samples a tile of the gather stages at most
TILE_MAX = 8192                  # outputs per tile at most
UP_MAX, TAPS_MAX = 640, 20481    # FVAD_RESAMPLE_UP_MAX, FVAD_RESAMPLE_TAPS_MAX
# (up, down, half, taps): 32 kHz, two ratios with up and down coprime above 1 on either side of 1, 16 kHz at the default length,
# 44.1 kHz short and at the default length, 11.025 kHz at its shortest
CASES = ((2, 3, 4, "sinc"), (5, 7, 2, "noise"), (7, 5, 2, "sinc"), (1, 3, 16, "sinc"), (147, 160, 2, "noise"), (147, 160, 16, "sinc"),
         (147, 640, 1, "sinc"))
NAMED = ("first", "last", "dup", "tie-D", "silence")
E_LANE, E_CH = cc.N_LANES, 2     # stream E: two lanes behind clip_cases'
N_LANES = cc.N_LANES + E_CH
gamma, U = rr.gamma, rr.U


def out_len(n, up, down):
    return -(-int(n) * up // down)


def tile_out(up, down, n_taps):
    """the resampling gather's tile in OUTPUT samples, by brute force: the most n, in eights, at most TILE_MAX, whose window
    floor(((n - 1) down + 2 K) / up) + 1 fits WINDOW"""
    n = TILE_MAX // 8 * 8
    while n > 0 and ((n - 1) * down + n_taps - 1) // up + 1 > WINDOW:
        n -= 8
    return n


assert tile_out(147, 160, 5121) == 7488 and tile_out(147, 640, 20481) == 1848 and tile_out(1, 3, 97) == 2696


def len_for(L, up, down):
    """the shortest clip with out_len >= L"""
    n = max(1, ((L - 1) * down) // up)
    while out_len(n, up, down) < L:
        n += 1
    return n


def reach(n_taps, up):
    return -(-((n_taps - 1) // 2) // up)


def case_taps(up, down, half, kind):
    """float32 taps: the design rule tilted to one side, so that reversing them shows, or finite noise of the same length"""
    if kind == "noise":
        return rr.case_taps(up, down, half, "noise")
    h = rr.design(up, down, half)
    return (h * (1.0 + 0.5 * np.linspace(-1.0, 1.0, len(h)))).astype(np.float32)


def plan(lens_out, out_pcm16):
    per16 = 8 if out_pcm16 else 4
    offsets, at = [], 0
    for n in lens_out:
        offsets.append(at)
        at += (int(n) + per16 - 1) // per16 * per16
    return np.array(offsets, np.uint64), at


class Table:
    """clips [n][4] uint64: the named clips of clip_cases.case_table(), then the case's edge and short clips in stream E"""

    def __init__(self, up, down, half, kind):
        self.up, self.down, self.half, self.kind = up, down, half, kind
        self.taps = case_taps(up, down, half, kind)
        self.n_taps = len(self.taps)
        self.To, self.R = tile_out(up, down, self.n_taps), reach(self.n_taps, up)
        assert self.To >= 8
        base, names = cc.case_table()
        clips = [tuple(int(v) for v in base[names[k]]) for k in NAMED]
        self.named = np.arange(len(clips))
        edge, short, at = [], [], 0
        for target in (self.To - 1, self.To, self.To + 1, 2 * self.To + 1, 1):
            for i in range(8):
                a = at + 1 + (i - (at + 1)) % 8          # 1 .. 8 guard samples, the start at alignment i
                n = len_for(target, up, down)
                edge.append(len(clips))
                clips.append((E_LANE, E_CH, a, a + n))
                at = a + n
        for j, n in enumerate(sorted({n for n in (1, 2, self.R - 1, self.R, self.R + 1, 2 * self.R + 1, self.R // 2) if n > 0})):
            a = at + 1 + ((3 * j + 1) - (at + 1)) % 8
            short.append(len(clips))
            clips.append((E_LANE, E_CH, a, a + n))
            at = a + n
        self.edge, self.short = np.array(edge), np.array(short)
        self.clips = np.array(clips, np.uint64)
        self.n_samples = max(cc.N_SAMPLES, at + 3)
        self.n_lanes = N_LANES
        self.out_lens = np.array([out_len(b - a, up, down) for _, _, a, b in clips], np.uint64)

    def __repr__(self):
        return f"{self.up}/{self.down}-half{self.half}-{self.kind}"

    def source(self, pcm16, seed=5):
        """[N_LANES][n_samples]: clip_cases' source in its lanes, stream E behind them, NaN / the sentinel outside the clips"""
        rng = np.random.default_rng(seed + 1)
        out = np.zeros((N_LANES, self.n_samples), np.int16 if pcm16 else np.float32)
        out[:cc.N_LANES, :cc.N_SAMPLES] = cc.make_source(pcm16, seed)
        if pcm16:
            x = rng.integers(-15000, 15000, self.n_samples).astype(np.int16)
            out[E_LANE], out[E_LANE + 1] = x, np.rint(x * float(cc.SCALE)).astype(np.int16)
        else:
            x = rng.uniform(-0.45, 0.45, self.n_samples).astype(np.float32)
            out[E_LANE], out[E_LANE + 1] = x, x * cc.SCALE
        return cc.mask_outside(out, self.clips)


def _zero_extended(x64, at, pad):
    """x64 [n][1] lying at samples [at, at + n) of a signal that is zero elsewhere -> (frames, frame_base, file_frames) for
    resample_model, `pad` zeros (fewer in front of sample 0) on either side"""
    front = min(pad, at)
    return np.concatenate([np.zeros((front, 1)), x64, np.zeros((pad, 1))]), at - front, at + len(x64) + pad


def resampled_of(full, channels, taps, up, down, out_pcm16=False, mutation=None, starts=None, To=None):
    """what a resampled export has to give, from the full-rate model result `full` (picks and RMS) and the picked channels' f32
    samples `channels` [per clip].  mutation: None | "reversed" (the taps applied back to front) | "floor" (out_len floored) |
    "lane" (the phase counted from the lane index `starts[i]` of the clip's first sample, not from the clip) | "tile" (the zero
    extension at the edges of the tile's own samples instead of the clip's: To the tile)"""
    t = np.asarray(taps, np.float32)[::-1] if mutation == "reversed" else np.asarray(taps, np.float32)
    ys, bs = [], []
    for i, x in enumerate(channels):
        x64 = cc.as_f32(x).astype(np.float64)[:, None]
        n_out = out_len(len(x), up, down)
        if mutation == "floor":
            n_out = max(len(x) * up // down, 1)
        pad = reach(len(t), up) + 2
        if mutation == "lane":
            a = int(starts[i])
            xs, base, ff = _zero_extended(x64, a, pad)
            y, b = rr.resample_model(xs, t, up, down, out_len(a, up, down), n_out, frame_base=base, file_frames=ff)
        elif mutation == "tile":
            y, b = np.zeros((1, n_out)), np.zeros((1, n_out))
            for o0 in range(0, n_out, To):
                lo, hi = min(len(x), -(-o0 * down // up)), min(len(x), -(-(o0 + To) * down // up))   # the samples between the tile's first output and the next tile's
                n = min(To, n_out - o0)
                if hi > lo:
                    xs, base, ff = _zero_extended(x64[lo:hi], lo, pad)
                    y[:, o0:o0 + n], b[:, o0:o0 + n] = rr.resample_model(xs, t, up, down, o0, n, frame_base=base, file_frames=ff)
        else:
            y, b = rr.resample_model(x64, t, up, down, 0, n_out)
        ys.append(y[0])
        bs.append(b[0])
    offsets, total = plan([len(y) for y in ys], out_pcm16)
    res = {k: np.asarray(full[k]).copy() for k in ("best_channel", "best_rms", "runner_up_rms")}
    res.update(offsets=offsets, total=total, y=ys, bound=bs, up=up, n_taps=len(t), out_lens=np.array([len(y) for y in ys], np.uint64),
               samples=[cc.convert(y.astype(np.float32), out_pcm16) for y in ys])
    return res


def model_export(src, clips, taps, up, down, mutation=None, To=None):
    """the statement of fvad_clips_export_resampled (f32 output) in numpy float64; mutation: resampled_of's"""
    clips = np.asarray(clips, np.int64)
    full = cc.model_export(src, clips, False)
    chans = [src[l0 + p, a:b] for (l0, _, a, b), p in zip(clips, full["best_channel"])]
    return resampled_of(full, chans, taps, up, down, mutation=mutation, starts=clips[:, 2], To=To)


def compare(got, want, what=""):
    """a result with f32 `samples` (the library's, cut from its output, or a model's) against the model's `want`: picks, offsets
    and lengths exact, both RMS within one f32 ulp, every sample within g B[o] + ulp_f32(y[o]) of y[o]"""
    assert np.array_equal(got["best_channel"], want["best_channel"]), (what, "best_channel", np.flatnonzero(got["best_channel"] != want["best_channel"]))
    assert np.array_equal(got["offsets"], want["offsets"]) and got["total"] == want["total"], (what, "offsets")
    for k in ("best_rms", "runner_up_rms"):
        assert cc.within_one_ulp(got[k], want[k]), (what, k)
    for i, (s, y, b) in enumerate(zip(got["samples"], want["y"], want["bound"])):
        rr.compare(s, y, b, want["up"], want["n_taps"], (what, "samples of clip", i))


def failing(got, want):
    """the clips of `got` (a model's result) whose samples `compare` refuses against `want`"""
    bad = []
    for i, (s, y, b) in enumerate(zip(got["samples"], want["y"], want["bound"])):
        try:
            rr.compare(s, y, b, want["up"], want["n_taps"])
        except AssertionError:
            bad.append(i)
    return bad


# ------------------------------------------------------------------ a table that stays in global memory
# The gather keeps a [j][o mod up] table of at most TABLE_LDS entries in LDS beside the window (kClipResampleTableLds of
# csrc/kernels.h); every table of CASES is shorter.  147/640 with half 5: 6401 taps, 44 x 147 = 6468 entries.
TABLE_LDS = 6144
LONG_TABLE = (147, 640, 5, "sinc")


def long_table_case(pcm16, seed=7):
    """the smallest shape that takes the gather with the table in global memory through a full tile, a last tile and a seam
    inside a tile -> (src [2][n], clips [1][4], SplitLayout): two lanes, channel 1 the quieter, one clip of WINDOW + 3 samples
    from the odd sample 1 (two gather tiles), NaN / the sentinel around it; the split form's seam at sample WINDOW + 1 of the
    clip, which only the second tile's window holds"""
    n = WINDOW + 3
    rng = np.random.default_rng(seed)
    if pcm16:
        x = rng.integers(-15000, 15000, n + 3).astype(np.int16)
        src = np.stack([x, np.rint(x * float(cc.SCALE)).astype(np.int16)])
    else:
        x = rng.uniform(-0.45, 0.45, n + 3).astype(np.float32)
        src = np.stack([x, x * cc.SCALE])
    clips = np.array([(0, 2, 1, 1 + n)], np.uint64)
    src = cc.mask_outside(src, clips)
    return src, clips, st.SplitLayout(src, clips, [(0, WINDOW + 1)])


# ------------------------------------------------------------------ the split form
def cuts_of(n, up, down, R, To):
    """the seams of a clip of n samples"""
    c2 = To * down // up                                           # the clip sample under the second tile's first output
    c3 = 2 * To * down // up                                       # ... and under the third's
    s = [0, n, 1, R - 1, R, R + 1, n - 1, n - R + 1, n - R, n - R - 1, n // 2, c2 - max(R // 2, 1), c2, c2 + (To // 2) * down // up,
         c3 + max(R // 2, 1), c3 - 1, max(R // 2, 1), n - max(R // 2, 1)]
    return sorted({int(v) for v in s if 0 <= v <= n})


def split_case(table, src):
    """one 2 T_o + 1 clip and the table's two longest short clips at every seam of cuts_of -> SplitLayout"""
    picks = [int(table.edge[24 + 3])] + [int(k) for k in table.short[-2:]]
    cuts = []
    for i in picks:
        n = int(table.clips[i, 3] - table.clips[i, 2])
        cuts += [(i, s) for s in cuts_of(n, table.up, table.down, table.R, table.To)]
    return st.SplitLayout(src, table.clips, cuts)


def model_export_split(layout, taps, up, down, mutation=None):
    """the statement of fvad_clips_export_split_resampled (f32 output) in numpy over layout.A / layout.B.  mutation: None |
    "restart" (the phase restarted at the seam: each piece resampled as a clip of its own, out_len kept)"""
    full = sc.model_export_split(layout, layout.rows, False)
    chans = [cc.as_f32(s) for s in full["samples"]]                # the picked channel, A's piece then B's
    res = resampled_of(full, chans, taps, up, down)
    if mutation == "restart":
        for i, r in enumerate(layout.rows.astype(np.int64)):
            x, na = chans[i], int(r[3])
            if 0 < na < len(x):
                pieces = [rr.resample_model(p.astype(np.float64)[:, None], taps, up, down, 0, out_len(len(p), up, down))[0][0] for p in (x[:na], x[na:])]
                y = np.concatenate(pieces + [np.zeros(2)])[:len(res["y"][i])]
                res["samples"][i] = y.astype(np.float32)
    return res
