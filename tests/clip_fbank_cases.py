"""The yardstick, the units and the case table of the filter-bank clip tests (fvad_clips_export_fbank*; test_clips_fbank_host.py,
test_clips_fbank_gpu.py, test_clips_fbank_harness_gpu.py).  Signals, `pick`, `clip_stream` and `distance` are clip_mel_cases.py's.

The rule, in numpy (include/fvad.h, "Kaldi-style filter-bank features"): of a clip's quietest channel the stream
s[i] = f32(f32(sample skip + i * step) * scale), L = ceil((len - skip) / step) of them; T = 1 + (L - win) // hop frames
x = s[t * hop : t * hop + win] (snip_edges: no tap leaves the stream); d = x - mean(x) (remove_dc); y[i] = d[i] - preemph * d[i - 1]
with d[-1] = d[0]; z = y * w, zero-padded to n_fft; P = |rfft(z)|^2; mel = M @ P; feat = ln(max(mel, floor)).

The reference is float64 throughout (`model`), on exactly the f32 stream (the scaled product rounded once, as the rule has it),
window, matrix, preemph and floor the kernel is given.  A feature counts in units of
    U = [ eps * sum_k |M[m][k]| (2 |X_k| X2 + P_k)  +  sum_k |M[m][k]| 2 |X_k| E2 ] / max(mel, floor)  +  eps * max(|feat|, 1)
with eps = 2^-24: the first term is clip_mel_cases' unit on the conditioned frame's spectrum (X2 the 2-norm of the spectrum; the
logarithm is natural, so no ln 10), the second carries the conditioning's own rounding to the taps: per tap it is bounded by
    e_i = eps |w_i| (|x_i| + |mean| + |d_i| + preemph |d_{i-1}| + |y_i|)
-- the roundings of the mean, the difference, the product, the second difference and the windowing -- and a tap-error vector e
moves a bin by at most its 2-norm E2, so P_k by 2 |X_k| E2.

The tolerance TOL is four times the worst distance of a plain float32 evaluation of the same steps (`f32_eval`) over
`case_table()`.  F32_WORST is that distance, measured on the CPU and committed as a literal; test_clips_fbank_host.py asserts that
the measurement still gives it."""
import numpy as np

import clip_mel_cases as mc
from clip_mel_cases import EPS, TILE, TILE_FRAMES, clip_stream, distance, phase_skip, pick, to_f32  # noqa: F401  (shared with the tests)

FLOOR = np.float32(2.0 ** -23)   # FLT_EPSILON, Kaldi's floor of an energy
PREEMPH = np.float32(0.97)
SHAPES = [(400, 512, 160, 80), (512, 512, 128, 128), (6, 8, 4, 3), (4, 4, 1, 1), (5, 8, 2, 2)]  # (win, n_fft, hop, n_mels)
TABLE_SHAPES = SHAPES[:3]
SCALES = (1.0, 32768.0)
SIGNALS = mc.SIGNALS + ("noise0.01+dc0.1",)

# the worst distance of f32_eval from the float64 model over case_table(), in units U:
# measured 2026-10-21 with `python tests/clip_fbank_cases.py` (numpy 2.2, single-precision pocketfft)
F32_WORST = 0.8390
TOL = 4 * F32_WORST


def tile_frames(win, hop):
    """frames per workgroup: the tile's window (F - 1) hop + win fits TILE staged samples, at most TILE_FRAMES"""
    return min((TILE - win) // hop + 1, TILE_FRAMES)


def povey(n):
    """Kaldi's default window, float64 rounded once"""
    return ((0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / (n - 1))) ** 0.85).astype(np.float32)


def hamming(n):
    """Kaldi's "hamming" window, float64 rounded once.  Its ends are 0.08, not 0 as Povey's: only under such a window does a
    frame's first tap -- Kaldi's replicated first sample -- reach the features at all"""
    return (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n) / (n - 1))).astype(np.float32)


def window_for(shape):
    """the harness's shape under the harness's window, every other shape under Hamming"""
    return povey(shape[0]) if shape == SHAPES[0] else hamming(shape[0])


def design(sr, n_fft, n_mels, low, high):
    """Kaldi's bank written out: HTK mel, triangles in the mel domain, no normalisation, a zero Nyquist column; float64,
    rounded once"""
    def to_mel(f):
        return 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)
    if high <= 0:
        high = sr / 2 + high
    pts = to_mel(low) + (to_mel(high) - to_mel(low)) * np.arange(n_mels + 2) / (n_mels + 1)
    mk = to_mel(np.arange(n_fft // 2) * (sr / n_fft))
    M = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        l, c, r = pts[m], pts[m + 1], pts[m + 2]
        M[m, :n_fft // 2] = np.maximum(0.0, np.minimum((mk - l) / (c - l), (r - mk) / (r - c)))
    return M.astype(np.float32)


def matrix_for(shape):
    _, n_fft, _, n_mels = shape
    return design(16000.0, n_fft, n_mels, 20.0, 0.0)


def n_frames(L, win, hop):
    return 0 if L < win else 1 + (L - win) // hop


def frame_index(L, win, hop, mutation=None):
    """[T][win] indices into the stream.  mutation: "centred" (frames centred with reflection, T = L // hop as the log-mel export
    has them), "lastframe" (the last frame dropped)"""
    if mutation == "centred":
        j = np.arange(L // hop)[:, None] * hop + np.arange(win)[None, :] - win // 2
        j = np.where(j < 0, -j, np.where(j >= L, 2 * (L - 1) - j, j))
        return np.clip(j, 0, L - 1)
    T = n_frames(L, win, hop) - (1 if mutation == "lastframe" else 0)
    return np.arange(T)[:, None] * hop + np.arange(win)[None, :]


def scaled(s, scale):
    """the stream as the kernel conditions it: one rounded f32 product"""
    out = np.asarray(s, np.float32) * np.float32(scale)
    assert out.dtype == np.float32
    return out


def condition(x, w, n_fft, preemph, remove_dc, mutation=None):
    """frames x [T][win] (any float type: the arithmetic runs in x's) -> (z [T][n_fft], the pieces the unit needs).  mutation:
    "y0" (y[0] = d[0]), "pre-first" (pre-emphasis before the DC removal), "mean-nfft" (the mean over n_fft), "win-first" (the
    window before the pre-emphasis)"""
    ft = x.dtype.type
    win = x.shape[1]
    p, w = ft(preemph), np.asarray(w).astype(x.dtype)

    def pre(v):
        prev = np.concatenate([v[:, :1], v[:, :-1]], axis=1)
        out = v - p * prev
        if mutation == "y0":
            out[:, 0] = v[:, 0]
        return out, prev

    def dc(v):
        mean = v.sum(axis=1, dtype=x.dtype)[:, None] / ft(n_fft if mutation == "mean-nfft" else win)
        return (v - mean if remove_dc else v), (mean if remove_dc else np.zeros_like(mean))
    if mutation == "pre-first":
        y, prev = pre(x)
        y, mean = dc(y)
        d = y
    elif mutation == "win-first":
        d, mean = dc(x)
        y, prev = pre(d * w)
    else:
        d, mean = dc(x)
        y, prev = pre(d)
    z = np.zeros((x.shape[0], n_fft), x.dtype)
    z[:, :win] = y if mutation == "win-first" else y * w
    return z, dict(x=x, mean=mean, d=d, prev=prev, y=y)


def model(s, w, M, shape, scale=1.0, preemph=PREEMPH, remove_dc=True, floor=FLOOR, mutation=None):
    """float64 features [T][n_mels] of the stream s (float32, unscaled) and their units U"""
    win, n_fft, hop, _ = shape
    xs = scaled(s, scale).astype(np.float64)
    x = xs[frame_index(len(xs), win, hop, mutation)]
    z, c = condition(x, w, n_fft, np.float64(np.float32(preemph)), remove_dc, mutation)
    X = np.fft.rfft(z, axis=1)
    P = X.real ** 2 + X.imag ** 2
    Md = np.asarray(M, np.float64)
    mel = np.maximum(P @ Md.T, np.float64(np.float32(floor)))
    feat = np.log10(mel) if mutation == "log10" else np.log(mel)
    X2 = np.sqrt(P.sum(axis=1))[:, None]
    wd = np.abs(np.asarray(w, np.float64))
    e = EPS * wd * (np.abs(c["x"]) + np.abs(c["mean"]) + np.abs(c["d"]) + float(np.float32(preemph)) * np.abs(c["prev"]) + np.abs(c["y"]))
    E2 = np.sqrt((e * e).sum(axis=1))[:, None]
    U = (EPS * ((2 * np.abs(X) * X2 + P) @ np.abs(Md).T) + (2 * np.abs(X) * E2) @ np.abs(Md).T) / mel + EPS * np.maximum(np.abs(feat), 1.0)
    return feat, U


def f32_eval(s, w, M, shape, scale=1.0, preemph=PREEMPH, remove_dc=True, floor=FLOOR):
    """the same steps in plain float32: numpy's sums, single-precision rfft, f32 power, f32 matmul, f32 log"""
    win, n_fft, hop, _ = shape
    xs = scaled(s, scale)
    z, _ = condition(xs[frame_index(len(xs), win, hop)], np.asarray(w, np.float32), n_fft, np.float32(preemph), remove_dc)
    assert z.dtype == np.float32
    X = np.fft.rfft(z, axis=1)
    assert X.dtype == np.complex64, "numpy computes the rfft of float32 in double here"
    P = X.real * X.real + X.imag * X.imag
    mel = np.maximum(P @ np.asarray(M, np.float32).T, np.float32(floor))
    assert mel.dtype == np.float32
    return np.log(mel)


def model_clip(lanes, sample_from, step, phase, shape, w, M, mutation=None, **kw):
    """the float64 model of one clip whose first sample has lane index sample_from.  mutation: model's, condition's and
    frame_index's, or "phase1" (the skips of phase 1 where the case has phase 2), "loud" (the loudest channel picked)"""
    skip = phase_skip(sample_from, step, 1 if mutation == "phase1" and step > 1 else phase)
    ch = None
    if mutation == "loud":
        ch = max(range(len(lanes)), key=lambda c: float((to_f32(lanes[c]).astype(np.float64) ** 2).sum()))
    _, s = clip_stream(lanes, step, skip, ch)
    return model(s, w, M, shape, mutation=mutation, **kw)


# ------------------------------------------------------------------ the case table: signals x shapes x scales, two-channel clips at step 3
def signal(name, L, rng):
    if name == "noise0.01+dc0.1":
        return (0.1 + 0.01 * rng.standard_normal(L)).astype(np.float32)
    return mc.signal(name, L, rng)


class Case:
    """a clip of two channels at step 3, phase 2: channel 1 carries the signal on its kept samples and noise of the signal's
    size between them; channel 0 is four times as loud"""

    def __init__(self, shape, name, scale, seed):
        self.shape, self.name, self.scale = shape, name, scale
        win, n_fft, hop, _ = shape
        rng = np.random.default_rng(seed)
        self.step, self.phase, self.sample_from = 3, 2, 7 + seed % 3
        L = 9 * hop + win + hop // 2
        s = signal(name, L, rng)
        skip = phase_skip(self.sample_from, self.step, self.phase)
        n = skip + (L - 1) * self.step + 1 + seed % self.step
        size = max(float(np.abs(s).max()), 1e-4)
        quiet = (size * 0.5 * rng.standard_normal(n)).astype(np.float32)
        quiet[skip::self.step] = s
        loud = (4 * size * rng.standard_normal(n) + 4 * np.resize(s, n)).astype(np.float32)
        self.lanes = np.stack([loud, quiet])
        self.w, self.M = window_for(shape), matrix_for(shape)

    def __repr__(self):
        return f"{'/'.join(map(str, self.shape))}-{self.name}-x{self.scale:g}"

    def stream(self):
        return clip_stream(self.lanes, self.step, phase_skip(self.sample_from, self.step, self.phase))[1]

    def model(self, mutation=None):
        return model_clip(self.lanes, self.sample_from, self.step, self.phase, self.shape, self.w, self.M, mutation, scale=self.scale)

    def f32(self):
        return f32_eval(self.stream(), self.w, self.M, self.shape, scale=self.scale)


def case_table():
    return [Case(shape, name, scale, 11 * i + j) for i, shape in enumerate(TABLE_SHAPES) for j, name in enumerate(SIGNALS) for scale in SCALES]


def f32_worst(table=None):
    worst = 0.0
    for c in table or case_table():
        ref, U = c.model()
        worst = max(worst, distance(c.f32(), ref, U))
    return worst


if __name__ == "__main__":
    for c in case_table():
        ref, U = c.model()
        print(f"{c!r:48s} {distance(c.f32(), ref, U):8.4f}")
    print(f"F32_WORST = {f32_worst():.4f}")
