"""The yardstick, the units and the case table of the log-mel clip tests (fvad_clips_export_mel*; test_clips_mel_host.py,
test_clips_mel_gpu.py, test_clips_mel_harness_gpu.py).

The rule, in numpy (include/fvad.h, "batch Recorder with a front end"): of a clip's quietest channel the stream
s[i] = f32(sample skip + i * step), L = ceil((len - skip) / step) of them; T = L // hop frames of n_fft taps, frame t tap i
reading s[rho(t * hop + i - n_fft / 2)] with rho(j) = -j below 0 and 2 (L - 1) - j from L on; P = |rfft(frame * w)|^2;
mel = M @ P; feat = log10(max(mel, floor)).

The reference is float64 throughout (`model`), on exactly the f32 samples, window, matrix and floor the kernel is given.  With
eps = 2^-24 and X2 the 2-norm of the frame's reference spectrum, a feature counts in units of
    U = eps * sum_k |M[m][k]| (2 |X_k| X2 + P_k) / (ln 10 * max(mel, floor)) + eps * max(|feat|, 1)
-- an f32 transform leaves every bin with an error of a few eps of the frame's whole energy, |dX_k| ~ eps X2, so
dP_k ~ 2 |X_k| dX_k, weighted by the matrix and carried through the logarithm, plus the rounding of the result itself.  Relative
to the frame's energy, as K4's units are.  The tolerance TOL is four times the worst distance of a plain float32 evaluation
(`f32_eval`: numpy's single-precision rfft, f32 power, f32 matmul, f32 log10) over `case_table()`: room for another summation
order and another FFT factorisation, which the K4 tests showed to cost the same order; an indexing mistake costs hundreds.

F32_WORST is that worst distance, measured on the CPU and committed as a literal; test_clips_mel_host.py asserts that the
measurement still gives it."""
import numpy as np

EPS = 2.0 ** -24
FLOOR = np.float32(1e-10)
SHAPES = [(400, 160, 80), (512, 128, 128), (8, 4, 3), (4, 1, 1), (254, 100, 5), (2048, 512, 40)]  # (n_fft, hop, n_mels)
TABLE_SHAPES = SHAPES[:3]
TILE, TILE_FRAMES = 8192, 32     # kClipTile (kFeatSrcTile), kFeatTileFrames

# the worst distance of f32_eval from the float64 model over case_table(), in units U:
# measured 2026-10-20 with `python tests/clip_mel_cases.py` (numpy 2.2, single-precision pocketfft)
F32_WORST = 1.6097
TOL = 4 * F32_WORST


def tile_frames(n_fft, hop):
    """frames per workgroup: the tile's window (F - 1) hop + n_fft fits TILE staged samples, at most TILE_FRAMES"""
    return min((TILE - n_fft) // hop + 1, TILE_FRAMES)


def hann(n):
    """the periodic Hann window, float32"""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)


def design(sr, n_fft, n_mels, fmin, fmax):
    """Slaney's filter bank written out: float64, rounded once"""
    def to_mel(f):
        f = np.asarray(f, np.float64)
        return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))

    def to_hz(m):
        m = np.asarray(m, np.float64)
        return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)))
    edges = to_hz(to_mel(fmin) + (to_mel(fmax) - to_mel(fmin)) * np.arange(n_mels + 2) / (n_mels + 1))
    fk = np.arange(n_fft // 2 + 1) * (sr / n_fft)
    M = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        up = (fk - edges[m]) / (edges[m + 1] - edges[m])
        down = (edges[m + 2] - fk) / (edges[m + 2] - edges[m + 1])
        M[m] = np.maximum(0.0, np.minimum(up, down)) * (2.0 / (edges[m + 2] - edges[m]))
    return M.astype(np.float32)


def matrix_for(shape):
    n_fft, _, n_mels = shape
    return design(16000.0, n_fft, n_mels, 0.0, 8000.0)


def to_f32(lane):
    """a lane's samples as the kernels read them"""
    return lane.astype(np.float32) / np.float32(32768.0) if lane.dtype == np.int16 else lane.astype(np.float32)


def pick(lanes):
    """Recorder.findBestChannel over EVERY sample of the clip: rms = f32(sqrt(sum / n)) in float64, strict <, from 9999"""
    best, best_vol = 0, np.float32(9999.0)
    for c, lane in enumerate(lanes):
        x = to_f32(lane).astype(np.float64)
        vol = np.float32(np.sqrt((x * x).sum() / len(x)))
        if vol < best_vol:
            best, best_vol = c, vol
    return best


def phase_skip(sample_from, step, phase):
    return (phase + step - int(sample_from) % step) % step


def frame_index(L, n_fft, hop, mutation=None):
    """[T][n_fft] indices into the stream.  mutation: "edge" (the reflection repeats the edge sample), "late" (every frame
    starts one sample late), "lastframe" (the last frame dropped)"""
    T = L // hop - (1 if mutation == "lastframe" else 0)
    j = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :] - n_fft // 2 + (1 if mutation == "late" else 0)
    if mutation == "edge":
        j = np.where(j < 0, -j - 1, np.where(j >= L, 2 * L - 1 - j, j))
    else:
        j = np.where(j < 0, -j, np.where(j >= L, 2 * (L - 1) - j, j))
    return np.clip(j, 0, L - 1)  # (only a mutation can leave the stream)


def model(s, w, M, hop, floor=FLOOR, mutation=None):
    """float64 features [T][n_mels] of the stream s (float32) and their units U"""
    s = np.asarray(s, np.float32).astype(np.float64)
    n_fft = len(w)
    X = np.fft.rfft(s[frame_index(len(s), n_fft, hop, mutation)] * np.asarray(w, np.float64), axis=1)
    P = X.real ** 2 + X.imag ** 2
    Md = np.asarray(M, np.float64)
    if mutation == "row":
        Md = np.roll(Md, -1, axis=0)
    mel = np.maximum(P @ Md.T, np.float64(np.float32(floor)))
    feat = np.log10(mel)
    X2 = np.sqrt(P.sum(axis=1))[:, None]
    U = EPS * ((2 * np.abs(X) * X2 + P) @ np.abs(Md).T) / (np.log(10.0) * mel) + EPS * np.maximum(np.abs(feat), 1.0)
    return feat, U


def f32_eval(s, w, M, hop, floor=FLOOR):
    """the same in plain float32: numpy's single-precision rfft, f32 power, f32 matmul, f32 log10"""
    s = np.asarray(s, np.float32)
    X = np.fft.rfft(s[frame_index(len(s), len(w), hop)] * np.asarray(w, np.float32), axis=1)
    assert X.dtype == np.complex64, "numpy computes the rfft of float32 in double here: use the oracle's orc_fftr_forward"
    P = X.real * X.real + X.imag * X.imag
    mel = np.maximum(P @ np.asarray(M, np.float32).T, np.float32(floor))
    assert mel.dtype == np.float32
    return np.log10(mel)


def distance(got, ref, U):
    """the largest |got - ref| in units"""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.abs(got.astype(np.float64) - ref) / U).max()) if got.size else 0.0


def clip_stream(lanes, step, skip, channel=None):
    """the feature stream of a clip given as its lanes [C][len]: (picked channel, s)"""
    ch = pick(lanes) if channel is None else channel
    return ch, to_f32(lanes[ch][skip::step])


def model_clip(lanes, sample_from, step, phase, shape, w, M, mutation=None):
    """the float64 model of one clip whose first sample has lane index sample_from.  mutation: model's and frame_index's, or
    "phase1" (the skips of phase 1 where the case has phase 2), "loud" (the loudest channel picked)"""
    skip = phase_skip(sample_from, step, 1 if mutation == "phase1" and step > 1 else phase)
    ch = None
    if mutation == "loud":
        ch = max(range(len(lanes)), key=lambda c: float((to_f32(lanes[c]).astype(np.float64) ** 2).sum()))
    _, s = clip_stream(lanes, step, skip, ch)
    return model(s, w, M, shape[1], mutation=mutation)


# ------------------------------------------------------------------ the case table: signals x shapes, as two-channel clips at step 3
SIGNALS = ("noise0.3", "noise1e-4", "tone+noise", "tone", "dc", "nyquist", "impulse", "loud-silent")


def signal(name, L, rng):
    n = np.arange(L)
    if name == "noise0.3":
        x = 0.3 * rng.standard_normal(L)
    elif name == "noise1e-4":
        x = 1e-4 * rng.standard_normal(L)
    elif name == "tone+noise":
        x = 0.9 * np.sin(2 * np.pi * 0.0611 * n) + 1e-4 * rng.standard_normal(L)
    elif name == "tone":
        x = 0.9 * np.sin(2 * np.pi * 0.0611 * n)
    elif name == "dc":
        x = np.full(L, 0.5)
    elif name == "nyquist":
        x = 0.5 * (-1.0) ** n
    elif name == "impulse":
        x = np.zeros(L)
        x[L // 2] = 1.0
    else:
        x = np.where(n < L // 2, 0.3 * rng.standard_normal(L), 0.0)
    return x.astype(np.float32)


class Case:
    """a clip of two channels at step 3, phase 2: channel 1 carries the signal on its kept samples and noise of the signal's
    size between them; channel 0 is four times as loud"""

    def __init__(self, shape, name, seed):
        self.shape, self.name = shape, name
        n_fft, hop, _ = shape
        rng = np.random.default_rng(seed)
        self.step, self.phase, self.sample_from = 3, 2, 7 + seed % 3
        L = 9 * hop + n_fft // 2 + 3
        s = signal(name, L, rng)
        skip = phase_skip(self.sample_from, self.step, self.phase)
        n = skip + (L - 1) * self.step + 1 + seed % self.step
        scale = max(float(np.abs(s).max()), 1e-4)
        quiet = (scale * 0.5 * rng.standard_normal(n)).astype(np.float32)
        quiet[skip::self.step] = s
        loud = (4 * scale * rng.standard_normal(n) + 4 * np.resize(s, n)).astype(np.float32)
        self.lanes = np.stack([loud, quiet])
        self.w, self.M = hann(n_fft), matrix_for(shape)

    def __repr__(self):
        return f"{self.shape[0]}/{self.shape[1]}/{self.shape[2]}-{self.name}"

    def stream(self):
        return clip_stream(self.lanes, self.step, phase_skip(self.sample_from, self.step, self.phase))[1]

    def model(self, mutation=None):
        return model_clip(self.lanes, self.sample_from, self.step, self.phase, self.shape, self.w, self.M, mutation)


def case_table():
    return [Case(shape, name, 11 * i + j) for i, shape in enumerate(TABLE_SHAPES) for j, name in enumerate(SIGNALS)]


def f32_worst(table=None):
    worst = 0.0
    for c in table or case_table():
        ref, U = c.model()
        worst = max(worst, distance(f32_eval(c.stream(), c.w, c.M, c.shape[1]), ref, U))
    return worst


if __name__ == "__main__":
    for c in case_table():
        ref, U = c.model()
        print(f"{c!r:32s} {distance(f32_eval(c.stream(), c.w, c.M, c.shape[1]), ref, U):8.4f}")
    print(f"F32_WORST = {f32_worst():.4f}")
