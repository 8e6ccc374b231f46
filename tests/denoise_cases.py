"""Case tables, float64 references, gain models and the error metric shared by test_denoise_f64_host.py and
test_denoise_f64_gpu.py: K1 (stft_kernel: chunk RMS, /3 decimation, sqrt-Hann 320-point real FFT, log-power features) and K3
(istft_kernel: gain, inverse FFT, window, overlap-add, x3 lerp) against float64 of exactly the inputs each kernel was given, one
kernel at a time -- never against another path of the library.  Only the f32 sqrt-Hann window (orc.nsnet2_window) is shared with
the library and the oracle, widened to f64.

Reference   ref_k1: X64[f] = rfft(f64(ai[160 f : 160 f + 320]) * f64(w)), features log10(max(|X64|^2, f64(f32(1 / 1e12f)))),
            decimation x[::3] (exact), RMS sqrt(mean(f64(x)^2)) over the chunk's 24000 samples (PCM16: s / 32768 first).
            ref_k3: y[f] = irfft(g X, 320) * f64(w) (numpy divides by 320: the reference's 1 / n_fft; bins 0 and 160 real),
            d[160 f + j] = y[f-1][160 + j] + y[f][j], out[3 m + 2] = d[m], out[3 m + j] = d[m-1] + (d[m] - d[m-1]) (j + 1) / 3,
            from the f32 spectrogram and the f32 gains K3 read, clamped to [-80, 1].
Metric      k4_cases.EPS, bin_units and _units, and in addition (all in units of eps = 2^-24 times):
              spectrogram bin (real and imaginary part each)   ||X64[f]||_2
              feature                                          0.8686 ||X||_2 / max(|X_k|, 1e-6) + max(|feat|, 1): amplitude
                                                               round-off carried through log10 of the power, plus the log's own
              RMS                                              rms
              decimated output sample m of hop f               ||y64[f-1]||_2 + ||y64[f]||_2; an interpolated sample takes the
                                                               larger unit of its two neighbours
            Where the reference is identically zero (digital silence) the output must be exactly zero (either sign of zero: a
            butterfly's 0 * negative twiddle is -0), features must be -12 to 2e-6.  Non-finite output counts as infinitely far.
Tolerance   the oracle's own worst distance over the whole case table (ORACLE_*_UNITS below, measured on the CPU and asserted by
            test_denoise_f64_host.py); a GPU kernel gets k4_cases.GPU_FACTOR times that, for the reason given in k4_cases.
Gain models weight dictionaries whose gains have a closed form and whose bits cannot depend on a GEMM's accumulation order:
            bias-only (every matrix zero, gain = sigmoid(fc4_b[k])) and selection models (one nonzero entry per weight row, every
            one of them a power of two, so that each pre-activation is one EXACT product plus a bias: the same bits whether the
            bias is added after the product or fused into it):
              gain[t, k] = sigmoid(a relu(tanh(c2 tanh(c1[k] feat[t, j(k)]))) + b[k]).
Out of scope  gains above 1 or below -80: the clamp's two branches are unreachable through a sigmoid output and there is no
            gain tap; no entry point is added for them.
"""
import ctypes as C

import numpy as np

import k4_cases as k4
import orc

EPS = k4.EPS
CHUNK, DEC, HOP, NFFT, NB, FRAMES, ROWS, WARM = 24000, 8000, 160, 320, 161, 50, 54, 4
P_MIN = np.float64(np.float32(1.0) / np.float32(1e12))      # std.math.pow(f32, 10, -12) of the reference
DIMS = (161, 400, 400, 600, 600)                            # NSNet2: bins, fc1, hidden, fc2, fc3

# The oracle's worst distance from the float64 reference over the whole chunk table, in the units above, rounded up to two
# decimals.  Measured with
#   python -m pytest tests/test_denoise_f64_host.py -k oracle -s
# which prints the figures (and asserts that the oracle still stays inside these).
ORACLE_SPEC_UNITS = 1.77
ORACLE_FEAT_UNITS = 0.81
ORACLE_RMS_UNITS = 1303.98      # the sequential f32 sum of 24000 equal squares ("dropped 0.9")
ORACLE_DEN_UNITS = {"bias_mixed": 0.87, "bias_unity": 0.63, "select_varied": 1.10, "select_alternating": 1.37}

# The oracle's RMS figure is that of a sequential sum and cannot see one sample of 24000 missing (some 350 units).  A bound that
# can, for any summation whose longest chain of f32 additions is at most 96 long (K1: 256 threads x 24 float4s = 96 squares
# each) under a tree of at most 8 levels (six across a wavefront, two across four wavefronts): every square and every addition
# rounds by at most one unit (2^-24 relative) of the sum so far, which never exceeds the total: (1 + 96 + 8) units on the sum,
# half of that on its square root, one unit each for the division and the square root: 54.5, stated as 55.
RMS_TREE_UNITS = 55.0

# |gain - closed form| allowed to an f32 evaluation of a gain model (gains live in [0, 1]): two tanh, one exp and one division,
# each within 2 ulp of a value <= 1 (an ulp of 1 is 1.2e-7; the GPU's fast exp / tanh: twice that), the tanh errors reach the
# sigmoid's argument multiplied by a <= 16, and sigmoid' <= 1 / 4: (2 + 2) * 2 * 16 / 4 + 2 * 2 = 36 ulp of 1 = 4.3e-6
GAIN_ABS_TOL = 4.3e-6


def window64():
    return orc.nsnet2_window().astype(np.float64)


# ------------------------------------------------------------------ the reference: K1

def ref_spec(dec_hist):
    """dec_hist: f32 decimated samples, 160 of history followed by 160 n -> float64 complex [n][161]"""
    x = np.asarray(dec_hist)
    assert x.dtype == np.float32 and x.ndim == 1 and (x.shape[0] - HOP) % HOP == 0
    n = (x.shape[0] - HOP) // HOP
    idx = HOP * np.arange(n)[:, None] + np.arange(NFFT)[None, :]
    return np.fft.rfft(x.astype(np.float64)[idx] * window64(), axis=1)


def ref_features(X64):
    return np.log10(np.maximum(np.abs(X64) ** 2, P_MIN))


def ref_k1(ai):
    """ai: the 8160 f32 decimated samples of a chunk (160 previous + 8000) -> (X64 [50][161], features [50][161])"""
    assert np.asarray(ai).shape == (DEC + HOP,)
    X = ref_spec(ai)
    return X, ref_features(X)


def as_f32(x):
    """a lane's samples as the kernel sees them: PCM16 is s / 32768 (exact in f32)"""
    x = np.asarray(x)
    return (x.astype(np.float32) * np.float32(1.0 / 32768.0)) if x.dtype == np.int16 else x


def ref_lane_k1(x):
    """x: a lane's raw 48 kHz samples (f32 or int16), whole chunks -> (X64 [n][50][161], feat64 [n][50][161], rms64 [n])"""
    x = as_f32(x)
    n = x.shape[0] // CHUNK
    x = x[: n * CHUNK]
    dec = np.concatenate([np.zeros(HOP, np.float32), x[::3]])
    X = ref_spec(dec).reshape(n, FRAMES, NB)
    rms = np.sqrt((x.astype(np.float64).reshape(n, CHUNK) ** 2).mean(axis=1))
    return X, ref_features(X), rms


# ------------------------------------------------------------------ the reference: K3

def ref_k3(spec, gains, ola_in=None, last_in=0.0, norm_in=0.0):
    """spec: complex [n][50][161] (the f32 array K3 read; any complex type is widened), gains: f32 [n][50][161] or a scalar.
    ola_in: y[-1][160:320] (zeros at t = 0), last_in: d[-1], norm_in: ||y[-1]||_2 (for the metric only).
    Returns a dict: d [8000 n], out [24000 n], unit_d, unit_out (eps included), ola_out [160], last_out, norm_out."""
    X = np.asarray(spec).astype(np.complex128).reshape(-1, NB)
    g = np.clip(np.asarray(gains, np.float64), -80.0, 1.0)
    g = np.broadcast_to(g.reshape(-1, NB) if g.ndim else g, X.shape)
    Y = X * g
    Y[:, 0] = Y[:, 0].real
    Y[:, NB - 1] = Y[:, NB - 1].real
    y = np.fft.irfft(Y, NFFT, axis=1) * window64()
    carry = np.zeros(HOP) if ola_in is None else np.asarray(ola_in, np.float64)
    prev_half = np.concatenate([carry[None, :], y[:-1, HOP:]])
    d = (prev_half + y[:, :HOP]).reshape(-1)
    dm1 = np.concatenate([[np.float64(last_in)], d[:-1]])
    out = np.empty((d.shape[0], 3))
    out[:, 0] = dm1 + (d - dm1) * (1.0 / 3.0)
    out[:, 1] = dm1 + (d - dm1) * (2.0 / 3.0)
    out[:, 2] = d
    norms = np.sqrt((y * y).sum(axis=1))
    hop_unit = EPS * (np.concatenate([[np.float64(norm_in)], norms[:-1]]) + norms)
    unit_d = np.repeat(hop_unit, HOP)
    um1 = np.concatenate([unit_d[:1], unit_d[:-1]])
    unit_out = np.stack([np.maximum(um1, unit_d)] * 2 + [unit_d], axis=1)
    return {"d": d, "out": out.reshape(-1), "unit_d": unit_d, "unit_out": unit_out.reshape(-1), "ola_out": y[-1, HOP:].copy(),
            "last_out": d[-1], "norm_out": norms[-1]}


def fused_lerp_rows(out):
    """the x3 upsampler's own rule on its own output: out[3 m + j], j = 0, 1, must be the fused lerp (b - a) t + a of a =
    out[3 m - 1] and b = out[3 m + 2], the difference rounded to f32 first, t = f32((j + 1) / 3).  Returns the wanted f32
    [(n - 1)][2] for m = 1 .. n - 1 (m = 0 needs the sample before the array)."""
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape[0] % 3 == 0
    a, b = out[2:-3:3], out[5::3]
    diff = (b - a).astype(np.float64)       # np.float32 - np.float32: one f32 rounding
    want = [(diff * np.float64(np.float32(j + 1) / np.float32(3)) + a.astype(np.float64)).astype(np.float32) for j in range(2)]
    return np.stack(want, axis=1)


# ------------------------------------------------------------------ the metric

def _any_zero(got):
    """-0.0 -> +0.0 (k4._units asks for +0.0 where the reference has nothing; here either zero is exact)"""
    return np.asarray(got) + np.float32(0.0)


def _worst(u):
    i = np.unravel_index(np.argmax(u), u.shape)
    return float(u[i]), tuple(int(v) for v in i)


def spec_units(got, X64):
    """got: complex64 [F][161]; X64: [F][161].  Worst component error in units of eps ||X64[f]||_2 (k4.bin_units over the
    interleaved real and imaginary parts).  Returns (worst, (frame, bin))."""
    got = np.ascontiguousarray(np.asarray(got).reshape(-1, NB), np.complex64)
    X = np.asarray(X64).reshape(-1, NB)
    ref = np.stack([X.real, X.imag], axis=2).reshape(X.shape[0], 2 * NB)
    w, (f, c) = k4.bin_units(_any_zero(got.view(np.float32)), ref)
    return w, (f, c // 2)


def feat_units(got, X64):
    """got: f32 [F][161] features of the frames whose float64 spectrum is X64.  Returns (worst, (frame, bin))."""
    got = np.ascontiguousarray(np.asarray(got).reshape(-1, NB))
    X = np.asarray(X64).reshape(-1, NB)
    amp = np.abs(X)
    x2 = np.sqrt((amp * amp).sum(axis=1))[:, None]
    ref = ref_features(X)
    unit = EPS * (0.8686 * x2 / np.maximum(amp, 1e-6) + np.maximum(np.abs(ref), 1.0))
    u = k4._units(got, ref, unit)
    silent = x2[:, 0] == 0.0
    ok = np.isfinite(got[silent]) & (np.abs(got[silent].astype(np.float64) + 12.0) <= 2e-6)
    u[silent] = np.where(ok, 0.0, np.inf)
    return _worst(u)


def rms_units(got, rms64):
    got = np.ascontiguousarray(np.asarray(got).reshape(-1))
    ref = np.asarray(rms64, np.float64).reshape(-1)
    w, (i,) = _worst(k4._units(_any_zero(got), ref, EPS * ref))
    return w, i


def den_units(got, ref, key="out"):
    """got: f32 samples; ref: ref_k3's dict.  The distance of every sample, in its own unit (key 'out': the 48 kHz samples,
    'd': the decimated ones)."""
    got = np.ascontiguousarray(np.asarray(got).reshape(-1))
    return k4._units(_any_zero(got), ref[key], ref["unit_" + key])


def seam_mask(n_chunks):
    """48 kHz samples of the first 160 decimated samples of every chunk: the seam to chunk g - 1 or to the carry"""
    m = np.zeros((n_chunks, CHUNK), bool)
    m[:, : 3 * HOP] = True
    return m.reshape(-1)


def run_boundary_mask(n_chunks, around=4):
    """48 kHz samples within `around` decimated samples of K3's run boundaries: pairs floor(25 run / n_runs), n_runs = 4, 8, 12"""
    m = np.zeros((n_chunks, DEC), bool)
    for n_runs in (4, 8, 12):
        for run in range(1, n_runs):
            p0 = (25 * run) // n_runs
            m[:, 320 * p0 - around: 320 * p0 + around] = True
    return np.repeat(m.reshape(-1), 3)


# ------------------------------------------------------------------ launches (nn_dispatch.cpp, run_chunks)

def launch_sizes(total, cap):
    """chunks per launch of a call of `total` chunks under max_chunks_per_launch = cap"""
    return [min(cap, total - i) for i in range(0, total, cap)]


def fft_parts(n):
    """workgroup form of K1 / K3 at a launch of n chunks: 3 up to 85 chunks, 2 up to 128, then 1"""
    return 3 if n <= 85 else (2 if n <= 128 else 1)


# ------------------------------------------------------------------ inputs

FLIP_BIN = 40
TONE_BINS = [0, 1, 79, 80, 81, 159, 160]


def _tone48(k, amp, phase):
    """a tone exactly on bin k of the 16 kHz frame, written at 48 kHz: decimation keeps sin(2 pi k m / 320 + phase)"""
    t = np.arange(CHUNK, dtype=np.float64)
    return (amp * np.sin(2.0 * np.pi * k * t / (3 * NFFT) + phase)).astype(np.float32)


def _dec_only(dec, fill=0.0):
    x = np.full(CHUNK, fill, np.float32)
    x[::3] = dec
    return x


def chunk_table():
    """[(label, 24000 f32 samples)]: ordered so that neighbours are unlike and silence sits between loud chunks"""
    rng = np.random.default_rng(20240)
    m = np.arange(DEC)
    imp = lambda pos: _dec_only(np.where(m == pos, 1.0, 0.0).astype(np.float32))     # noqa: E731
    t = np.arange(CHUNK, dtype=np.float64)
    quiet = (0.9 * np.sin(2.0 * np.pi * 37.37 * t / (3 * NFFT) + 0.3) + rng.uniform(-1e-4, 1e-4, CHUNK)).astype(np.float32)
    # the sign of an on-bin tone flips every second hop: frames whose two hops agree are loud in bin FLIP_BIN, frames whose hops
    # disagree cancel there (the window is symmetric) -- a feature that alternates from frame to frame
    sign = 1.0 - 2.0 * ((m // HOP // 2) % 2)
    flip = _dec_only((0.5 * sign * np.sin(2.0 * np.pi * FLIP_BIN * m / NFFT + 0.7)).astype(np.float32))
    tones = {k: _tone48(k, a, 0.7 + 0.37 * i) for i, (k, a) in enumerate(zip(TONE_BINS, (0.25, 0.9, 0.5, 0.7, 1e-3, 0.6, 0.8)))}
    return [
        ("noise 1.0", rng.uniform(-1.0, 1.0, CHUNK).astype(np.float32)),
        ("silence", np.zeros(CHUNK, np.float32)),
        ("full scale", np.where(rng.uniform(-1, 1, CHUNK) < 0, -1.0, 1.0).astype(np.float32)),
        ("amplitude 1e-7", rng.uniform(-1e-7, 1e-7, CHUNK).astype(np.float32)),
        ("quiet bins", quiet),
        ("noise 1e-4", rng.uniform(-1e-4, 1e-4, CHUNK).astype(np.float32)),
        ("tone 0", tones[0]),
        ("dropped 0.9", _dec_only(np.zeros(DEC, np.float32), fill=0.9)),
        ("tone 1", tones[1]),
        ("dc -1e-9", np.full(CHUNK, -1e-9, np.float32)),
        ("tone 79", tones[79]),
        ("impulse 0", imp(0)),
        ("tone 80", tones[80]),
        ("impulse 159", imp(159)),
        ("tone 81", tones[81]),
        ("impulse 160", imp(160)),
        ("tone 159", tones[159]),
        ("impulse 7999", imp(7999)),
        ("tone 160", tones[160]),
        ("dc 0.5", np.full(CHUNK, 0.5, np.float32)),
        ("nyquist", _dec_only((0.5 * (1.0 - 2.0 * (m % 2))).astype(np.float32))),
        ("flip tone", flip),
        ("flip tone b", flip),      # twice in a row: the alternation crosses a chunk seam
    ]


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = chunk_table()
    return _TABLE


def lane_indices(lane, n_chunks):
    """table entries of lane `lane`: consecutive entries from a start of its own (neighbouring lanes are 7 entries apart)"""
    return [(7 * lane + i) % len(table()) for i in range(n_chunks)]


def make_lane(lane, n_chunks):
    return np.concatenate([table()[i][1] for i in lane_indices(lane, n_chunks)]) if n_chunks else np.zeros(0, np.float32)


def to_pcm16(x):
    return np.clip(np.rint(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def significant_power_normal(X64):
    """the normal-range condition on the inputs: |X|^2 of each bin that reaches one unit of the spectrogram metric lies inside
    normal f32.  Returns the offending (frame, bin) pairs."""
    X = np.asarray(X64).reshape(-1, NB)
    amp = np.abs(X)
    x2 = np.sqrt((amp * amp).sum(axis=1))[:, None]
    sig = (amp >= EPS * x2) & (x2 > 0)
    sq = amp * amp
    bad = sig & ((sq < float(np.finfo(np.float32).tiny)) | (sq > float(np.finfo(np.float32).max)))
    return [tuple(int(v) for v in i) for i in np.argwhere(bad)]


# ------------------------------------------------------------------ gain models

def _zeros(dims=DIMS):
    return {k: np.zeros(s, np.float32) for k, s in orc.WEIGHT_SHAPES(*dims).items()}


def bias_vector(kind):
    if kind == "bias_unity":
        return np.full(NB, 40.0, np.float32)            # sigmoid(40) rounds to exactly 1 in f32 and in f64 arithmetic alike
    b = np.linspace(-12.0, 12.0, NB).astype(np.float32)
    b[[3, 80, 157]] = 0.0                               # gain exactly 0.5
    b[[10, 150]] = 40.0
    b[[20, 140]] = -40.0
    b[[0, 30, 160]] = -100.0                            # gain 0 (3.8e-44 in exact arithmetic): bins 0 and 160 among them
    return b


SELECT = {
    # j(k): which feature bin drives gain k; c1[k], c2, a: powers of two; b[k]: the fc4 bias
    "select_varied": dict(j=(7 * np.arange(NB) + 3) % NB, c1=np.where(np.arange(NB) % 2 == 0, -0.125, 0.125), c2=2.0, a=8.0,
                          b=np.linspace(-4.0, 0.0, NB)),
    # every gain follows bin FLIP_BIN: ~1 in frames where it is loud (log-power > 0), ~0 where it cancels
    "select_alternating": dict(j=np.full(NB, FLIP_BIN), c1=np.full(NB, 1.0), c2=2.0, a=16.0, b=np.full(NB, -8.0)),
}
MODELS = ["bias_mixed", "bias_unity", "select_varied", "select_alternating"]


def model_weights(name, dims=DIMS):
    """weight dictionary (ONNX layout: orc.WEIGHT_SHAPES / fv.weight_shapes; GRU gate order z, r, h; bias = input biases then
    recurrent biases, as _nsnet2_float64 of tests/test_gpu.py reads them)"""
    nb, f1, H, f2, f3 = dims
    w = _zeros(dims)
    if name.startswith("bias"):
        w["fc4_b"][:] = bias_vector(name)
        return w
    s = SELECT[name]
    src = lambda n: np.arange(n) % nb       # noqa: E731  unit i of every layer belongs to the chain of bin i mod 161
    u1, uh, u2, u3 = src(f1), src(H), src(f2), src(f3)
    w["fc1_w"][np.arange(f1), s["j"][u1]] = 1.0                     # x1[i] = feat[j(i)]
    for name_w, name_b, n_in, c in (("gru1_w", "gru1_b", f1, s["c1"][uh]), ("gru2_w", "gru2_b", H, s["c2"])):
        pick = np.arange(H) % n_in if n_in < H else np.arange(H)     # unit i reads unit i of the layer below
        for gate in range(3):                                       # z, r, h: one entry per row
            w[name_w][gate * H + np.arange(H), pick] = c if gate == 2 else 1.0
        w[name_b][:H] = -100.0                                      # z = sigmoid(x - 100) = 0: h = n = tanh(c x); R = 0
    w["fc2_w"][np.arange(f2), np.arange(f2) % H] = 1.0
    w["fc3_w"][np.arange(f3), np.arange(f3) % f2] = 1.0
    w["fc4_w"][np.arange(nb), np.arange(nb)] = s["a"]
    w["fc4_b"][:] = s["b"]
    return w


def closed_form_gains(name, feat):
    """float64 gains of a model on f32 features [..., 161]"""
    f = np.asarray(feat, np.float64)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))    # noqa: E731
    if name.startswith("bias"):
        return np.broadcast_to(sig(bias_vector(name).astype(np.float64)), f.shape).copy()
    s = SELECT[name]
    r = np.maximum(np.tanh(s["c2"] * np.tanh(s["c1"] * f[..., s["j"]])), 0.0)
    return sig(s["a"] * r + s["b"].astype(np.float32).astype(np.float64))


# ------------------------------------------------------------------ the oracle

def oracle_k1(ai):
    """orc_nsnet2_spec_features on the 8160 decimated samples -> (complex64 [50][161], f32 [50][161])"""
    s = np.zeros((FRAMES, NB, 2), np.float32)
    f = np.zeros((FRAMES, NB), np.float32)
    orc.lib().orc_nsnet2_spec_features(orc.fptr(np.ascontiguousarray(ai, np.float32)), s.ctypes.data_as(C.POINTER(orc.Cpx)), orc.fptr(f))
    return s.view(np.complex64)[..., 0], f


def oracle_rms(x):
    x = np.ascontiguousarray(x, np.float32)
    return np.float32(orc.lib().orc_rms_volume(orc.fptr(x), x.shape[0], None, 0))


def oracle_audio_output(den):
    """the Denoiser's 8160 overlap-add samples after a chunk: [0, 8000) the decimated output, [8000, 8160) its carry"""
    return np.ctypeslib.as_array(orc.lib().orc_nsnet2_audio_output(den.h), (DEC + HOP,)).copy()
