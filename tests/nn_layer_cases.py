"""The float64 model, the per-kernel references, the units, the models, the inputs and the mutations shared by
test_nn_layers_host.py and test_nn_layers_gpu.py: every NSNet2 layer against float64 of exactly the inputs that layer was given,
one kernel at a time.

References  Each takes what the evaluation under test itself produced for the previous layer (and, for a GRU, for the previous
            step), so errors do not compound and every row of every step is judged locally:
              h1[t]  = GRUstep64(W' f64(feat[t]) + b', f64(h1_got[t-1])),   W' = W_ih1 W_fc1, b' = W_ih1 b_fc1 + Wb1 in float64
              h2[t]  = GRUstep64(W_ih2 f64(h1_got[t]) + Wb2, f64(h2_got[t-1])),   h_got[-1] = 0
              f2     = relu(W2 f64(h2_got) + b2),  f3 = relu(W3 f64(f2_got) + b3),  gains = sigmoid(W4 f64(f3_got) + b4)
            Where h1 does not exist (the pipelined gru_ws2k / gru_ws2m recurrence) the two GRU layers are judged as one:
            "h12" is h2 of float64 through both layers from the features.  Its unit is h2's with what the steps before it
            and the layer below it hand on: E1[t]^2 = u1[t]^2 + P(E1[t-1])^2, E2[t]^2 = u2[t]^2 + P(E1[t])^2 + P(E2[t-1])^2, u the
            local units below and P an error vector pushed through the step's Jacobian as independent errors are (root of the
            sum of squares: sqrt(W^2 e^2) per pre-activation).  The worst-case form (sum of |W| e) is useless here: it grows
            to 1e32 units over 54 steps of the seed-7 model, while the local unit alone makes the oracle cost 1000 on the
            saturated model, whose second layer amplifies the first layer's honest rounding.  (Measured, test_nn_layers_host.)
Units       eps = 2^-24.  A pre-activation a = sum_k w_k x_k + b counts in U(a) = eps (sum_k |w_k x_k| + |b|), and so does a relu
            output.  A gain counts in g (1 - g) U(a) + eps g.  A hidden value counts in sum_g |dh/da_g| U(a_g) + eps over the
            gates z, r, n of  h = (1 - z) n + z h_prev,  n = tanh(a_n + r gh_n)  (a_z, a_r: input + recurrent terms and both
            biases; the n gate: U(a_n) + r U(gh_n)), derivatives in float64 at the reference point; the + eps covers the
            exponential and the reciprocal on values in [-1, 1].  A difference where the unit is 0 (every term exactly zero)
            counts as infinite.
Tolerance   TOL[layer] = 4 x the oracle's worst distance over models x inputs below, judged exactly as the GPU is (from its
            own previous-layer outputs: orc_nsnet2_forward_layers).  Measured on the CPU by test_nn_layers_host.py, which
            prints the figures and asserts that the constants are those figures.
"""
import numpy as np

import denoise_cases as D
import orc

EPS = 2.0 ** -24
LAYERS = ("h1", "h2", "f2", "f3", "gains")
H = 400
SKIP = 4    # warm-up rows of an engine chunk (NSNet2.zig:12-16)

# The oracle's worst distance per quantity over MODELS x input_table(), in the units above, rounded up to two decimals.
# Measured with
#   python -m pytest tests/test_nn_layers_host.py -k oracle_distances -s
ORACLE_UNITS = {"h1": 3.16, "h2": 3.04, "h12": 7.35, "f2": 4.18, "f3": 5.27, "gains": 4.44}   # measured: 3.156, 3.037, 7.343, 4.175, 5.266, 4.436
GPU_FACTOR = 4.0
TOL = {k: GPU_FACTOR * v for k, v in ORACLE_UNITS.items()}


def sig(v):
    return 1.0 / (1.0 + np.exp(-v))


# ------------------------------------------------------------------ the shared float64 model

def _gru64(x, w_, r_, b_):
    Hn = r_.shape[1]
    wb, rb = b_[: 3 * Hn], b_[3 * Hn:]
    h = np.zeros(Hn)
    out = np.empty((x.shape[0], Hn))
    for t in range(x.shape[0]):
        gi = w_ @ x[t] + wb
        gh = r_ @ h + rb
        z = sig(gi[:Hn] + gh[:Hn])
        r = sig(gi[Hn:2 * Hn] + gh[Hn:2 * Hn])
        n = np.tanh(gi[2 * Hn:] + r * gh[2 * Hn:])
        h = (1 - z) * n + z * h
        out[t] = h
    return out


def nsnet2_float64(w, f):
    """The ONNX graph in float64 numpy: fc1 -> GRU x2 (gate order z,r,h; linear_before_reset = 1; zero initial
    state) -> relu(fc2) -> relu(fc3) -> sigmoid(fc4)"""
    W = {k: np.asarray(v, np.float64) for k, v in w.items()}
    x = f.astype(np.float64) @ W["fc1_w"].T + W["fc1_b"]
    x = _gru64(x, W["gru1_w"], W["gru1_r"], W["gru1_b"])
    x = _gru64(x, W["gru2_w"], W["gru2_r"], W["gru2_b"])
    x = np.maximum(x @ W["fc2_w"].T + W["fc2_b"], 0)
    x = np.maximum(x @ W["fc3_w"].T + W["fc3_b"], 0)
    return sig(x @ W["fc4_w"].T + W["fc4_b"])


# ------------------------------------------------------------------ models

class Model:
    """f32 weights (ONNX layout) and their float64 copies; fc1 folded into the first input projection in float64"""

    def __init__(self, name, w):
        self.name = name
        self.w = {k: np.ascontiguousarray(v, np.float32) for k, v in w.items()}
        W = self.W = {k: v.astype(np.float64) for k, v in self.w.items()}
        self.Wf = W["gru1_w"] @ W["fc1_w"]                                 # [1200][161]
        self.bf = W["gru1_w"] @ W["fc1_b"] + W["gru1_b"][: 3 * H]
        self.gru = {"h1": (self.Wf, self.bf, W["gru1_r"], W["gru1_b"][3 * H:]),
                    "h2": (W["gru2_w"], W["gru2_b"][: 3 * H], W["gru2_r"], W["gru2_b"][3 * H:])}
        self.dense = {"f2": (W["fc2_w"], W["fc2_b"]), "f3": (W["fc3_w"], W["fc3_b"]), "gains": (W["fc4_w"], W["fc4_b"])}


def tile_scales(n):
    """2^((j // 16) % 5 - 2) for unit j: five magnitudes from 1/4 to 4, one per column tile of 16"""
    return 2.0 ** ((np.arange(n) // 16) % 5 - 2)


def model_weights(name, weights7):
    """"synth": the library's seed-7 weights.  "saturated": the scaling of test_nsnet2_saturated_gates_match_oracle (input
    weights x 8, biases x 4 + 0.5: gate pre-activations of +-40).  "tiles": distinct magnitudes per column tile -- output unit
    j of fc1 / fc2 / fc3 scaled by tile_scales and the next layer's column j by its inverse (powers of two and a positively
    homogeneous relu: the same function, other magnitudes in every tile), and unit j's rows of the two GRUs' input weights and
    input biases scaled the same way (not compensated: h is bounded, the model is simply another one; the recurrent matrices
    stay as they are).  A tile that lands in the wrong place then costs orders of magnitude.  "select": denoise_cases'
    select_varied, where every pre-activation that matters is a single exact product."""
    if name == "select":
        return D.model_weights("select_varied")
    w = {k: np.array(v, np.float32) for k, v in weights7.items()}
    if name == "saturated":
        for k in ("gru1_w", "gru2_w"):
            w[k] *= np.float32(8.0)
        for k in ("gru1_b", "gru2_b"):
            w[k] = (w[k] * np.float32(4.0) + np.float32(0.5)).astype(np.float32)
    elif name == "tiles":
        for out_w, out_b, nxt in (("fc1_w", "fc1_b", "gru1_w"), ("fc2_w", "fc2_b", "fc3_w"), ("fc3_w", "fc3_b", "fc4_w")):
            s = tile_scales(w[out_w].shape[0]).astype(np.float32)
            w[out_w] *= s[:, None]
            w[out_b] *= s
            w[nxt] /= s[None, :]
        s3 = np.tile(tile_scales(H), 3).astype(np.float32)
        for k in ("gru1", "gru2"):
            w[k + "_w"] *= s3[:, None]
            w[k + "_b"][: 3 * H] *= s3
    else:
        assert name == "synth", name
    return w


MODELS = ("synth", "saturated", "tiles", "select")
_models = {}


def model(name, weights7):
    if name not in _models:
        _models[name] = Model(name, model_weights(name, weights7))
    return _models[name]


# ------------------------------------------------------------------ inputs

def make_inputs(n_seq, T, seed):
    """[n_seq][T][161] f32: uniform(-11, 2) log-power features; sequence 0 starts with literal-zero warm-up rows (a first chunk),
    sequence 1 has -12 (silence) in a third of its bins, sequence 2 is loud (20 .. 60), sequence 3 repeats one row (whatever
    still depends on t there is the recurrence's)"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(-11, 2, (n_seq, T, 161)).astype(np.float32)
    f[0, : min(SKIP, max(T - 1, 1))] = 0.0
    if n_seq > 1:
        f[1, :, ::3] = -12.0
    if n_seq > 2:
        f[2] = rng.uniform(20, 60, (T, 161)).astype(np.float32)
    if n_seq > 3:
        f[3] = f[3, 0]
    return f


def input_table():
    """the host test's inputs: every sequence kind at the engine's length, and the short and odd lengths"""
    return [make_inputs(5, 54, 101), make_inputs(4, 1, 102), make_inputs(4, 2, 103), make_inputs(4, 7, 104), make_inputs(4, 55, 105)]


# ------------------------------------------------------------------ one kernel at a time

def _gru_step64(Wx, bx, R, rb, x, h_prev, mutate=None, ex=None, ep=None):
    """rows x [N][K], h_prev [N][H] (float64) -> (h, unit) [N][H].  ex / ep: error vectors of x and of h_prev (the "h12" unit):
    the unit then includes them, pushed through this step as independent errors"""
    ax, ah = np.abs(x), np.abs(h_prev)
    gi, Ui = x @ Wx.T + bx, ax @ np.abs(Wx).T + np.abs(bx)
    gh, Uh = h_prev @ R.T + rb, ah @ np.abs(R).T + np.abs(rb)
    if mutate:
        gi, gh = mutate(gi, gh)
    az, ar = gi[:, :H] + gh[:, :H], gi[:, H:2 * H] + gh[:, H:2 * H]
    z, r = sig(az), sig(ar)
    ghn = gh[:, 2 * H:]
    n = np.tanh(gi[:, 2 * H:] + r * ghn)
    h = (1 - z) * n + z * h_prev
    Uz, Ur = EPS * (Ui[:, :H] + Uh[:, :H]), EPS * (Ui[:, H:2 * H] + Uh[:, H:2 * H])
    Un = EPS * (Ui[:, 2 * H:] + r * Uh[:, 2 * H:])
    dn = (1 - z) * (1 - n * n)
    cz, cr = z * (1 - z) * np.abs(h_prev - n), dn * np.abs(ghn) * r * (1 - r)
    unit = cz * Uz + cr * Ur + dn * Un + EPS
    if ep is not None:
        Pi = (ex * ex) @ (Wx * Wx).T if ex is not None else np.zeros_like(gi)    # squared errors of the pre-activations
        Ph = (ep * ep) @ (R * R).T
        P = Pi + Ph
        prop = cz * cz * P[:, :H] + cr * cr * P[:, H:2 * H] + dn * dn * (Pi[:, 2 * H:] + r * r * Ph[:, 2 * H:]) + (z * ep) ** 2
        unit = np.sqrt(unit * unit + prop)
    return h, unit


def ref_gru(m, layer, x, h_got):
    """layer "h1": x = features [n][T][161]; "h2": x = the h1 under test [n][T][400].  h_got: the same layer's states under test
    [n][T][400].  -> (reference, unit), both [n][T][400] float64"""
    n, T = h_got.shape[:2]
    hp = np.concatenate([np.zeros((n, 1, H)), np.asarray(h_got, np.float64)[:, :-1]], axis=1)
    h, u = _gru_step64(*m.gru[layer], np.asarray(x, np.float64).reshape(n * T, -1), hp.reshape(n * T, H))
    return h.reshape(n, T, H), u.reshape(n, T, H)


def ref_dense(m, layer, x):
    """layer "f2" | "f3" | "gains" on rows x [..., K] of the previous layer under test -> (reference, unit)"""
    Wm, b = m.dense[layer]
    x = np.asarray(x, np.float64)
    a, U = x @ Wm.T + b, EPS * (np.abs(x) @ np.abs(Wm).T + np.abs(b))
    if layer == "gains":
        g = sig(a)
        return g, g * (1 - g) * U + EPS * g
    return np.maximum(a, 0), U


def float64_layers(m, feat, mut=None, skip=0):
    """float64 through the whole network, sequences batched: feat [n][T][161] -> {"h1", "h2", "f2", "f3", "gains"} and, under
    "u_h2", the unit of "h12" (h2 through both layers); f2 / f3 / gains over rows skip .. T-1.  mut: a mutation of MUTATIONS
    (None: the model as it is)."""
    mut = mut or {}
    f = np.asarray(feat, np.float64)
    n, T = f.shape[:2]
    out = {k: np.empty((n, T, H)) for k in ("h1", "h2", "u_h2")}
    x_l1 = mut["l1_input"](f) if "l1_input" in mut else f
    h1, h2, e1, u2 = np.zeros((n, H)), np.zeros((n, H)), np.zeros((n, H)), np.zeros((n, H))
    for t in range(T):
        hp = mut["h1_prev"](h1) if "h1_prev" in mut else h1
        h1, e1 = _gru_step64(*m.gru["h1"], x_l1[:, t], hp, mut.get("gates1"), None, e1)
        h2, u2 = _gru_step64(*m.gru["h2"], h1, h2, None, e1, u2)
        out["h1"][:, t], out["h2"][:, t], out["u_h2"][:, t] = h1, h2, u2
    x = out["h2"][:, skip:]
    if "fc2_rows" in mut:
        x = mut["fc2_rows"](out["h2"], skip)
    out["f2"] = ref_dense(m, "f2", x)[0]
    W3, b3 = m.dense["f3"]
    a3 = out["f2"] @ (mut["fc3_w"](W3) if "fc3_w" in mut else W3).T + b3
    if "fc3_extra" in mut:
        a3 = a3 + mut["fc3_extra"](out["f2"], W3)
    out["f3"] = np.maximum(a3, 0)
    out["gains"] = ref_dense(m, "gains", out["f3"])[0]
    return out


def distance(got, ref, unit):
    """worst |got - ref| / unit and where; a difference over a zero unit is infinite, no difference is 0"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(d == 0, 0.0, d / unit)
    c = np.where(np.isfinite(np.asarray(got, np.float64)), c, np.inf)   # NaN under test: a row nobody wrote
    i = np.unravel_index(np.argmax(c), c.shape)
    return float(c[i]), tuple(int(v) for v in i)


def judge(m, feat, got, skip=0):
    """got: {"h1" (or None), "h2", "f2", "f3", "gains"} of one evaluation on feat [n][T][161] (f2 / f3 / gains: rows skip .. T-1).
    -> {quantity: (worst distance, index)}; "h12" instead of "h1" and "h2" where h1 is None."""
    res = {}
    if got.get("h1") is not None:
        res["h1"] = distance(got["h1"], *ref_gru(m, "h1", feat, got["h1"]))
        res["h2"] = distance(got["h2"], *ref_gru(m, "h2", got["h1"], got["h2"]))
    else:
        full = float64_cached(m, feat)
        res["h12"] = distance(got["h2"], full["h2"], full["u_h2"])
    res["f2"] = distance(got["f2"], *ref_dense(m, "f2", np.asarray(got["h2"])[:, skip:]))
    res["f3"] = distance(got["f3"], *ref_dense(m, "f3", got["f2"]))
    res["gains"] = distance(got["gains"], *ref_dense(m, "gains", got["f3"]))
    return res


_f64_cache = {}


def float64_cached(m, feat):
    """float64_layers per (model, input), computed once"""
    feat = np.ascontiguousarray(feat, np.float32)
    key = (m.name, feat.shape, hash(feat.tobytes()))
    if key not in _f64_cache:
        _f64_cache[key] = float64_layers(m, feat)
    return _f64_cache[key]


def oracle_layers(m, feat):
    """orc_nsnet2_forward_layers per sequence, stacked: {"h1", ...: [n][T][width] f32}"""
    per = [orc.nsnet2_forward_layers(m.w, s) for s in feat]
    return {k: np.stack([p[k] for p in per]) for k in LAYERS}


def gains_metric(g, ref):
    """the end-to-end checks' metric (assert_rel(..., 1e-4, floor=1e-2) of tests/test_gpu.py): worst relative error, floor 1e-2"""
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(g, np.float64) - ref) / np.maximum(np.abs(ref), 1e-2)).max())


# ------------------------------------------------------------------ mutations of the float64 model

MUT_UNIT = 37   # the one unit the single-unit mutations touch (tile 2, lane 5)


def _rbias_n(gi, gh):
    gh = gh.copy()
    gh[:, 2 * H + MUT_UNIT] += 1e-3
    return gi, gh


def _swap_zr(gi, gh):
    gi, gh = gi.copy(), gh.copy()
    for g in (gi, gh):
        g[:, [MUT_UNIT, H + MUT_UNIT]] = g[:, [H + MUT_UNIT, MUT_UNIT]]
    return gi, gh


def _neighbour_state(h):
    """sequence 1 of the batch (a row of the first 16-row tile) reads the state of sequence 2"""
    h = h.copy()
    h[1] = h[2]
    return h


def _fc3_drop(W3):
    W3 = W3.copy()
    W3[MUT_UNIT, 123] = 0.0
    return W3


def chunked_features(n_chunks, seed):
    """one lane of n_chunks engine chunks as sequences [n_chunks][54][161]: rows 0..3 of chunk g are rows 50..53 of chunk g - 1
    (K1's copyBackwards), literal zeros in the first"""
    f = np.random.default_rng(seed).uniform(-11, 2, (n_chunks, 54, 161)).astype(np.float32)
    f[0, :SKIP] = 0.0
    f[1:, :SKIP] = f[:-1, 50:]
    return f


def _own_warmup_rows(f):
    f = f.copy()
    f[1:, :SKIP] = f[1:, 50:]
    return f


# name -> (the layer it touches, mutation, whether it needs the engine's chunk layout with skip = 4)
MUTATIONS = {
    "one unit's recurrent n-bias + 1e-3": ("h1", {"gates1": _rbias_n}, False),
    "z and r swapped for one unit": ("h1", {"gates1": _swap_zr}, False),
    "one k term dropped from one fc3 row": ("f3", {"fc3_w": _fc3_drop}, False),
    "h[t-1] of the neighbouring sequence in a 16-row tile": ("h1", {"h1_prev": _neighbour_state}, False),
    "fc2 reads row t instead of t + skip": ("f2", {"fc2_rows": lambda h2, skip: h2[:, : h2.shape[1] - skip]}, True),
    "warm-up rows 0..3 from the chunk's own rows 50..53": ("h1", {"l1_input": _own_warmup_rows}, True),
    # the padding column holds what unit 0 holds and is weighted like unit 599
    "a padding column (unit 600) leaks into fc3's sum": ("f3", {"fc3_extra": lambda f2, W3: f2[..., :1] * W3[:, 599]}, False),
}
