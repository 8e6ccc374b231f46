"""The yardstick of K1 and K3, checked on the CPU: the float64 references of denoise_cases against closed forms that involve no
FFT, the gain models against their closed forms, the input table's conditions, and the oracle's own distance from the
references over the whole chunk table -- the constants from which the GPU tolerances of test_denoise_f64_gpu.py derive."""
import numpy as np
import pytest

import denoise_cases as dc
import k4_cases as k4
import orc
from test_gpu import _nsnet2_float64

N_TABLE = len(dc.table())
WRAP = N_TABLE + 1      # a lane that walks the whole table and meets its first entry again: every adjacency of the table


def _ai_of(x, c):
    """audio_input of chunk c of a lane: the previous chunk's last 160 decimated samples (zeros at t = 0), then 8000"""
    dec = dc.as_f32(x)[::3]
    prev = dec[dc.DEC * c - dc.HOP: dc.DEC * c] if c else np.zeros(dc.HOP, np.float32)
    return np.ascontiguousarray(np.concatenate([prev, dec[dc.DEC * c: dc.DEC * (c + 1)]]))


# ------------------------------------------------------------------ the references against closed forms

def test_unity_gains_reproduce_the_windowed_input_without_any_fft():
    # with all gains 1, irfft(rfft(x w)) w = x w^2, so d[160 f + j] = ai[160 f + j] (w[j]^2 + w[160 + j]^2) in exact arithmetic,
    # ai the lane's decimated samples behind their 160 samples of history (zeros at t = 0: there hop 0 is all zero)
    w = dc.window64()
    for lane in (0, 2, 4):
        x = dc.make_lane(lane, 2)
        ai = np.concatenate([np.zeros(dc.HOP), x[::3].astype(np.float64)])
        X = np.concatenate([dc.ref_k1(_ai_of(x, c))[0] for c in range(2)])
        assert np.array_equal(X.reshape(2, dc.FRAMES, dc.NB), dc.ref_lane_k1(x)[0])
        r = dc.ref_k3(X, 1.0)
        want = (ai[:-dc.HOP].reshape(-1, dc.HOP) * (w[:dc.HOP] ** 2 + w[dc.HOP:] ** 2)[None, :]).reshape(-1)
        scale = np.abs(ai).max()
        assert np.abs(r["d"] - want).max() <= 1e-12 * scale, (lane, np.abs(r["d"] - want).max())
        # the K1 -> K3 round trip with gains 0.5 is half of the gains-1 result
        h = dc.ref_k3(X, np.float32(0.5))
        assert np.abs(h["d"] - 0.5 * r["d"]).max() <= 1e-15 * scale and np.abs(h["out"] - 0.5 * r["out"]).max() <= 1e-15 * scale
        # and chunk by chunk through the carries it is the same thing
        a = dc.ref_k3(X[:dc.FRAMES], 1.0)
        b = dc.ref_k3(X[dc.FRAMES:], 1.0, ola_in=a["ola_out"], last_in=a["last_out"], norm_in=a["norm_out"])
        assert np.array_equal(np.concatenate([a["out"], b["out"]]), r["out"])


def test_window_overlap_adds_to_one():
    # sqrt-Hann, symmetric: w[j]^2 + w[160 + j]^2 is 1 only for the periodic window; the symmetric one is off by O(1 / 320) --
    # the reference keeps the library's and the oracle's table, whatever it sums to
    w = dc.window64()
    s = w[:dc.HOP] ** 2 + w[dc.HOP:] ** 2
    assert np.abs(s - 1.0).max() < 0.02 and np.allclose(w, w[::-1], atol=1e-7)


@pytest.mark.parametrize("k", dc.TONE_BINS + [37])
def test_ref_k1_of_a_tone_on_a_bin_is_analytic(k):
    # x[n] = A sin(2 pi k n / 320 + phi) under window w: X[k] = (A / 2i) (e^{i phi} W[0] - e^{-i phi} W[2 k mod 320]), W the DFT
    # of the window -- computed here as plain sums over the f32 table, no FFT.  Bins 0 and 160: the two images coincide.
    A, phi = 0.75, 0.7
    n = np.arange(dc.DEC + dc.HOP, dtype=np.float64)
    ai = (A * np.sin(2.0 * np.pi * k * n / dc.NFFT + phi)).astype(np.float32)
    X, feat = dc.ref_k1(ai)
    w = dc.window64()
    m = np.arange(dc.NFFT)
    for f in (0, 1, 17, 49):
        ph = phi + 2.0 * np.pi * k * (dc.HOP * f) / dc.NFFT
        for q in {k, max(k - 1, 0), min(k + 1, 160)}:
            Wm = (w * np.exp(-2j * np.pi * (q - k) * m / dc.NFFT)).sum()
            Wp = (w * np.exp(-2j * np.pi * (q + k) * m / dc.NFFT)).sum()
            want = A / 2j * (np.exp(1j * ph) * Wm - np.exp(-1j * ph) * Wp)
            # the f32 samples differ from the ideal tone by 2^-24 relative each: 1e-6 of the bin's scale with room
            assert abs(X[f, q] - want) <= 1e-6 * A * w.sum(), (k, f, q, X[f, q], want)
    assert np.array_equal(feat, np.log10(np.maximum(np.abs(X) ** 2, dc.P_MIN)))
    assert abs(float(dc.P_MIN) - 1e-12) < 1e-19


def test_ref_upsampler_and_rms():
    rng = np.random.default_rng(3)
    X = rng.normal(size=(1, dc.FRAMES, dc.NB)) + 1j * rng.normal(size=(1, dc.FRAMES, dc.NB))
    r = dc.ref_k3(X, 1.0, ola_in=rng.normal(size=dc.HOP), last_in=0.25)
    d, out = r["d"], r["out"]
    assert np.array_equal(out[2::3], d)
    assert abs(out[0] - (0.25 + (d[0] - 0.25) / 3)) < 1e-15 and abs(out[1] - (0.25 + 2 * (d[0] - 0.25) / 3)) < 1e-15
    assert np.abs(out[3::3] - (2 * d[:-1] + d[1:]) / 3).max() < 1e-14 and np.abs(out[4::3] - (d[:-1] + 2 * d[1:]) / 3).max() < 1e-14
    assert r["last_out"] == d[-1] and r["ola_out"].shape == (dc.HOP,)
    # two chunks at once = one after the other through the carries
    X2 = rng.normal(size=(2, dc.FRAMES, dc.NB)) + 1j * rng.normal(size=(2, dc.FRAMES, dc.NB))
    g2 = rng.uniform(0, 1, (2, dc.FRAMES, dc.NB)).astype(np.float32)
    both = dc.ref_k3(X2, g2)
    a = dc.ref_k3(X2[:1], g2[:1])
    b = dc.ref_k3(X2[1:], g2[1:], ola_in=a["ola_out"], last_in=a["last_out"], norm_in=a["norm_out"])
    assert np.array_equal(both["out"], np.concatenate([a["out"], b["out"]]))
    assert np.array_equal(both["unit_out"][dc.CHUNK + 2:], b["unit_out"][2:])      # (b does not know the unit before its first sample)
    # the clamp
    assert np.array_equal(dc.ref_k3(X, 3.0)["d"], dc.ref_k3(X, 1.0)["d"])
    # RMS: PCM16 is s / 32768; the dropped samples count
    s = dc.to_pcm16(dc.make_lane(0, 1))
    _, _, rms = dc.ref_lane_k1(s)
    assert abs(rms[0] - np.sqrt(np.mean((s.astype(np.float64) / 32768.0) ** 2))) < 1e-15
    labels = [l for l, _ in dc.table()]
    x = dc.table()[labels.index("dropped 0.9")][1]
    X1, feat, rms = dc.ref_lane_k1(x)
    assert not X1.any() and (feat == -12.0 + (np.log10(dc.P_MIN) + 12.0)).all() and abs(rms[0] - 0.9 * np.sqrt(2.0 / 3.0)) < 1e-7


def test_fused_lerp_rows_is_the_upsamplers_rule():
    rng = np.random.default_rng(5)
    d = rng.uniform(-1, 1, 100).astype(np.float32)
    out = np.zeros(300, np.float32)
    out[2::3] = d
    for m in range(1, 100):
        for j in range(2):
            t = np.float32(j + 1) / np.float32(3)
            out[3 * m + j] = np.float32(np.float64(np.float32(d[m] - d[m - 1])) * np.float64(t) + np.float64(d[m - 1]))
    assert np.array_equal(dc.fused_lerp_rows(out), out.reshape(100, 3)[1:, :2])
    sw = out.copy()
    sw.reshape(100, 3)[:, [0, 1]] = out.reshape(100, 3)[:, [1, 0]]      # frac1 and frac2 swapped
    assert not np.array_equal(dc.fused_lerp_rows(sw), sw.reshape(100, 3)[1:, :2])


# ------------------------------------------------------------------ the metric refuses what it must

def test_metric_refuses_what_it_must():
    x = dc.make_lane(0, 3)                      # noise 1.0 | silence | full scale
    X, feat, rms = dc.ref_lane_k1(x)
    Xf = X.reshape(-1, dc.NB)
    assert dc.spec_units(Xf.astype(np.complex64), Xf)[0] <= 1.0
    assert dc.feat_units(feat.astype(np.float32), Xf)[0] <= 1.0
    assert dc.rms_units(rms.astype(np.float32), rms)[0] <= 1.0
    assert dc.spec_units(np.roll(Xf, 1, axis=0).astype(np.complex64), Xf)[0] > 1e3         # a frame too early
    assert dc.spec_units(np.conj(Xf).astype(np.complex64), Xf)[0] > 1e3
    assert dc.feat_units(np.roll(feat.reshape(-1, dc.NB), 1, axis=1).astype(np.float32), Xf)[0] > 1e3
    bad = Xf.astype(np.complex64)
    bad[60, 5] = 1e-30                                                                      # a silent frame must be zero
    assert dc.spec_units(bad, Xf)[0] == np.inf
    neg = Xf.astype(np.complex64)
    neg[60, 5] = -0.0                                                                       # ... of either sign
    assert dc.spec_units(neg, Xf)[0] <= 1.0
    nanf = feat.astype(np.float32)
    nanf[0, 0, 0] = np.nan
    assert dc.feat_units(nanf, Xf)[0] == np.inf
    floor = feat.astype(np.float32)
    floor[1, 3, 3] = -11.9999                                                               # silence: -12 to 2e-6
    assert dc.feat_units(floor, Xf)[0] == np.inf
    one_short = x[: dc.CHUNK].astype(np.float64).copy()      # one sample of 24000 missing from the sum
    one_short[12345] = 0.0
    short = dc.rms_units(np.array([np.sqrt((one_short ** 2).mean())], np.float32), rms[:1])[0]
    assert dc.RMS_TREE_UNITS < short < k4.GPU_FACTOR * dc.ORACLE_RMS_UNITS, short
    # K3: a chunk read from the wrong place, gains a row off, the interpolation weights swapped
    g = np.random.default_rng(1).uniform(0, 1, X.shape).astype(np.float32)
    s32 = X.astype(np.complex64)
    r = dc.ref_k3(s32, g)
    assert dc.den_units(r["out"].astype(np.float32), r).max() <= 1.0
    assert dc.den_units(dc.ref_k3(s32, np.roll(g, 1, axis=1))["out"].astype(np.float32), r).max() > 1e3
    sw = r["out"].astype(np.float32).reshape(-1, 3)[:, [1, 0, 2]].reshape(-1)
    assert dc.den_units(sw, r).max() > 1e3
    # fetch(pi < 0) reading chunk g instead of g - 1: chunk 2's first hop built on chunk 2's own last frame, not silence's
    wrong = dc.ref_k3(s32[2:], g[2:], ola_in=dc.ref_k3(s32[2:], g[2:])["ola_out"])["out"][: 3 * dc.HOP]
    right = r["out"].astype(np.float32).copy()
    right[2 * dc.CHUNK: 2 * dc.CHUNK + 3 * dc.HOP] = wrong
    u = dc.den_units(right, r)
    assert u[dc.seam_mask(3)].max() > 1e3 and u[~dc.seam_mask(3)].max() <= 1.0
    assert dc.seam_mask(3).sum() == 3 * 480 and dc.run_boundary_mask(1).sum() > 0
    # K1's to_next rows dropped: the warm-up rows of the next chunk keep stale values -- the bit-for-bit row rule of the GPU test


# ------------------------------------------------------------------ the input table's conditions

def test_chunk_table_meets_its_conditions():
    tab = dc.table()
    labels = [l for l, _ in tab]
    assert len(set(labels)) == len(labels) and all(x.dtype == np.float32 and x.shape == (dc.CHUNK,) for _, x in tab)
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(tab, dc.chunk_table()))           # deterministic
    for need in ["noise 1.0", "noise 1e-4", "quiet bins", "dc 0.5", "dc -1e-9", "nyquist", "full scale", "amplitude 1e-7", "silence",
                 "dropped 0.9"] + [f"tone {k}" for k in dc.TONE_BINS] + [f"impulse {p}" for p in (0, 159, 160, 7999)]:
        assert need in labels, need
    assert max(np.abs(x).max() for _, x in tab) == 1.0
    # neighbours differ, and so do neighbouring lanes; silence sits between loud chunks
    for i in range(N_TABLE - 1):
        assert not np.array_equal(tab[i][1][::3], tab[i + 1][1][::3]) or labels[i].startswith("flip")
    i = labels.index("silence")
    assert np.abs(tab[i - 1][1]).max() > 0.99 and np.abs(tab[i + 1][1]).max() == 1.0
    for lane in range(4):
        assert dc.lane_indices(lane, 5) != dc.lane_indices(lane + 1, 5)
    # every entry next to every other one it meets in a wrapped lane; spectra of the whole table
    X, feat, rms = dc.ref_lane_k1(dc.make_lane(0, WRAP))
    assert dc.significant_power_normal(X) == []
    p = np.abs(X) ** 2
    assert (p < dc.P_MIN).any() and (p > dc.P_MIN).any()
    for name in ("silence", "dropped 0.9"):
        c = labels.index(name)
        assert not X[c, 1:].any()                # (frame 0 still holds the previous chunk's last hop)
    quiet = p[labels.index("amplitude 1e-7"), 1:]       # the feature floor runs through this chunk: most bins under it, the rest
    assert (quiet < dc.P_MIN).mean() > 0.8 and (quiet > dc.P_MIN).any() and quiet.max() < 10 * dc.P_MIN     # just above
    assert rms[labels.index("dropped 0.9")] > 0.7 and rms[labels.index("silence")] == 0.0
    # the impulses sit where they should: decimated 159 is the last sample of hop 0, 160 the first of hop 1
    for pos in (0, 159, 160, 7999):
        x = tab[labels.index(f"impulse {pos}")][1]
        assert x[3 * pos] == 1.0 and np.count_nonzero(x) == 1
    # tone k is loudest in bin k
    for k in dc.TONE_BINS:
        assert int(np.argmax(np.abs(X[labels.index(f"tone {k}"), 10]))) == k
    # the launch sizes of the GPU tests take the forms they are meant to
    assert [dc.fft_parts(n) for n in (1, 2, 85, 86, 128, 129)] == [3, 3, 3, 2, 2, 1]
    assert dc.launch_sizes(129, 85) == [85, 44] and dc.launch_sizes(129, 128) == [128, 1] and dc.launch_sizes(129, 129) == [129]


def test_flip_tone_alternates_in_its_bin():
    labels = [l for l, _ in dc.table()]
    c = labels.index("flip tone b")
    _, feat, _ = dc.ref_lane_k1(dc.make_lane(0, WRAP))
    f = feat[c, :, dc.FLIP_BIN]
    # frames whose two hops carry the same sign (the odd ones, and frame 0 behind the first flip chunk) against the others
    assert (f[1::2] > 3.0).all() and f[0] > 3.0 and (f[2::2] < -0.5).all(), (f[:6])
    g = dc.closed_form_gains("select_alternating", feat[c])
    assert (g[1::2] > 0.999).all() and (g[2::2] < 0.001).all()        # every bin: frame f ~ 1, frame f + 1 ~ 0


# ------------------------------------------------------------------ gain models

def _model_features():
    """[54][161] f32 rows as the network sees them: table features (floor, loud, alternating) and a sweep of the range"""
    _, feat, _ = dc.ref_lane_k1(dc.make_lane(0, WRAP))
    rows = np.concatenate([feat[21, :20], feat[0, :10], feat[4, :10], feat[1, :4]]).astype(np.float32)
    sweep = np.linspace(-12.0, 5.0, 10 * dc.NB).reshape(10, dc.NB).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([rows, sweep]))


@pytest.mark.parametrize("name", dc.MODELS)
def test_gain_models_equal_their_closed_forms(name, capsys):
    w = dc.model_weights(name)
    shapes = orc.WEIGHT_SHAPES(*dc.DIMS)
    assert {k: v.shape for k, v in w.items()} == shapes and all(v.dtype == np.float32 for v in w.values())
    if name.startswith("select"):
        for k in ("fc1_w", "gru1_w", "gru2_w", "fc2_w", "fc3_w", "fc4_w"):
            assert (np.count_nonzero(w[k], axis=1) == 1).all(), k                   # one entry per row ...
            nz = np.abs(w[k][w[k] != 0]).astype(np.float64)
            assert np.array_equal(np.log2(nz), np.round(np.log2(nz))), k             # ... a power of two
        assert not w["gru1_r"].any() and not w["gru2_r"].any() and not w["gru1_b"][1200:].any() and not w["gru2_b"][1200:].any()
    f = _model_features()
    assert f.shape == (dc.ROWS, dc.NB)
    want = dc.closed_form_gains(name, f)
    g64 = _nsnet2_float64(w, f)
    assert np.abs(g64 - want).max() <= 1e-15, (name, np.abs(g64 - want).max())
    g_orc = orc.nsnet2_forward(w, f)
    e = np.abs(g_orc.astype(np.float64) - want).max()
    with capsys.disabled():
        print(f"\n    {name}: oracle gains {e:.3g} from the closed form (bound {dc.GAIN_ABS_TOL:.3g}); gains span "
              f"{want.min():.3g} .. {want.max():.3g}")
    assert e <= dc.GAIN_ABS_TOL, (name, e)
    if name == "bias_unity":
        assert (g_orc == 1.0).all()
    elif name == "bias_mixed":
        assert {0.5, 1.0} <= set(np.unique(g_orc)) and g_orc.min() < 1e-30 and (np.diff(g_orc, axis=0) == 0).all()
    else:
        assert want.min() < 0.05 and want.max() > 0.95
        assert (np.abs(np.diff(want, axis=0)).max(axis=0) > 0.1).all()               # every bin's gain moves between frames
        if name == "select_varied":
            assert (np.abs(np.diff(want, axis=1)).max(axis=1) > 0.1).all()           # ... and differs between bins


# ------------------------------------------------------------------ the oracle's own distance: the constants

def test_oracle_k1_stays_inside_the_recorded_constants(capsys):
    labels = [l for l, _ in dc.table()]
    x = dc.make_lane(0, WRAP)
    X, feat, rms = dc.ref_lane_k1(x)
    ws = wf = wr = 0.0
    at = {}
    for c in range(WRAP):
        s, f = dc.oracle_k1(_ai_of(x, c))
        for key, (w, pos) in (("spec", dc.spec_units(s, X[c])), ("feat", dc.feat_units(f, X[c]))):
            if w > at.get(key, (-1.0,))[0]:
                at[key] = (w, labels[c % N_TABLE], pos)
        w, _ = dc.rms_units(np.array([dc.oracle_rms(x[dc.CHUNK * c: dc.CHUNK * (c + 1)])], np.float32), rms[c: c + 1])
        if w > at.get("rms", (-1.0,))[0]:
            at["rms"] = (w, labels[c % N_TABLE], 0)
    ws, wf, wr = at["spec"][0], at["feat"][0], at["rms"][0]
    with capsys.disabled():
        print(f"\n    K1 oracle over {WRAP} chunks: spectrogram {ws:.4g} ({at['spec'][1]}, frame/bin {at['spec'][2]}); features "
              f"{wf:.4g} ({at['feat'][1]}, {at['feat'][2]}); rms {wr:.7g} ({at['rms'][1]})")
    for w, const in ((ws, dc.ORACLE_SPEC_UNITS), (wf, dc.ORACLE_FEAT_UNITS), (wr, dc.ORACLE_RMS_UNITS)):
        assert const / 3 <= w <= const, (w, const)      # measurements, not allowances
    # far below what an indexing mistake costs.  (Not so the RMS: the oracle's sequential f32 sum of 24000 squares is ~1300 units
    # off on a constant signal; the bound is the oracle's all the same, and the GPU test prints how far inside the kernel sits)
    assert k4.GPU_FACTOR * max(dc.ORACLE_SPEC_UNITS, dc.ORACLE_FEAT_UNITS) < 1e3


@pytest.mark.parametrize("name", dc.MODELS)
def test_oracle_k3_stays_inside_the_recorded_constants(name, capsys):
    # an orc.Denoiser under the gain model; the reference from the oracle's own pre-gain spectrogram, its own gains() rows
    # 4..53 and its own carries
    labels = [l for l, _ in dc.table()]
    x = dc.make_lane(0, WRAP)
    den = orc.Denoiser(dc.model_weights(name))
    ola, last, norm = None, 0.0, 0.0
    worst, where, seam = 0.0, None, 0.0
    for c in range(WRAP):
        rc, y = den.denoise(x[dc.CHUNK * c: dc.CHUNK * (c + 1)])
        assert rc == 0
        spec, _ = dc.oracle_k1(_ai_of(x, c))
        r = dc.ref_k3(spec[None], den.gains()[dc.WARM:][None], ola_in=ola, last_in=last, norm_in=norm)
        u = dc.den_units(y, r)
        i = int(np.argmax(u))
        if u[i] > worst:
            worst, where = float(u[i]), (labels[c % N_TABLE], i)
        seam = max(seam, float(u[: 3 * dc.HOP].max()))
        ao = dc.oracle_audio_output(den)
        ola, last, norm = ao[dc.DEC:], ao[dc.DEC - 1], r["norm_out"]
    with capsys.disabled():
        print(f"\n    K3 oracle under {name}: {worst:.4g} units at {where}; at chunk seams {seam:.3g}")
    const = dc.ORACLE_DEN_UNITS[name]
    assert const / 3 <= worst <= const, (name, worst, const)
    assert k4.GPU_FACTOR * const < 1e3
