"""Case tables, the float64 reference and the error metric shared by test_k4_bands_host.py and test_k4_bands_gpu.py: K4 (the
VAD-side real FFT, |X| * norm, the speech-band sums) against a float64 transform of exactly the samples the kernel was given,
one kernel at a time -- never against another path of the library.

Reference   ref_bins(x, F) = |rfft(f64(x) * f64(w))| * f64(norm), w the f32 periodic Hann window of the library and the oracle
            (orc.hann_periodic), norm the f32 value orc_window_norm_factor(w) / (float)F; ref_band(lo, hi) its f64 sum over
            lo..hi inclusive.
Metric      eps = 2^-24, X2 = ||ref_bins||_2 of the frame.  A bin's error counts in units of eps * X2; a band's in units of
            eps * (sqrt(n) * X2 + n * ref_band), n = hi - lo + 1: the transform's round-off (which scales with the frame's
            energy, not with the bin's own value: the metric stays tight for a quiet band under a loud one) plus the bound of an
            index-order f32 sum of n non-negative terms.  A frame whose reference spectrum is all zeros (digital silence) has no
            unit: there every output must be exactly +0.0.
Tolerance   the oracle's own worst distance over the whole table (ORACLE_BIN_UNITS / ORACLE_BAND_UNITS, per FFT size, measured
            on the CPU and asserted by test_k4_bands_host.py); a GPU kernel gets GPU_FACTOR times that: it is a valid f32
            transform of another factorisation (Stockham passes, a 16 x 32 split; kissfft goes radix-4 first), so its error is of
            the same order, not the same bits -- and an indexing or twiddle mistake costs O(1 / eps) units.
"""
import numpy as np

import orc

EPS = 2.0 ** -24
GPU_FACTOR = 4.0

WAVE_SIZES = [512, 1024, 2048]                              # vadfft_bands_kernel<R> (and the pruned kernel at 1024)
GENERIC_SIZES = [4, 6, 254, 960, 1000, 4096, 6250, 16384]   # rfft_generic_bands_kernel (16384: 131 KB of LDS, bins to 8192)
SIZES = sorted(WAVE_SIZES + GENERIC_SIZES)
ALL_BIN_SIZES = 2048    # one-hot tones walk every bin up to this size

# The oracle's worst distance from the float64 reference over frame_table(F) x band_set(F), in the units above, rounded up to
# two decimals.  Measured with
#   python -m pytest tests/test_k4_bands_host.py -k oracle_stays -s
# which prints the figures per size (and asserts that the oracle still stays inside these).
ORACLE_BIN_UNITS = {4: 1.08, 6: 1.07, 254: 4.78, 512: 2.85, 960: 2.31, 1000: 2.67, 1024: 3.28, 2048: 2.71, 4096: 2.19,
                    6250: 2.41, 16384: 2.18}
ORACLE_BAND_UNITS = {4: 0.56, 6: 0.70, 254: 4.00, 512: 1.57, 960: 1.35, 1000: 1.47, 1024: 1.81, 2048: 1.54, 4096: 1.21,
                     6250: 1.33, 16384: 1.20}

# bands of the pruned four-frames-per-wavefront kernel at 1024 points (inside bins 1..47) and their next-door neighbours, which
# the full-spectrum kernel takes: in one call both launch classes run and the rows scatter through `idx`
PRUNED_EDGES = [(1, 47), (1, 1), (47, 47), (16, 16), (32, 32), (15, 33)]
PRUNED_NEIGHBOURS = [(0, 47), (1, 48), (48, 48)]
BAND_COUNTS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600]


# ------------------------------------------------------------------ the reference

def window_and_norm(F):
    """(f32 window, f32 norm) as BufferedFFT.init makes them"""
    w = orc.hann_periodic(F)
    nf = np.float32(orc.lib().orc_window_norm_factor(orc.fptr(w), F))
    return w, np.float32(nf / np.float32(F))


def ref_bins(x, F):
    """x: [n_frames][F] (or [F]) f32 samples -> float64 [n_frames][F/2 + 1]"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.shape[-1] == F
    w, norm = window_and_norm(F)
    return np.abs(np.fft.rfft(x.astype(np.float64) * w.astype(np.float64), axis=-1)) * np.float64(norm)


def ref_band(bins, lo, hi):
    """float64 sum of bins lo..hi inclusive, per frame"""
    return np.asarray(bins)[..., lo:hi + 1].sum(axis=-1)


def bin_units(got, bins):
    """got, bins: [n_frames][NB].  Worst |got - bins| / (eps X2) over the frames that have a spectrum; a silent frame (X2 == 0)
    counts inf unless every value is exactly +0.0.  Returns (worst, (frame, bin))."""
    got = np.asarray(got)
    x2 = np.sqrt((bins * bins).sum(axis=1))
    u = _units(got, bins, EPS * x2[:, None] * np.ones_like(bins))
    i = np.unravel_index(np.argmax(u), u.shape)
    return float(u[i]), tuple(int(v) for v in i)


def band_units(got, bins, bands):
    """got: [n_bands][n_frames] f32 band sums; bins: ref_bins of the frames.  Worst |got - ref_band| / (eps (sqrt(n) X2 + n
    ref_band)); silent frames as in bin_units.  Returns (worst, (band index, frame))."""
    got = np.asarray(got)
    assert got.shape == (len(bands), bins.shape[0]), (got.shape, len(bands), bins.shape)
    x2 = np.sqrt((bins * bins).sum(axis=1))
    ref = np.stack([ref_band(bins, lo, hi) for lo, hi in bands])
    n = np.array([hi - lo + 1 for lo, hi in bands], np.float64)[:, None]
    u = _units(got, ref, EPS * (np.sqrt(n) * x2[None, :] + n * ref))
    i = np.unravel_index(np.argmax(u), u.shape)
    return float(u[i]), tuple(int(v) for v in i)


def _units(got, ref, unit):
    assert got.dtype == np.float32 and got.shape == ref.shape
    err = np.abs(got.astype(np.float64) - ref)
    silent = unit == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(silent, 0.0, err / np.where(silent, 1.0, unit))
    pos_zero = got.view(np.uint32) == 0
    u[silent & ~pos_zero] = np.inf      # exactly +0.0 where the reference has nothing at all
    u[~np.isfinite(got)] = np.inf
    return u


# ------------------------------------------------------------------ the oracle's K4 (orc_buffered_fft_frame + orc_band_sum)

def oracle_bins(x, F):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros((x.shape[0], F // 2 + 1), np.float32)
    for i in range(x.shape[0]):
        orc.lib().orc_buffered_fft_frame(orc.fptr(x[i]), F, orc.fptr(out[i]))
    return out


def oracle_bands(obins, bands):
    """[n_bands][n_frames] f32 from the oracle's magnitudes"""
    L = orc.lib()
    out = np.zeros((len(bands), obins.shape[0]), np.float32)
    for f in range(obins.shape[0]):
        p = orc.fptr(obins[f])
        for j, (lo, hi) in enumerate(bands):
            out[j, f] = L.orc_band_sum(p, lo, hi)
    return out


# ------------------------------------------------------------------ inputs

def tone_bins(F):
    """bins the one-hot tones visit: every bin up to 2048 points; above, bins 0..49, a stride through the middle, the last 3"""
    h = F // 2
    if F <= ALL_BIN_SIZES:
        return list(range(h + 1))
    return sorted(set(range(50)) | set(range(50, h - 2, max(1, h // 16) + 1)) | {h - 2, h - 1, h})


TONE_AMPS = [1.0, 0.25, 0.9, 1e-3, 0.5, 1e-6, 0.7, 1e-9]


def one_hot_tone(F, k, i=0):
    """amplitude-A sine exactly on bin k; the phase keeps bins 0 and F/2 (where a sine of phase 0 vanishes) alive"""
    n = np.arange(F, dtype=np.float64)
    return (TONE_AMPS[i % len(TONE_AMPS)] * np.sin(2.0 * np.pi * k * n / F + 0.7 + 0.37 * (i % 5))).astype(np.float32)


def quiet_band_frame(F, seed=2):
    """a 0.9 tone at a non-integer low bin over 1e-4 noise: every other band sits some 80 dB under the loudest bin"""
    n = np.arange(F, dtype=np.float64)
    k = 2.37 if F >= 32 else 0.37
    noise = np.random.default_rng(1000 * F + seed).uniform(-1e-4, 1e-4, F)
    return (0.9 * np.sin(2.0 * np.pi * k * n / F + 0.3) + noise).astype(np.float32)


def fixed_frames(F):
    """[(label, frame)]: everything of the table except the one-hot tones"""
    rng = np.random.default_rng(77 * F + 1)
    out = [("noise 1.0", rng.uniform(-1.0, 1.0, F).astype(np.float32)),
           ("noise 1.0 b", rng.uniform(-1.0, 1.0, F).astype(np.float32)),
           ("noise 1e-4", rng.uniform(-1e-4, 1e-4, F).astype(np.float32)),
           ("quiet band", quiet_band_frame(F)),
           ("dc", np.full(F, 0.5, np.float32)),
           ("dc 1e-9", np.full(F, -1e-9, np.float32)),
           ("nyquist", (0.5 * (1.0 - 2.0 * (np.arange(F) % 2))).astype(np.float32))]
    for pos in (1, F // 2, F - 1):      # (sample 0 meets the window's zero: the frame would be silence)
        x = np.zeros(F, np.float32)
        x[pos] = 1.0
        out.append((f"impulse {pos}", x))
    out.append(("silence", np.zeros(F, np.float32)))
    return out


def frame_table(F):
    """(frames [n][F] f32, labels): the fixed frames, then one one-hot tone per bin of tone_bins(F)"""
    fx = fixed_frames(F)
    labels = [l for l, _ in fx] + [f"tone {k}" for k in tone_bins(F)]
    frames = [x for _, x in fx] + [one_hot_tone(F, k, i) for i, k in enumerate(tone_bins(F))]
    return np.ascontiguousarray(np.stack(frames), np.float32), labels


def sweep_frames(F):
    """the short table of the band-count sweeps and the geometry tests: the fixed frames and a few tones"""
    h = F // 2
    ks = sorted({k for k in (1, 15, 16, 17, 32, 47, 48, h - 1) if 0 <= k <= h})
    fx = fixed_frames(F)
    frames = [x for _, x in fx] + [one_hot_tone(F, k, i) for i, k in enumerate(ks)]
    return np.ascontiguousarray(np.stack(frames), np.float32), [l for l, _ in fx] + [f"tone {k}" for k in ks]


def speech_band(F, rate=48000):
    """the reference's 500-2000 Hz at this size (11..43 at 1024 points)"""
    L = orc.lib()
    return int(L.orc_fft_freq_to_bin(F, rate, 500.0)), int(L.orc_fft_freq_to_bin(F, rate, 2000.0))


def clip_band(F, lo, hi):
    h = F // 2
    lo = min(max(lo, 0), h)
    return lo, min(max(hi, lo), h)


def edge_bands(F):
    """the bands that are not single bins: the whole spectrum and its ends, the speech band, and -- at every size, clipped to
    it -- the pruned kernel's edges at 1024 points with their neighbours"""
    h = F // 2
    out = [(0, 0), (0, h), (h, h), speech_band(F)]
    out += [clip_band(F, lo, hi) for lo, hi in PRUNED_EDGES + PRUNED_NEIGHBOURS]
    out += [(11, 43)] if h >= 43 else []
    return out


def band_set(F):
    """single bins for every bin the tones visit, the edge bands, duplicates"""
    singles = [(k, k) for k in tone_bins(F)]
    edges = edge_bands(F)
    return singles + edges + [singles[0], singles[-1], edges[1], edges[3]]


def cycled_bands(F, count, pruned_only=False):
    """`count` bands: the edge bands and some single bins, cycled, each round with other edges; duplicates stay in (the same
    band returns every few rounds).  pruned_only: every band inside bins 1..47 (1024 points: one launch class)."""
    h = F // 2
    base = edge_bands(F) + [(k, k) for k in (0, 1, 2, 16, 32, 47, 48, h - 1, h) if k <= h]
    lo_min, hi_max = (1, min(47, h)) if pruned_only else (0, h)
    if pruned_only:
        base = [b for b in base if b[0] >= 1 and b[1] <= 47]
    out = []
    for i in range(count):
        lo, hi = base[i % len(base)]
        r = (i // len(base)) % 4            # round r: grow the band by r bins on alternating sides
        lo, hi = (lo - r, hi) if i % 2 else (lo, hi + r)
        lo = min(max(lo, lo_min), hi_max)
        out.append((lo, min(max(hi, lo), hi_max)))
    return out


def significant_bins_normal(frames, F):
    """the normal-range condition on the inputs: in every frame, |X|^2 (before norm) of each bin that reaches one unit of the
    metric lies inside normal f32.  Returns the offending (frame, bin) pairs."""
    bins = ref_bins(frames, F)
    _, norm = window_and_norm(F)
    x2 = np.sqrt((bins * bins).sum(axis=1))
    sq = (bins / np.float64(norm)) ** 2
    sig = bins >= EPS * x2[:, None]
    sig &= x2[:, None] > 0
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    bad = sig & ((sq < tiny) | (sq > huge))
    return [tuple(int(v) for v in i) for i in np.argwhere(bad)]

