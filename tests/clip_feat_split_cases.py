"""The layouts, the seam table and the numpy model of the split-source feature exports (fvad_clips_export_split_mel*,
fvad_clips_export_split_fbank*; test_clips_feat_split_host.py, test_clips_feat_split_gpu.py).  The yardsticks are
clip_mel_cases.py's and clip_fbank_cases.py's float64 models and tolerances as they are: a split export has to give the
contiguous export's bits, so no new number is needed.

The mapping (include/fvad.h): stream sample i of a clip is clip sample e = skip + i * step, in piece A when e < a_len, else in
piece B at e - a_len; n_a = ceil((a_len - skip) / step) of them lie in A (0 for a_len <= skip).  The stride is counted from the
clip's first sample and runs through the seam: B's first kept sample is wherever the stride lands in B."""
import numpy as np

import clip_fbank_cases as fc
import clip_mel_cases as mc
from clip_split_cases import FEW_PAIRS  # noqa: F401  (the piece offsets the GPU test rotates through)

SENTINEL = np.int16(32767)       # full scale: a PCM16 sample that must never reach a feature
SPLIT_FIELDS = 7


def n_a(a_len, skip, step):
    """the stream samples that lie in piece A"""
    return -(-(a_len - skip) // step) if a_len > skip else 0


def split_stream(pa, pb, skip, step, mutation=None):
    """the feature stream (in the pieces' dtype) of one channel given as its two pieces.  mutation: "drop" (the first kept
    sample of B dropped), "dup" (it is read twice), "b_from" (B read from its first sample on, whatever the stride's phase)"""
    a_len = len(pa)
    na = n_a(a_len, skip, step)
    first_b = skip + na * step - a_len          # where the stride lands in B
    if mutation == "b_from":
        first_b = 0
    sa, sb = pa[skip::step], pb[first_b::step]
    assert len(sa) == na
    if mutation == "drop":
        sb = sb[1:]
    if mutation == "dup":
        sb = np.concatenate([sb[:1], sb])
    return np.concatenate([sa, sb])


def mel_reflect_a_only(pa, pb, skip, step, w, M, hop, floor=mc.FLOOR):
    """the wrong log-mel model whose reflected taps in front of the clip are taken from piece A alone: tap j < 0 reads clip
    sample min(skip - j * step, a_len - 1) of A; every other tap is right.  float64 features [T][n_mels]"""
    s = mc.to_f32(split_stream(pa, pb, skip, step)).astype(np.float64)
    a = mc.to_f32(pa).astype(np.float64)
    L, n_fft = len(s), len(w)
    j = np.arange(L // hop)[:, None] * hop + np.arange(n_fft)[None, :] - n_fft // 2
    right = s[np.clip(np.where(j >= L, 2 * (L - 1) - j, np.abs(j)), 0, L - 1)]
    wrong = a[np.clip(skip + np.abs(j) * step, 0, len(a) - 1)]
    X = np.fft.rfft(np.where(j < 0, wrong, right) * np.asarray(w, np.float64), axis=1)
    return np.log10(np.maximum((X.real ** 2 + X.imag ** 2) @ np.asarray(M, np.float64).T, np.float64(np.float32(floor))))


def seams(n, skip, step, taps, hop, centred, tile_frames):
    """The seam table of a clip of n samples: a_len values in [0, n].  taps: n_fft (centred: the log-mel frames, reflected over
    n_fft / 2 stream samples at both ends) or win (frames from t * hop on)."""
    L = -(-(n - skip) // step)
    pad = taps // 2 if centred else 0
    T = L // hop if centred else 1 + (L - taps) // hop
    m = L // 2
    s = {0, 1, skip, skip + 1, m * step + skip - 1, m * step + skip, m * step + skip + 1, n - 1, n}
    quarter = step * taps // 4
    if quarter > 1:
        s |= {quarter // 2 + 1, n - (quarter // 2 + 1)}     # inside the left and the right reflected zone (a_len, b_len < step taps / 4)
    if T > tile_frames:                                      # tile 1's staged window [w0, w1): its first and last source sample
        w0 = max(tile_frames * hop - pad, 0)
        w1 = min((min(2 * tile_frames, T) - 1) * hop - pad + taps, L)
        for e in (skip + w0 * step, skip + (w1 - 1) * step):
            s |= {e - 1, e, e + 1}
    t = T // 2                                               # the first tap of a frame
    e = skip + max(t * hop - pad, 0) * step
    s |= {e - 1, e, e + 1}
    return sorted(v for v in s if 0 <= v <= n)


class Layout:
    """Clips laid out twice: contiguous in `host` [n_lanes][stride] (rows [n][4]) and as two pieces in A and B (split [n][7]),
    both buffers of the same dtype, filled with NaN (f32) or SENTINEL (PCM16) wherever no clip sample lies, every piece with at
    least one such sample on both sides.  A and B have other lane counts, strides and lane orders than the contiguous source."""

    def __init__(self, pcm16):
        self.pcm16 = pcm16
        self.items = []          # dict(lanes [C][n], a_len, skip, step, off=(x, y))

    def add(self, lanes, a_len, skip, step, off=(0, 0), **tags):
        lanes = np.asarray(lanes)
        assert 0 <= a_len <= lanes.shape[1]
        self.items.append(dict(lanes=lanes, a_len=int(a_len), skip=int(skip), step=int(step), off=off, **tags))
        return len(self.items) - 1

    def build(self):
        per16 = 8 if self.pcm16 else 4
        dt = np.int16 if self.pcm16 else np.float32
        fill = SENTINEL if self.pcm16 else np.nan
        cmax = max(it["lanes"].shape[0] for it in self.items)
        self.n_lanes, self.a_lanes, self.b_lanes = cmax + 1, cmax + 2, cmax + 3
        at, at_a, at_b = 5, 3, 6
        place = []
        for it in self.items:
            n, na = it["lanes"].shape[1], it["a_len"]
            place.append((at, at_a, at_b))
            at += n + 3
            at_a += na + per16 + 2
            at_b += n - na + per16 + 2
        self.n_samples, self.a_samples, self.b_samples = at + 7, at_a + per16, at_b + per16
        self.stride, self.a_stride, self.b_stride = self.n_samples + 5, self.a_samples + 3 | 1, self.b_samples + 7 | 1
        self.host = np.full((self.n_lanes, self.stride), fill, dt)
        self.A = np.full((self.a_lanes, self.a_stride), fill, dt)
        self.B = np.full((self.b_lanes, self.b_stride), fill, dt)
        rows, split = [], []
        for k, (it, (c0, ca, cb)) in enumerate(zip(self.items, place)):
            x = it["lanes"]
            C_, n = x.shape
            na = it["a_len"]
            l0, la, lb = k % (self.n_lanes - C_ + 1), (k + 1) % (self.a_lanes - C_ + 1), (k + 2) % (self.b_lanes - C_ + 1)
            fa = ca + (it["off"][0] - (la * self.a_stride + ca)) % per16     # the first channel's address offset within 16 bytes
            fb = cb + (it["off"][1] - (lb * self.b_stride + cb)) % per16
            self.host[l0:l0 + C_, c0:c0 + n] = x
            self.A[la:la + C_, fa:fa + na] = x[:, :na]
            self.B[lb:lb + C_, fb:fb + n - na] = x[:, na:]
            rows.append((l0, C_, c0, c0 + n))
            split.append((C_, la if na else 0, fa if na else 0, na, lb if na < n else 0, fb if na < n else 0, n - na))
        self.rows, self.split = np.array(rows, np.uint64), np.array(split, np.uint64)
        return self

    def a(self, address=None):
        return (address, self.a_lanes, self.a_stride, self.a_samples)

    def b(self, address=None):
        return (address, self.b_lanes, self.b_stride, self.b_samples)

    def skips(self, idx):
        return np.array([self.items[i]["skip"] for i in idx], np.uint32)

    def pieces(self, i, ch):
        """channel ch of clip i as the split row addresses it: (piece A, piece B), read back from the buffers"""
        C_, la, fa, na, lb, fb, nb = (int(v) for v in self.split[i])
        return self.A[la + ch, fa:fa + na], self.B[lb + ch, fb:fb + nb]

    def stream(self, i, mutation=None):
        """(picked channel, the split model's stream of clip i) -- the pick over every sample of the clip"""
        it = self.items[i]
        ch = mc.pick(it["lanes"])
        pa, pb = self.pieces(i, ch)
        return ch, mc.to_f32(split_stream(pa, pb, it["skip"], it["step"], mutation))


def clip_lanes(rng, L, step, skip, C_, pick, signal, pcm16, canaries, tail=None):
    """[C_][n] samples whose channel `pick` carries `signal` on its kept samples and is the quietest.  canaries (one channel): every
    off-stride sample is NaN (f32) or full scale (PCM16)"""
    n = skip + (L - 1) * step + 1 + (int(rng.integers(0, step)) if tail is None else tail)
    s = mc.signal(signal, L, rng)
    scale = max(float(np.abs(s).max()), 1e-3)
    lanes = []
    for c in range(C_):
        g = 1.0 if c == pick else 2.0 + 0.5 * c
        x = (g * 0.7 * scale * rng.standard_normal(n)).astype(np.float32)
        if c == pick:
            if canaries:
                x[:] = np.nan
            x[skip::step] = s
        lanes.append(x)
    return quantise(np.stack(lanes), pcm16, canaries)


def quantise(x, pcm16, canaries=False):
    if not pcm16:
        return x.astype(np.float32)
    q = np.clip(np.rint(np.nan_to_num(x) * 8192.0), -32768, 32767).astype(np.int16)
    if canaries:
        q[np.isnan(x)] = SENTINEL
    return q


def seam_pick_lanes(rng, n, a_len, pcm16):
    """three channels of n samples whose quietest over the whole clip is channel 2, while over piece A alone it is channel 0
    and over piece B alone channel 1: the pick is decided only across the seam"""
    x = np.stack([rng.standard_normal(n) * np.where(np.arange(n) < a_len, 0.05, 0.9),
                  rng.standard_normal(n) * np.where(np.arange(n) < a_len, 0.9, 0.05),
                  rng.standard_normal(n) * 0.3]).astype(np.float32)
    q = quantise(x, pcm16)
    assert mc.pick(q) == 2 and mc.pick(q[:, :a_len]) == 0 and mc.pick(q[:, a_len:]) == 1
    return q


def mel_model(stream, shape, w, M, floor=mc.FLOOR):
    return mc.model(stream, w, M, shape[1], floor)


def fbank_model(stream, shape, w, M, scale, floor=fc.FLOOR):
    return fc.model(stream, w, M, shape, scale=scale, floor=floor)
