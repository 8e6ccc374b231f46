"""Case tables and input builders shared by test_vad_oracle_host.py and test_vad_oracle_gpu.py: the VAD sweep stack (bands, ring
lengths, frame ratios, the machines with their lazy long-term bound, the scorer) against the CPU oracle (orc_vad, orc_pipeline,
orc_stats), never against the library's own host path.

The oracle side is always orc_vad_create + orc_vad_run (one machine per (stream, config)), fed the same band sums and frame
ratios as the library; its audit is restated from the per-frame trace with the formula of vad_machine.h's decide()."""
import ctypes as C
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import orc

# (sample rate, channels, FFT size): frames inside one chunk, across two, across three (16 kHz: 8000-sample chunks), sizes that
# do not divide the chunk, rates other than 48 kHz
CASES = [(48000, 1, 1024), (48000, 2, 512), (48000, 2, 2048), (48000, 3, 960), (48000, 2, 1000), (16000, 2, 16384),
         (96000, 1, 4096), (32000, 2, 254)]
CASE_IDS = ["%dk-%dch-F%d" % (r // 1000, c, f) for r, c, f in CASES]
# seconds of audio per case: enough frames for segments, the oracle pipeline about 2 s per case
CASE_SECONDS = {(48000, 1, 1024): 24.0, (48000, 2, 512): 16.0, (48000, 2, 2048): 16.0, (48000, 3, 960): 12.0,
                (48000, 2, 1000): 16.0, (16000, 2, 16384): 60.0, (96000, 1, 4096): 16.0, (32000, 2, 254): 16.0}

# ring lengths the lazy bound and the device's exact chain (blocks of 64 slots, re-anchor after 4096 lazy pushes) must get right:
# 8437 = 180 s at 1024 points, 16875 = 180 s at 512
RINGS = [1, 2, 63, 64, 65, 4096, 8437, 16875]
LONG_SIZES = [512, 1024, 2048]
LONG_RATE, LONG_CHUNK = 48000, 24000

POOL = min(16, os.cpu_count() or 1)

TRACE_DT = np.dtype([("index", "<u8"), ("min_volume", "<f4"), ("short_term", "<f8"), ("channel_vol_ratio", "<f8"),
                     ("threshold", "<f8"), ("threshold_met", "<i4"), ("state_after", "<i4")], align=True)
assert TRACE_DT.itemsize == C.sizeof(orc.VadTrace)


def chunk_of(rate):
    return int(orc.lib().orc_nsnet2_chunk_size(rate))


# ------------------------------------------------------------------ ring lengths and band edges as f32 sees them

def ring_len(rate, F, sec):
    """(size_t)(rate / F * sec) in f32 (VADMachine.zig:75-106), before any @max clamp"""
    p = np.float32(np.float32(rate) / np.float32(F)) * np.float32(sec)
    return int(p)


def sec_for_ring(rate, F, n):
    """(on, below): the smallest f32 seconds whose product reaches n (exactly n where f32 has such a product), and the f32 just
    below it, whose product is the largest below n -- truncated to n - 1 slots (lround would say n)"""
    e = np.float32(np.float32(rate) / np.float32(F))
    x = np.float32(n / float(e))
    while np.float32(e * x) < n:
        x = np.nextafter(x, np.float32(np.inf))
    while True:
        y = np.nextafter(x, np.float32(0))
        if np.float32(e * y) < n:
            break
        x = y
    return float(x), float(np.nextafter(x, np.float32(0)))


def half_bin_edge(rate, F, k):
    """an f32 frequency whose f32 quotient by the bin width is exactly k + 0.5 (or the nearest to it from above)"""
    bw = np.float32(np.float32(rate) / np.float32(F))
    x = np.float32((k + 0.5) * float(bw))
    for _ in range(64):
        q = np.float32(x / bw)
        if q == np.float32(k + 0.5):
            return float(x)
        x = np.nextafter(x, np.float32(np.inf) if q < k + 0.5 else np.float32(0))
    return float(x)


def freq_to_bin(rate, F, f):
    return int(orc.lib().orc_fft_freq_to_bin(F, rate, float(f)))


def band_edges(rate, F):
    """speech band edges at this rate and size: 0, Nyquist, half bins on even and odd k, non-integer Hz"""
    nyq = rate / 2.0
    nb = F // 2
    ks = sorted({2, 3, max(2, nb // 8) & ~1, max(3, nb // 8) | 1, max(4, nb // 3) & ~1, max(5, nb // 3) | 1})
    edges = [0.0, nyq, 437.3, 1733.71, 2999.99] + [half_bin_edge(rate, F, k) for k in ks if k + 1 < nb]
    return [e for e in edges if e <= nyq]


# ------------------------------------------------------------------ configs

def edge_configs(rate, F):
    """the edge table of one (rate, F): ring clamps and exact / one-ulp-below ring lengths, ties, thresholds <= 0, band edges"""
    nyq = rate / 2.0
    on = {n: sec_for_ring(rate, F, n) for n in (1, 2, 63, 64, 65)}
    fast = {"has_initial_long_term_avg": 0, "min_consecutive_sec_to_open": 0.0, "min_vad_duration_sec": 0.0, "max_speech_gap_sec": 0.5}
    out = [{},
           {"long_term_speech_avg_sec": 0.0, "short_term_speech_avg_sec": 0.0, **fast},       # both @max(1, ..) clamps
           {"speech_threshold_factor": 1.0, "short_term_speech_avg_sec": on[1][0], "initial_long_term_avg": 0.5},
           {"initial_long_term_avg": 0.0, "speech_threshold_factor": 0.0},                    # threshold 0 throughout
           {"initial_long_term_avg": 0.0, "speech_threshold_factor": 3.0, "long_term_speech_avg_sec": 5.0},
           {"speech_threshold_factor": 0.0, "has_initial_long_term_avg": 0, "long_term_speech_avg_sec": on[64][0]},
           {"speech_min_freq": 0.0, "speech_max_freq": nyq, "speech_threshold_factor": 2.0, **fast},
           {"min_consecutive_sec_to_open": 0.0, "max_speech_gap_sec": 0.0, "min_vad_duration_sec": 0.0, "speech_threshold_factor": 2.0}]
    for n in (1, 2, 63, 64, 65):
        for which in (0, 1):
            out.append({"long_term_speech_avg_sec": on[n][which], "speech_threshold_factor": 2.0 + 0.25 * which, **fast})
    # one-slot and two-slot short-term and channel-ratio rings, on and one ulp below
    out += [{"short_term_speech_avg_sec": on[2][1], "channel_vol_ratio_avg_sec": on[1][0], "speech_threshold_factor": 3.0,
             "long_term_speech_avg_sec": 10.0},
            {"short_term_speech_avg_sec": on[2][0], "channel_vol_ratio_avg_sec": on[2][1], "speech_threshold_factor": 3.0,
             "long_term_speech_avg_sec": 10.0},
            {"channel_vol_ratio_avg_sec": on[2][0], "channel_vol_ratio_threshold": 0.6, "speech_threshold_factor": 2.5,
             "long_term_speech_avg_sec": 8.0},
            {"channel_vol_ratio_avg_sec": on[64][1], "channel_vol_ratio_threshold": 0.9, "speech_threshold_factor": 2.5,
             "long_term_speech_avg_sec": 8.0, "short_term_speech_avg_sec": on[65][1]}]
    edges = band_edges(rate, F)
    for i, lo in enumerate(edges):
        hi = edges[(i + 3) % len(edges)]
        lo, hi = min(lo, hi), max(lo, hi)
        out.append({"speech_min_freq": lo, "speech_max_freq": hi, "speech_threshold_factor": 3.0, "long_term_speech_avg_sec": 12.0,
                    "has_initial_long_term_avg": 0})
    return out


def random_configs(rate, n, seed):
    """draws in the style of test_vad_sweep_gpu.sweep_configs, bands below this rate's Nyquist"""
    rng = np.random.default_rng(seed)
    nyq = rate / 2.0
    bands = [(500.0, 2000.0), (300.0, 3400.0), (1000.0, 4000.0), (200.0, 1200.0), (123.4, 0.45 * nyq)]
    out = []
    for _ in range(n):
        lo, hi = bands[rng.integers(len(bands))]
        c = {"speech_min_freq": lo, "speech_max_freq": min(hi, nyq), "long_term_speech_avg_sec": float(rng.choice([2.0, 6.0, 15.0, 30.0])),
             "short_term_speech_avg_sec": float(rng.uniform(0.05, 0.6)), "speech_threshold_factor": float(rng.uniform(1.5, 8.0)),
             "channel_vol_ratio_avg_sec": float(rng.uniform(0.1, 2.0)), "channel_vol_ratio_threshold": float(rng.uniform(0.2, 0.6)),
             "min_consecutive_sec_to_open": float(rng.uniform(0.0, 0.5)), "max_speech_gap_sec": float(rng.uniform(0.0, 3.0)),
             "min_vad_duration_sec": float(rng.uniform(0.0, 1.0))}
        if rng.uniform() < 0.4:
            c["has_initial_long_term_avg"] = 0
        else:
            c["initial_long_term_avg"] = float(rng.uniform(0.05, 1.0))
        out.append(c)
    return out


def case_configs(rate, F, seed):
    """about 40 configs of one case whose channel-ratio ring is not empty (those are refused: test f)"""
    cfgs = edge_configs(rate, F)
    cfgs += random_configs(rate, max(0, 40 - len(cfgs)), seed)
    one = sec_for_ring(rate, F, 1)[0]
    for c in cfgs:   # at 16 kHz and 16384 points a frame is ~1 s: widen the default and drawn ratio windows to one slot at least
        if ring_len(rate, F, c.get("channel_vol_ratio_avg_sec", 0.5)) < 1:
            c["channel_vol_ratio_avg_sec"] = one
    return cfgs


def long_configs(F):
    """the long-stream configs at one size: every ring of RINGS exactly and one f32 ulp below, ties with factor 1 and a one-frame
    short window, thresholds <= 0"""
    out = []
    one = sec_for_ring(LONG_RATE, F, 1)[0]
    for k, n in enumerate(RINGS):
        for which, x in enumerate(sec_for_ring(LONG_RATE, F, n)):
            c = {"long_term_speech_avg_sec": x, "speech_threshold_factor": [10.0, 4.0, 1.0, 2.0][(2 * k + which) % 4]}
            if (2 * k + which) % 4 >= 2:
                c["short_term_speech_avg_sec"] = one
            if k % 2:
                c["has_initial_long_term_avg"] = 0
            out.append(c)
    out += [{"initial_long_term_avg": 0.0, "speech_threshold_factor": 0.0},
            {"initial_long_term_avg": 0.0, "speech_threshold_factor": 1.0, "short_term_speech_avg_sec": one, "long_term_speech_avg_sec": 30.0},
            {"speech_threshold_factor": 1.0, "short_term_speech_avg_sec": one, "has_initial_long_term_avg": 0,
             "min_consecutive_sec_to_open": 0.0, "max_speech_gap_sec": 0.0, "min_vad_duration_sec": 0.0},
            {"speech_threshold_factor": 2.0, "short_term_speech_avg_sec": one, "long_term_speech_avg_sec": sec_for_ring(LONG_RATE, F, 64)[0],
             "has_initial_long_term_avg": 0, "min_vad_duration_sec": 0.0}]
    return out


# ------------------------------------------------------------------ inputs

def stream(pkg, rate, nch, seconds, seed):
    """synth.make_stream's audio, its samples read at `rate`"""
    pcm, _ = pkg.synth.make_stream(seconds * rate / 48000.0, seed=seed, n_channels=nch)
    if nch > 1:   # quieter channels, so that the channel ratio moves
        pcm = pcm * np.linspace(1.0, 0.7, nch, dtype=np.float32)[:, None]
    return np.ascontiguousarray(pcm, np.float32)


def oracle_case(pkg, weights, rate, nch, F, seed=1):
    """the oracle's inputs of one case -> dict.  At 48 kHz one orc_pipeline run (keep_denoised: every frame's bins kept).  The
    reference pipeline takes 48 kHz only (VADPipeline.zig:54-57), so at other rates the frames are the undenoised audio's:
    orc_buffered_fft_frame per frame, orc_rms_volume per chunk, and the frame ratios through orc_meta_push (oracle_frame_ratios)."""
    pcm = stream(pkg, rate, nch, CASE_SECONDS[(rate, nch, F)], seed)
    chunk = chunk_of(rate)
    out = {"rate": rate, "nch": nch, "F": F, "chunk": chunk, "pcm": pcm, "pipeline": rate == 48000}
    if rate != 48000:
        L = orc.lib()
        n_chunks = pcm.shape[1] // chunk
        nf = n_chunks * chunk // F
        rms = np.empty((n_chunks, nch), np.float32)
        for k in range(n_chunks):
            for c in range(nch):
                x = np.ascontiguousarray(pcm[c, k * chunk:(k + 1) * chunk])
                rms[k, c] = L.orc_rms_volume(orc.fptr(x), chunk, None, 0)
        bins = np.empty((nf, nch, F // 2 + 1), np.float32)
        for k in range(nf):
            for c in range(nch):
                L.orc_buffered_fft_frame(orc.fptr(np.ascontiguousarray(pcm[c, k * F:(k + 1) * F])), F, orc.fptr(bins[k, c]))
        out.update(rms=rms, bins=bins, ratio=oracle_frame_ratios(rms, nf, F, chunk))
        return out
    p = orc.Pipeline(weights, n_channels=nch, keep_denoised=True, sample_rate=rate, fft_size=F)
    assert p.err == 0
    p.push(pcm)
    nf = int(orc.lib().orc_pipeline_n_fft_frames(p.h))
    bins = np.empty((nf, nch, F // 2 + 1), np.float32)
    for k in range(nf):
        for c in range(nch):
            bins[k, c] = p.fft_bins(k, c)
    out.update(rms=p.chunk_rms(), ratio=p.frame_vol_ratio(), bins=bins, segments=p.segments(), band=p.band_volumes())
    p.__del__()
    return out


def oracle_frame_ratios(rms, n_frames, F, chunk):
    """the frame ratios of chunk RMS [n_chunks][nch] through the oracle's VADMetadata (orc_meta_push / orc_meta_to_result): the
    analyzer's and the denoiser's hand-over of each chunk (BufferedVolumeAnalyzer.zig:33-45, BufferedDenoiser.zig:83-86,115),
    then every chunk piece of a frame weighted by its sample count (BufferedFFT.zig:137-140)"""
    L = orc.lib()
    per_chunk = []
    for row in np.asarray(rms, np.float32):
        vmin, vmax = np.float32(1), np.float32(0)   # BufferedVolumeAnalyzer.analyseVolume (:48-69)
        for v in row:
            vmin, vmax = min(vmin, v), max(vmax, v)
        va = orc.MetaResult(1, 1, 1, 0.0 if vmax == 0 else float(np.float32(vmin / vmax)), float(vmin), float(vmax))
        for _ in range(2):
            m = orc.Meta()
            L.orc_meta_reset(C.byref(m))
            L.orc_meta_push(C.byref(m), C.byref(va), float(chunk))
            va = L.orc_meta_to_result(C.byref(m))
        per_chunk.append(va)
    out = np.empty(n_frames, np.float32)
    for f in range(n_frames):
        m = orc.Meta()
        L.orc_meta_reset(C.byref(m))
        lo, hi = f * F, (f + 1) * F
        for c in range(lo // chunk, (hi - 1) // chunk + 1):
            L.orc_meta_push(C.byref(m), C.byref(per_chunk[c]), float(min(hi, (c + 1) * chunk) - max(lo, c * chunk)))
        out[f] = L.orc_meta_to_result(C.byref(m)).volume_ratio
    return out


def oracle_cases(pkg, weights):
    with ThreadPoolExecutor(POOL) as ex:
        return list(ex.map(lambda c: oracle_case(pkg, weights, *c), CASES))


def band_sums(bins, lo, hi):
    """orc_band_sum over bins [n_frames][nch][nb] -> [nch][n_frames]"""
    L = orc.lib()
    nf, nch, _ = bins.shape
    out = np.empty((nch, nf), np.float32)
    for k in range(nf):
        for c in range(nch):
            out[c, k] = L.orc_band_sum(orc.fptr(bins[k, c]), lo, hi)
    return out


def band_blocks(bins, bands):
    """[n_bands][nch][n_frames] for a sweep's bands() list"""
    return np.ascontiguousarray(np.stack([band_sums(bins, lo, hi) for lo, hi in bands]))


def long_script(kind, n_frames, nch, F, seed):
    """band sums [nch][n_frames] of a 10-minute synthetic stream: 'drift' (a level wandering over four decades, bursts, frames
    within a hair of ten times the level), 'ties' (constant and power-of-two stretches, channels equal), 'silence'"""
    rng = np.random.default_rng(seed)
    if kind == "silence":
        return np.zeros((nch, n_frames), np.float32)
    t = np.arange(n_frames) * F / LONG_RATE
    if kind == "drift":
        step = rng.normal(0, 0.02 * math.sqrt(F / 1024.0), n_frames)
        level = 10 ** (np.cumsum(step) % 4 - 4)
        x = level * rng.uniform(0.5, 1.5, n_frames)
        burst = np.zeros(n_frames, bool)
        for s in rng.uniform(0, t[-1], 150):
            burst |= (t >= s) & (t < s + rng.uniform(0.3, 6.0))
        x[burst] *= 30
        near = rng.random(n_frames) < 0.05
        x[near] = level[near] * 10 * (1 + rng.normal(0, 1e-7, near.sum()))
    else:
        x = np.empty(n_frames)
        k = 0
        while k < n_frames:   # stretches of 1 .. 200 s at one value: powers of two, constants, a few random-valued frames
            d = int(rng.uniform(1.0, 200.0) * LONG_RATE / F)
            kind_k = rng.integers(4)
            if kind_k == 0:
                x[k:k + d] = 2.0 ** -int(rng.integers(2, 12))
            elif kind_k == 1:
                x[k:k + d] = float(np.float32(rng.uniform(0.001, 0.1)))
            elif kind_k == 2:
                x[k:k + d] = 2.0 ** -int(rng.integers(0, 4))   # a loud stretch above the long-term level
            else:
                x[k:k + d] = rng.uniform(0.001, 0.01, min(d, n_frames - k))
            k += d
    out = np.empty((nch, n_frames), np.float32)
    for c in range(nch):
        out[c] = x if (c == 0 or kind == "ties") else x * (1.0 + 0.5 * c)
    return out


LONG_KINDS = ["drift", "ties", "silence", "drift"]


def long_rms(kind, n_chunks, nch, seed):
    rng = np.random.default_rng(seed + 99)
    if kind == "silence":
        return np.zeros((nch, n_chunks), np.float32)
    if kind == "ties":   # equal channels (ratio 1), then stretches with one channel at half
        r = np.full((nch, n_chunks), 0.25, np.float32)
        r[1:, (np.arange(n_chunks) // 37) % 2 == 1] = 0.125
        return r
    base = rng.uniform(0.01, 0.2, n_chunks)
    return np.stack([base * (1.0 if c == 0 else rng.uniform(0.2, 1.0, n_chunks)) for c in range(nch)]).astype(np.float32)


def long_inputs(pkg, nch, n_chunks, sizes=LONG_SIZES, kinds=LONG_KINDS, seed=0):
    """synthetic streams: {F: band [S][nch][n_frames(F)]}, rms [S][nch][n_chunks], {F: ratios [S][n_frames(F)]}"""
    rms = np.stack([long_rms(k, n_chunks, nch, seed + s) for s, k in enumerate(kinds)])
    band, ratio = {}, {}
    for F in sizes:
        nf = n_chunks * LONG_CHUNK // F
        band[F] = np.stack([long_script(k, nf, nch, F, seed + s) for s, k in enumerate(kinds)])
        ratio[F] = np.stack([pkg.simulator.frame_ratios(rms[s].T, nf, fft_size=F, chunk=LONG_CHUNK) for s in range(len(kinds))])
    return band, rms, ratio


# ------------------------------------------------------------------ the oracle machines

def oracle_vad_config(ov):
    cfg = orc.VadConfig()
    orc.lib().orc_vad_config_default(C.byref(cfg))
    for k, v in (ov or {}).items():
        setattr(cfg, k, v)
    return cfg


def oracle_machine(ov, rate, nch, F, band, ratio):
    """orc_vad over band [nch][n_frames] and ratio [n_frames] -> (segments, audit (rel, abs, n_frames))"""
    L = orc.lib()
    cfg = oracle_vad_config(ov)
    bf = np.ascontiguousarray(np.asarray(band, np.float32).T)
    r = np.ascontiguousarray(ratio, np.float32)
    v = L.orc_vad_create(C.byref(cfg), rate, nch, F)
    try:
        L.orc_vad_run_frames(v, 0, bf.shape[0], orc.fptr(bf), orc.fptr(r))
        ns = L.orc_vad_n_segments(v)
        p = L.orc_vad_segments(v)
        segs = [(p[i].sample_from, p[i].sample_to, p[i].avg_channel_vol_ratio, p[i].vad_met_sec) for i in range(ns)]
        nt = L.orc_vad_n_trace(v)
        tr = np.zeros(0, TRACE_DT)
        if nt:
            addr = C.cast(L.orc_vad_traces(v), C.c_void_p).value
            tr = np.frombuffer((C.c_char * (nt * TRACE_DT.itemsize)).from_address(addr), TRACE_DT).copy()
    finally:
        L.orc_vad_destroy(v)
    return segs, trace_audit(tr, float(cfg.channel_vol_ratio_threshold))


def trace_audit(tr, ratio_threshold):
    """vad_machine.h's margin audit from the oracle's trace: min |st - thr| / thr over frames with thr > 0, min |ratio -
    ratio_threshold| over all frames, the frame count"""
    thr, st = tr["threshold"], tr["short_term"]
    pos = thr > 0
    rel = float(np.min(np.abs(st[pos] - thr[pos]) / thr[pos])) if pos.any() else math.inf
    ab = float(np.min(np.abs(tr["channel_vol_ratio"] - ratio_threshold))) if len(tr) else math.inf
    return rel, ab, len(tr)


def oracle_machines(jobs):
    """[(ov, rate, nch, F, band, ratio)] -> [(segments, audit)] on up to 16 threads"""
    with ThreadPoolExecutor(POOL) as ex:
        return list(ex.map(lambda j: oracle_machine(*j), jobs))


# ------------------------------------------------------------------ comparisons and scoring

def seg_bits(segs):
    return [(int(a), int(b), np.float32(r).view(np.uint32).item(), np.float32(m).view(np.uint32).item()) for a, b, r, m in segs]


def audit_bits(a):
    return np.asarray(a[:2], np.float64).view(np.uint64).tolist() + [int(a[2])]


STAT_CFGS = [{"ignore_shorter_than_sec": 0.0, "extrude_start": 0.0, "extrude_end": 0.0, "fill_gaps": 0.0},
             {"ignore_shorter_than_sec": 0.7, "extrude_start": 5.0, "extrude_end": 10.0, "fill_gaps": 5.0},   # a label gap exactly
             {"ignore_shorter_than_sec": 0.0, "extrude_start": 0.0, "extrude_end": 0.0, "fill_gaps": 5.0},
             {"ignore_shorter_than_sec": 0.2, "extrude_start": 12.0, "extrude_end": 40.0, "fill_gaps": 30.0},  # past every gap
             {"ignore_shorter_than_sec": 1e6, "extrude_start": 1.0, "extrude_end": 1.0, "fill_gaps": 30.0}]   # past every segment


def gap_labels(segs, rate):
    """labels with a gap of exactly 5 s (fill_gaps) inside each long oracle segment: integer seconds, exact in f32"""
    out = []
    for a, b, _, _ in segs:
        s = math.ceil(a / rate)
        if s + 7 < b / rate:
            out += [(float(s), float(s + 1)), (float(s + 6), float(s + 7))]
    return out


def oracle_stats(segs, labels, rate, sc):
    """orc_stats_from_segments(orc_segment_to_sec(segments), labels, sc) as float32 [11]"""
    L = orc.lib()
    secs = []
    for a, b, r, m in segs:
        s = orc.SpeechSegment(a, b, r, m)
        secs.append(L.orc_segment_to_sec(C.byref(s), rate))
    v = (orc.SegSec * max(len(secs), 1))(*secs)
    ref = (orc.SegSec * max(len(labels), 1))(*[orc.SegSec(a, b) for a, b in labels])
    cfg = orc.StatConfig(sc["ignore_shorter_than_sec"], sc["extrude_start"], sc["extrude_end"], sc["fill_gaps"])
    st = L.orc_stats_from_segments(v, len(secs), ref, len(labels), C.byref(cfg))
    return np.array([getattr(st, n) for n, _ in orc.SingleStats._fields_], np.float32)


def oracle_aggregate(stats_rows):
    """orc_stats_aggregate over float32 [n][11] -> float32 [23] in AggregateStats' field order"""
    arr = (orc.SingleStats * max(len(stats_rows), 1))()
    for i, row in enumerate(stats_rows):
        for (n, _), v in zip(orc.SingleStats._fields_, row):
            setattr(arr[i], n, float(v))
    return agg_array(orc.lib().orc_stats_aggregate(arr, len(stats_rows)))


def agg_array(a):
    out = []
    for n, t in a._fields_:
        v = getattr(a, n)
        out += [getattr(v, m) for m, _ in t._fields_] if hasattr(t, "_fields_") else [v]
    return np.array(out, np.float32)


def assert_stats_bits(got, want, what):
    assert np.array_equal(np.asarray(got, np.float32).view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), (what, got, want)
