"""Inputs of test_vad_chain_gpu.py: band sums and chunk RMS fed to the VAD machines directly (mono, 48 kHz), and the config sets
that make the cooperative form of the machines' kernel (context option vad_chain "coop", kernels_vad.hip) take every path.

The cooperative form differs from the lane form only where a machine runs its exact long-term chain, so every stream here has
frames near the threshold (the lazy bound cannot settle them: decide() asks for the chain) on top of bursts that open and close
segments, and every config set says how many exact evaluations its machines must reach (checked from lazy_stats)."""
import numpy as np

import vad_oracle_cases as V

RATE, CHUNK = 48000, 24000
TILE = 1024   # kernels_vad.hip: kCoopTile, the slots of one LDS tile of the cooperative chain

# long-term ring lengths around every boundary of the cooperative chain: the float4 tail (1 .. 5), one row of 64 lanes' slots
# (63 .. 65), one cooperative load of 64 rows (255 .. 257), one tile (TILE - 1 .. TILE + 1)
RINGS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1]

FAST = {"min_consecutive_sec_to_open": 0.0, "min_vad_duration_sec": 0.0, "max_speech_gap_sec": 0.25}


def script(n_frames, F, seed, factor=4.0):
    """band sums [n_frames]: a noise floor, bursts of 0.6 .. 1.5 s every 2 .. 4 s at 30 times the floor, and one frame in 12 within
    1e-7 of `factor` times the floor (a config with that speech_threshold_factor has to run the exact chain there)"""
    rng = np.random.default_rng(seed)
    fps = RATE / F
    floor = 0.01
    x = floor * rng.uniform(0.9, 1.1, n_frames)
    t = 0.5
    while t * fps < n_frames:
        d = rng.uniform(0.6, 1.5)
        x[int(t * fps):int((t + d) * fps)] *= 30.0
        t += d + rng.uniform(2.0, 4.0)
    near = rng.random(n_frames) < 1.0 / 12
    x[near] = floor * factor * (1 + rng.normal(0, 1e-7, int(near.sum())))
    return x.astype(np.float32)


def inputs(pkg, seconds, F=1024, seed=0, stress=False):
    """streams of `seconds` [s] each -> dict(band [S][max frames] (zero past a stream's end), rms [S][max chunks], ratio [per
    stream], n_frames, n_chunks).  stress: vad_oracle_cases' drift stream instead of script()"""
    n_chunks = [int(s * RATE) // CHUNK for s in seconds]
    n_frames = [k * CHUNK // F for k in n_chunks]
    band = np.zeros((len(seconds), max(n_frames)), np.float32)
    rms = np.zeros((len(seconds), max(n_chunks)), np.float32)
    ratio = []
    for s, (nf, nc) in enumerate(zip(n_frames, n_chunks)):
        band[s, :nf] = V.long_script("drift", nf, 1, F, seed + s)[0] if stress else script(nf, F, seed + s)
        rms[s, :nc] = V.long_rms("drift", nc, 1, seed + s)[0]
        ratio.append(pkg.simulator.frame_ratios(np.ascontiguousarray(rms[s:s + 1, :nc].T), nf, fft_size=F, chunk=CHUNK))
    return {"band": band, "rms": rms, "ratio": ratio, "n_frames": n_frames, "n_chunks": n_chunks, "F": F}


def ring_configs(F, rings=RINGS):
    """every ring of `rings` exactly on and one f32 ulp below (vad_oracle_cases.sec_for_ring: n and n - 1 slots), with and without
    an initial long-term average, the factor script() puts frames next to"""
    out = []
    for k, n in enumerate(rings):
        for which, x in enumerate(V.sec_for_ring(RATE, F, n)):
            c = {"long_term_speech_avg_sec": x, "speech_threshold_factor": 4.0, **FAST}
            if (k + which) % 2:
                c["has_initial_long_term_avg"] = 0
            out.append(c)
    return out


def factor_configs(n, seed, long_sec=5.0):
    """n configs that differ only in speech_threshold_factor (the first one on script()'s near-threshold frames)"""
    rng = np.random.default_rng(seed)
    return [{"long_term_speech_avg_sec": long_sec, "speech_threshold_factor": 4.0 if i % 3 == 0 else float(rng.uniform(2.0, 8.0)),
             "has_initial_long_term_avg": 0, **FAST} for i in range(n)]


def window_configs(n):
    """n configs over four long-term windows (2, 6, 15 and 20 s: 93 .. 937 slots at 1024 points), so that the lanes of a wavefront
    by stream have different ring lengths"""
    return [{"long_term_speech_avg_sec": [2.0, 6.0, 15.0, 20.0][i % 4], "speech_threshold_factor": 4.0,
             "has_initial_long_term_avg": (i // 4) % 2, "initial_long_term_avg": 0.02, **FAST} for i in range(n)]


def oracle(I, cfgs, sizes=None):
    """[stream][config] -> (segments, audit) of the oracle's machines on inputs(): I, or {F: I} with sizes per config"""
    jobs = []
    S = len((I if sizes is None else I[sizes[0]])["n_frames"])
    for s in range(S):
        for c, cfg in enumerate(cfgs):
            J = I if sizes is None else I[sizes[c]]
            nf = J["n_frames"][s]
            jobs.append((cfg, RATE, 1, J["F"], J["band"][s:s + 1, :nf], J["ratio"][s]))
    res = iter(V.oracle_machines(jobs))
    return [[next(res) for _ in cfgs] for _ in range(S)]
