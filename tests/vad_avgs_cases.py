"""Inputs of test_vad_avgs_host.py and test_vad_avgs_gpu.py: the short-term and channel-ratio averages of the device VAD machines
from tables (context option vad_avgs "table", csrc/kernels_vadavgs.hip and the table form of csrc/kernels_vad.hip).

Band sums and chunk RMS are fed to the machines directly, as vad_chain_cases.py does (its mono script() streams and config
sets serve the machine tests); the streams here add channels, for the min_volume rows.  The reference of an average is the
oracle's rolling average (orc_ra_push, oracle/orc_vad.c) pushed frame by frame."""
import ctypes as C

import numpy as np

import orc
import vad_chain_cases as K
import vad_oracle_cases as V

RATE, CHUNK = K.RATE, K.CHUNK
TILE = 256   # kernels.h: kAvgsTile, the frames of one workgroup of vad_minvol_kernel and vad_avgs_kernel

# ring lengths of the shared chain on the host, and of the table kernel: around a wavefront (63 .. 65), a frame tile (255 .. 257),
# the defaults (9, 23) and a 3 s short window at 512 points (282)
HOST_LENS = [1, 2, 3, 9, 23, 63, 64, 65, 282]
TABLE_LENS = [1, 2, 3, 9, 23, 63, 64, 65, 255, 256, 257, 282]

FAST = K.FAST


def oracle_avgs(x, length):
    """orc_ra_push of every x[k] into a ring of `length` slots without initial value -> float64 [len(x)]"""
    L = orc.lib()
    ra = L.orc_ra_create(int(length), 0, 0.0)
    try:
        return np.array([L.orc_ra_push(ra, float(v)) for v in np.asarray(x, np.float32)], np.float64)
    finally:
        L.orc_ra_destroy(ra)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def min_volume(band):
    """VADMachine.zig:153-158 over band [nch][n_frames]: from 999, the channels in order, replaced when strictly smaller"""
    mn = np.full(band.shape[1], 999, np.float32)
    for row in np.asarray(band, np.float32):
        mn = np.where(row < mn, row, mn)
    return mn


def inputs(seconds, F, nch, seed, ties=False):
    """streams of `seconds` [s] with nch channels -> dict(band [S * nch][max frames], rms [S * nch][max chunks], ratio [per
    stream] (the oracle's frame ratios), n_frames, n_chunks, F, nch).  The channels of vad_oracle_cases' drift stream differ by
    a factor; ties: its 'ties' stream instead, whose channels are equal (the minimum must keep the first)"""
    kind = "ties" if ties else "drift"
    n_chunks = [int(s * RATE) // CHUNK for s in seconds]
    n_frames = [k * CHUNK // F for k in n_chunks]
    band = np.zeros((len(seconds) * nch, max(n_frames)), np.float32)
    rms = np.zeros((len(seconds) * nch, max(n_chunks)), np.float32)
    ratio = []
    for s, (nf, nc) in enumerate(zip(n_frames, n_chunks)):
        b = V.long_script(kind, nf, nch, F, seed + s)
        if nch > 1 and not ties:   # the smallest channel changes from frame to frame
            b = b[(np.arange(nch)[:, None] + np.arange(nf)[None, :] // 7) % nch, np.arange(nf)[None, :]]
        band[s * nch:(s + 1) * nch, :nf] = b
        rms[s * nch:(s + 1) * nch, :nc] = V.long_rms(kind, nc, nch, seed + s)
        ratio.append(V.oracle_frame_ratios(rms[s * nch:(s + 1) * nch, :nc].T, nf, F, CHUNK))
    return {"band": band, "rms": rms, "ratio": ratio, "n_frames": n_frames, "n_chunks": n_chunks, "F": F, "nch": nch}


def len_configs(F, lens, below=False):
    """one config per ring length n of `lens`: short and ratio windows of exactly n slots (vad_oracle_cases.sec_for_ring's `on`),
    and with `below` a second one f32 ulp below (n - 1 slots; not for n = 1, whose ratio ring would be empty)"""
    out = []
    for n in lens:
        on, under = V.sec_for_ring(RATE, F, n)
        out.append({"short_term_speech_avg_sec": on, "channel_vol_ratio_avg_sec": on, **FAST})
        if below and n > 2:
            out.append({"short_term_speech_avg_sec": under, "channel_vol_ratio_avg_sec": under, **FAST})
    return out


def shared_grid():
    """128 configs over 4 short windows x 2 bands x 2 ratio windows x 8 factors on script()'s near-threshold frames: 8 short keys,
    2 ratio keys"""
    out = []
    for st in (0.1, 0.2, 0.5, 1.0):
        for lo in (300.0, 600.0):
            for cr in (0.3, 0.5):
                for f in (3.0, 3.5, 4.0, 4.5, 5.0, 6.0, 7.0, 8.0):
                    out.append({"short_term_speech_avg_sec": st, "speech_min_freq": lo, "channel_vol_ratio_avg_sec": cr,
                                "speech_threshold_factor": f, "long_term_speech_avg_sec": 5.0, "has_initial_long_term_avg": 0, **FAST})
    return out


def unique_grid(n):
    """n configs, every one with a short window and a ratio window of its own (n short keys, n ratio keys)"""
    return [{"short_term_speech_avg_sec": 0.05 * (i + 1), "channel_vol_ratio_avg_sec": 0.03 * (i + 1), "speech_threshold_factor": 4.0,
             "long_term_speech_avg_sec": [2.0, 6.0][i % 2], "has_initial_long_term_avg": i % 2, "initial_long_term_avg": 0.02, **FAST}
            for i in range(n)]


def upload(ctx, arr):
    d = ctx.device_alloc(arr.nbytes)
    ctx.to_device(d, arr)
    return d
