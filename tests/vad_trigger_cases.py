"""Tables of the shared-trigger tests (context option vad_trigger "shared"): trigger configs, the finishing fields that do not
reach the trigger, and the oracle's machines with their per-frame trace (threshold_met: the bits a trigger machine must emit)."""
import ctypes as C
import itertools

import numpy as np

import orc
import vad_chain_cases as K
import vad_oracle_cases as V

RATE, CHUNK = K.RATE, K.CHUNK
FINISH_FIELDS = ("min_consecutive_sec_to_open", "max_speech_gap_sec", "min_vad_duration_sec")
# 4 x 2 x 2 = 16 (open, gap, duration) combinations: open at once, after one frame (1024 / 48000 s) and later; close at once or
# after a gap; every duration or only segments of half a second
FINISH = [dict(zip(FINISH_FIELDS, v)) for v in itertools.product([0.0, 0.02, 0.1, 0.3], [0.0, 0.25], [0.0, 0.5])]
# each of these fields alone splits a trigger key (the base value, another value)
TRIGGER_FIELDS = {"speech_min_freq": 800.0, "long_term_speech_avg_sec": 7.0, "short_term_speech_avg_sec": 0.5,
                  "channel_vol_ratio_avg_sec": 1.0, "has_initial_long_term_avg": 0, "initial_long_term_avg": 0.03,
                  "speech_threshold_factor": 3.5, "channel_vol_ratio_threshold": 0.4}


def trigger_configs(n):
    """n configs with n distinct triggers: windows of 2, 6, 15 and 20 s, with and without an initial average, factors apart"""
    return [{"long_term_speech_avg_sec": [2.0, 6.0, 15.0, 20.0][i % 4], "speech_threshold_factor": 4.0 + 0.5 * (i // 8),
             "has_initial_long_term_avg": (i // 4) % 2, "initial_long_term_avg": 0.02} for i in range(n)]


def grid(triggers, finish=FINISH):
    """finish-major: the configs of one trigger are len(triggers) apart, so a wavefront by caller order mixes the keys"""
    return [dict(t, **f) for f in finish for t in triggers]


def oracle_trace(ov, rate, nch, F, band, ratio):
    """orc_vad over band [nch][n_frames] and ratio [n_frames] -> (segments, trace)"""
    L = orc.lib()
    cfg = V.oracle_vad_config(ov)
    bf = np.ascontiguousarray(np.asarray(band, np.float32).T)
    r = np.ascontiguousarray(ratio, np.float32)
    v = L.orc_vad_create(C.byref(cfg), rate, nch, F)
    try:
        L.orc_vad_run_frames(v, 0, bf.shape[0], orc.fptr(bf), orc.fptr(r))
        p = L.orc_vad_segments(v)
        segs = [(p[i].sample_from, p[i].sample_to, p[i].avg_channel_vol_ratio, p[i].vad_met_sec) for i in range(L.orc_vad_n_segments(v))]
        nt = L.orc_vad_n_trace(v)
        tr = np.zeros(0, V.TRACE_DT)
        if nt:
            addr = C.cast(L.orc_vad_traces(v), C.c_void_p).value
            tr = np.frombuffer((C.c_char * (nt * V.TRACE_DT.itemsize)).from_address(addr), V.TRACE_DT).copy()
    finally:
        L.orc_vad_destroy(v)
    return segs, tr


def pack(met):
    """threshold_met [n_frames] -> uint64 words: bit k % 64 of word k / 64 is frame k, the last word's upper bits zero"""
    met = np.asarray(met, bool)
    pad = np.zeros((len(met) + 63) // 64 * 64, np.uint8)
    pad[:len(met)] = met
    return np.packbits(pad.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u8").astype(np.uint64)


def seg_tuples(segs):
    return V.seg_bits([(s.sample_from, s.sample_to, s.avg_channel_vol_ratio, s.vad_met_sec) for s in segs])


# A hand-made threshold_met pattern (frames at 1024 points) for the finishing walk's word-edge cases: a burst from frame 60 (before
# sample 96000, and an opening time of ten frames lasts over the edge of words 0 and 1), a second burst that ends with frame 125 (a
# gap of ten frames lasts over the edge of words 1 and 2), a burst over frames 180 .. 329 (words 3 and 4 are all ones), and a burst
# over the last 20 frames (the stream ends open; ends opening for a longer opening time; cut at 340 frames it ends closing)
PATTERN_FRAMES = 700
PATTERN_BURSTS = [(60, 101), (110, 126), (180, 330), (680, 700)]
# a trigger whose threshold_met is the band itself: a short-term ring of one slot, a long-term average that stays between the two
# band values (0.001 and 1.0: from 0.02 x 4 down to 0.001 x 4)
PATTERN_TRIGGER = {"long_term_speech_avg_sec": 5.0, "speech_threshold_factor": 4.0, "initial_long_term_avg": 0.02,
                   "short_term_speech_avg_sec": V.sec_for_ring(RATE, 1024, 1)[0]}
CLOSED, OPENING, OPEN, CLOSING = range(4)   # VadTrace.state_after


def pattern():
    """-> (met [PATTERN_FRAMES] bool, band [1][PATTERN_FRAMES], ratio [PATTERN_FRAMES]: a ratio of its own per frame)"""
    met = np.zeros(PATTERN_FRAMES, bool)
    for a, b in PATTERN_BURSTS:
        met[a:b] = True
    band = np.where(met, np.float32(1.0), np.float32(0.001)).astype(np.float32)[None]
    ratio = np.random.default_rng(5).uniform(0.6, 1.0, PATTERN_FRAMES).astype(np.float32)
    return met, band, ratio
