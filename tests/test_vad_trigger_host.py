"""Shared triggers on the host (context option vad_trigger "shared"): the trigger keys of a sweep batch, and the finishing walk
of csrc/vad_finish.h (fvad_vad_finish_bits) over the oracle's own threshold_met bits against the oracle's segments, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import vad_chain_cases as K
import vad_oracle_cases as V
import vad_trigger_cases as T

BASE = {"long_term_speech_avg_sec": 5.0, "speech_threshold_factor": 4.0, "initial_long_term_avg": 0.02, **K.FAST}


def keys_of(fv, cfgs, sizes=None):
    sw = fv.VadSweep(1, cfgs) if sizes is None else fv.VadSweepSized(1, cfgs, sizes)
    try:
        return sw.trigger_keys()
    finally:
        sw.close()


# ------------------------------------------------------------------ keys
@pytest.mark.parametrize("field", sorted(T.TRIGGER_FIELDS))
def test_every_trigger_field_splits_a_key(fv, field):
    key_of, rep = keys_of(fv, [BASE, dict(BASE, **{field: T.TRIGGER_FIELDS[field]}), BASE])
    assert key_of == [0, 1, 0] and rep == [0, 1]


@pytest.mark.parametrize("field", T.FINISH_FIELDS)
def test_finishing_fields_do_not_split_a_key(fv, field):
    key_of, rep = keys_of(fv, [BASE, dict(BASE, **{field: 0.7})])
    assert key_of == [0, 0] and rep == [0]


def test_windows_that_truncate_to_the_same_slots_share_a_key(fv):
    a, b = 0.2, 0.205   # 9.375 and 9.6 frames at 1024 points: 9 slots both
    assert V.ring_len(K.RATE, 1024, a) == V.ring_len(K.RATE, 1024, b) == 9
    key_of, rep = keys_of(fv, [dict(BASE, short_term_speech_avg_sec=a), dict(BASE, short_term_speech_avg_sec=b)])
    assert key_of == [0, 0] and rep == [0]


def test_first_seen_order_counts_and_small_buffers(fv):
    t = T.trigger_configs(3)
    cfgs = [dict(t[2], **K.FAST), dict(t[0], **K.FAST), dict(t[2], max_speech_gap_sec=1.0), dict(t[1], **K.FAST), dict(t[0], min_vad_duration_sec=2.0)]
    sw = fv.VadSweep(2, cfgs)
    try:
        assert sw.trigger_keys() == ([0, 1, 0, 2, 1], [0, 1, 3])
        L, n = fv.lib(), fv.sz()
        assert L.fvad_vad_batch_trigger_keys(sw.h, None, 0, C.byref(n), None) == 0 and n.value == 3   # counts only
        key_of = (C.c_uint32 * 5)()
        assert L.fvad_vad_batch_trigger_keys(sw.h, key_of, 0, C.byref(n), None) == 0 and list(key_of) == [0, 1, 0, 2, 1]
        rep = (C.c_uint32 * 3)(7, 7, 7)
        assert L.fvad_vad_batch_trigger_keys(sw.h, None, 2, C.byref(n), rep) == fv.FVAD_ERR_BUFFER_TOO_SMALL
        assert n.value == 3 and list(rep) == [7, 7, 7]
        assert L.fvad_vad_batch_trigger_keys(sw.h, None, 3, C.byref(n), rep) == 0 and list(rep) == [0, 1, 3]
        assert L.fvad_vad_batch_trigger_keys(None, None, 3, C.byref(n), rep) != 0
    finally:
        sw.close()


def test_one_config_at_two_sizes_is_two_keys(fv):
    key_of, rep = keys_of(fv, [BASE, BASE, BASE], sizes=[512, 1024, 512])
    assert key_of == [0, 1, 0] and rep == [0, 1]


def test_retain_rederives_the_keys_and_the_representatives_span_the_batch(fv):
    t = T.trigger_configs(4)
    cfgs = T.grid([dict(x, speech_min_freq=f) for x, f in zip(t, [500.0, 500.0, 800.0, 800.0])], T.FINISH[:3])
    sw = fv.VadSweep(1, cfgs)
    try:
        key_of, rep = sw.trigger_keys()
        assert key_of == [0, 1, 2, 3] * 3 and rep == [0, 1, 2, 3]
        # the representatives alone give the batch's bands, sizes and averages keys in the batch's order
        sub = fv.VadSweep(1, [cfgs[c] for c in rep])
        assert sub.bands()[0] == sw.bands()[0] and sub.sizes == sw.sizes and sub.avg_keys()[:2] == sw.avg_keys()[:2]
        sub.close()
        keep = [1, 2, 4, 7, 9]   # drops key 0's first config (key 0 now follows 1 and 2) and all of key 3 but config 7
        sw.retain(None, keep)
        fresh = fv.VadSweep(1, [cfgs[c] for c in keep])
        assert sw.trigger_keys() == fresh.trigger_keys() == ([0, 1, 2, 3, 0], [0, 1, 2, 3])
        fresh.close()
    finally:
        sw.close()


def test_retain_between_host_parts_rederives_the_keys(fv, pkg):
    I = K.inputs(pkg, [12.0], seed=2)
    cfgs = T.grid(T.trigger_configs(2), T.FINISH[:2])
    sw = fv.VadSweep(1, cfgs)
    try:
        half = 6 * K.CHUNK // 1024
        sw.run_sized(np.ascontiguousarray(I["band"][None, :, :half]), np.ascontiguousarray(I["rms"][:, :6]), half)
        sw.retain(None, [1, 2, 3])
        assert sw.trigger_keys() == ([0, 1, 0], [0, 1])
    finally:
        sw.close()


# ------------------------------------------------------------------ the walk against the oracle
SECONDS = 40.0


@pytest.fixture(scope="module")
def stream(pkg):
    """one 40 s stream (1875 frames: 30 words, the last partial), one trigger: the oracle's bits and frame ratios"""
    I = K.inputs(pkg, [SECONDS], seed=31)
    trig = dict(BASE)
    _, tr = T.oracle_trace(trig, K.RATE, 1, 1024, I["band"][:1, :I["n_frames"][0]], I["ratio"][0])
    met = tr["threshold_met"] != 0
    words = T.pack(met)
    assert len(words) == 30 and I["n_frames"][0] % 64 != 0
    assert met.any() and not met.all() and (words == 0).any()
    return I, trig, met, words


def oracle_segs(I, cfg):
    return V.seg_bits(V.oracle_machine(cfg, K.RATE, 1, 1024, I["band"][:1, :I["n_frames"][0]], I["ratio"][0])[0])


def walk(fv, cfg, words, ratio, n, **kw):
    segs, st = fv.finish_bits(cfg, words, ratio, n, **kw)
    return T.seg_tuples(segs), st


FRAME = 1024 / 48000
FINISHING = ([dict(min_consecutive_sec_to_open=o, max_speech_gap_sec=0.25, min_vad_duration_sec=0.0) for o in (0.0, FRAME, 0.3, 5.0)] +
             [dict(min_consecutive_sec_to_open=0.0, max_speech_gap_sec=g, min_vad_duration_sec=0.0) for g in (0.0, 0.1, 0.25, 1.0, 3.5)] +
             [dict(min_consecutive_sec_to_open=0.0, max_speech_gap_sec=0.25, min_vad_duration_sec=d) for d in (0.0, 0.5, 100.0)])


@pytest.mark.parametrize("fin", FINISHING, ids=lambda f: "-".join(f"{v:g}" for v in f.values()))
def test_the_walk_gives_the_oracles_segments(fv, stream, fin):
    I, trig, met, words = stream
    cfg = dict(trig, **fin)
    want = oracle_segs(I, cfg)
    got, st = walk(fv, cfg, words, I["ratio"][0], I["n_frames"][0])
    assert got == want and int(st[5]) == len(want)
    if fin["min_vad_duration_sec"] == 100.0 or fin["min_consecutive_sec_to_open"] == 5.0:
        assert want == []   # all aborted / never open
    elif fin == FINISHING[0]:
        assert len(want) >= 2 and want[0][0] == 0   # the first burst starts before sample 96000: the start clamps to 0


def test_closing_frames_on_the_first_and_last_bit_of_a_word(fv, stream):
    """over gaps of 0 .. 39 frames the walk agrees with the oracle, and for some gap a segment's closing frame is bit 0 and for
    some bit 63 of a word (bit 64 of a word is bit 0 of the next)"""
    I, trig, met, words = stream
    found = set()
    for frames in range(0, 40):
        cfg = dict(trig, min_consecutive_sec_to_open=0.0, min_vad_duration_sec=0.0, max_speech_gap_sec=(frames * 1024 + 1) / 48000)
        want = oracle_segs(I, cfg)
        got, _ = walk(fv, cfg, words, I["ratio"][0], I["n_frames"][0])
        assert got == want, frames
        gap = int(np.float32(48000) * np.float32(cfg["max_speech_gap_sec"]))
        for s in want:
            end = s[1] - 96000   # speech_end
            close = end + -(-gap // 1024) * 1024 if gap else end + 1024
            found.add((close // 1024) % 64)
        if {0, 63} <= found:
            break
    assert {0, 63} <= found, sorted(found)


TEN = 10.5 * FRAME   # ten whole frames and a half: an opening time or a gap of ten frames, whatever the rounding
PATTERN_CASES = {   # finishing fields, frames of the pattern walked, state after the last frame
    "ends open": (dict(min_consecutive_sec_to_open=TEN, max_speech_gap_sec=TEN, min_vad_duration_sec=0.0), T.PATTERN_FRAMES, T.OPEN),
    "ends opening": (dict(min_consecutive_sec_to_open=30.5 * FRAME, max_speech_gap_sec=TEN, min_vad_duration_sec=0.0), T.PATTERN_FRAMES, T.OPENING),
    "ends closing": (dict(min_consecutive_sec_to_open=TEN, max_speech_gap_sec=TEN, min_vad_duration_sec=0.0), 340, T.CLOSING),
}


@pytest.mark.parametrize("name", PATTERN_CASES)
def test_a_hand_made_pattern_at_the_word_edges(fv, name):
    """vad_trigger_cases.pattern(): the oracle's trace shows that the bits are the pattern and that the machine is OPENING on both
    sides of the edge of words 0 and 1, CLOSING on both sides of the edge of words 1 and 2, OPEN through two all-ones words, and ends
    the stream open, opening or closing (that segment is dropped); the walk gives the oracle's segments"""
    fin, n, last = PATTERN_CASES[name]
    met, band, ratio = T.pattern()
    cfg = dict(T.PATTERN_TRIGGER, **fin)
    want, tr = T.oracle_trace(cfg, K.RATE, 1, 1024, band[:, :n], ratio[:n])
    state = tr["state_after"]
    assert len(tr) == n and ((tr["threshold_met"] != 0) == met[:n]).all()   # the oracle's bits are the pattern
    words = T.pack(tr["threshold_met"] != 0)
    assert words[3] == words[4] == np.uint64(0xFFFFFFFFFFFFFFFF) and (state[256:320] == T.OPEN).all()   # an all-ones word while OPEN
    if n > 448:
        assert words[6] == 0 and (state[384:448] == T.CLOSED).all()   # and an all-zero word while CLOSED
    assert state[-1] == last and state[n - 2] == last
    if name != "ends opening":
        assert state[63] == state[64] == T.OPENING and state[127] == state[128] == T.CLOSING   # across the word edges
        assert (state[192:256] == T.OPEN).all()   # (both all-ones words)
    assert len(want) == (1 if last == T.CLOSING else 2) and want[0][0] == 0   # the last is dropped; the first one's start clamps to 0
    got, st = walk(fv, cfg, words, ratio[:n], n)
    assert got == V.seg_bits(want) and int(st[5]) == len(want)
    # the same in two parts cut inside the all-ones words: the second part's words are part-relative
    a, st = walk(fv, cfg, T.pack(met[:250]), ratio[:250], 250)
    b, st2 = walk(fv, cfg, T.pack(met[250:n]), ratio[250:n], n - 250, first_sample=250 * 1024, state=st)
    assert a + b == got


@pytest.mark.parametrize("F", [1024, 960, 512])
def test_parts_at_every_chunk_boundary_equal_the_single_walk(fv, pkg, F):
    I = K.inputs(pkg, [6.0], F=F, seed=F)   # 12 chunks
    n = I["n_frames"][0]
    cfg = dict(BASE, max_speech_gap_sec=0.3, min_consecutive_sec_to_open=0.05)
    _, tr = T.oracle_trace(cfg, K.RATE, 1, F, I["band"][:1, :n], I["ratio"][0])
    met = tr["threshold_met"] != 0
    assert met.any()
    want, st_all = walk(fv, cfg, T.pack(met), I["ratio"][0], n, fft_size=F)
    assert want == V.seg_bits(V.oracle_machine(cfg, K.RATE, 1, F, I["band"][:1, :n], I["ratio"][0])[0])
    for cut in range(1, 12):
        f = cut * K.CHUNK // F
        a, st = walk(fv, cfg, T.pack(met[:f]), I["ratio"][0][:f], f, fft_size=F)
        b, st = walk(fv, cfg, T.pack(met[f:]), I["ratio"][0][f:], n - f, first_sample=f * F, state=st, fft_size=F)
        assert a + b == want and st.tolist() == st_all.tolist(), (F, cut)


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_frame_counts_around_a_word_and_garbage_past_the_end(fv, stream, n):
    I, trig, met, words = stream
    cfg = dict(trig, max_speech_gap_sec=0.0)
    want, st_want = walk(fv, cfg, T.pack(met[:n]), I["ratio"][0][:n], n)
    dirty = T.pack(met[:n]).copy()
    if n % 64:
        dirty[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)   # bits past n_frames are not the part's
    dirty = np.concatenate([dirty, np.full(2, 0xFFFFFFFFFFFFFFFF, np.uint64)])
    got, st = walk(fv, cfg, dirty, I["ratio"][0][:n], n)
    assert got == want and st.tolist() == st_want.tolist()
    ref = V.oracle_machine(cfg, K.RATE, 1, 1024, I["band"][:1, :n], I["ratio"][0][:n])[0]
    assert want == V.seg_bits(ref)
