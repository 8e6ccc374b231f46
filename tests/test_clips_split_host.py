"""The host side of the split-source Recorder (no GPU): fvad_clips_split_check's rules in their order, the proof that the table of
clip_split_cases.py bites -- three wrong versions of the split model each fail it --, and fvad_vad_batch_hold_from against the
oracle's machines at every cut of a run in parts."""
import ctypes as C

import numpy as np
import pytest

import clip_cases as cc
import clip_split_cases as sc
import orc
import vad_oracle_cases as voc

INVALID, OUT_OF_RANGE, TOO_SMALL = -100, -6, -106


# ------------------------------------------------------------------ fvad_clips_split_check
A = (0x10000, 4, 1001, 1000)          # (address, lanes, stride, samples): nothing is read through the addresses
B = (0x90000, 6, 2001, 2000)
OUT = 0x400000


def test_check_accepts_and_plans_like_clips_plan(fv):
    rows = [(2, 1, 10, 90, 3, 0, 10), (1, 0, 0, 0, 5, 1999, 1), (4, 0, 995, 5, 2, 0, 2000), (1, 3, 0, 1000, 0, 0, 0)]
    for pcm16 in (False, True):
        st, offsets, total = fv.clips_split_check(A, B, False, rows, out_pcm16=pcm16, out=OUT)
        want, want_total = fv.clips_plan([(0, 1, 0, r[3] + r[6]) for r in rows], pcm16)
        assert st == 0 and np.array_equal(offsets, want) and total == want_total
    assert fv.clips_split_check(A, B, False, np.zeros((0, 7), np.uint64))[0] == 0          # no clips: nothing to do
    # a piece of no samples has no other rule: its lane and range may be anything, its buffer may be NULL or have no lanes
    assert fv.clips_split_check((None, 0, 0, 0), B, False, [(1, 99, 1 << 40, 0, 0, 0, 5)], out=OUT)[0] == 0
    assert fv.clips_split_check(A, (None, 0, 0, 0), False, [(1, 0, 0, 5, 99, 1 << 40, 0)], out=OUT)[0] == 0
    # exactly the plan's total is enough
    assert fv.clips_split_check(A, B, False, rows[:1], out=OUT, out_capacity=100)[0] == 0
    # one lane: the stride is not looked at
    assert fv.clips_split_check((0x10000, 1, 0, 1000), B, False, [(1, 0, 0, 5, 0, 0, 5)], out=OUT)[0] == 0


def test_check_refuses_in_the_stated_order(fv):
    ok = [(2, 1, 10, 90, 3, 0, 10), (1, 0, 0, 0, 5, 1999, 1)]
    M = 1 << 64
    # each call breaks the rule named and every later rule too (where it can): the earlier rule's status comes back
    late = dict(out_capacity=1)                                       # (capacity, broken as well)
    for what, status, kw in (
            ("NULL out", INVALID, dict(out=None, src_format=9)),
            ("bad source format", INVALID, dict(src_format=2, out=OUT + 4)),
            ("bad output format", INVALID, dict(out_format=-1, out=OUT + 4)),
            ("NULL A that a row reads", INVALID, dict(a=(None,) + A[1:], out=OUT + 4)),
            ("NULL B that a row reads", INVALID, dict(b=(None,) + B[1:], out=OUT + 4)),
            ("A not aligned to its samples", INVALID, dict(a=(A[0] + 2,) + A[1:], b=(B[0], 6, 5, 2000))),
            ("B not aligned to its samples", INVALID, dict(b=(B[0] + 1, 6, 5, 2000))),
            ("out not 16-byte aligned", INVALID, dict(out=OUT + 8, a=(A[0], 4, 999, 1000))),
            ("A's stride below its samples", INVALID, dict(a=(A[0], 4, 999, 1000), clips=[(0, 0, 0, 1, 0, 0, 1)])),
            ("B's stride below its samples", INVALID, dict(b=(B[0], 6, 1999, 2000), clips=[(0, 0, 0, 1, 0, 0, 1)])),
            ("both lengths 0", INVALID, dict(clips=[ok[0], (1, 0, 0, 0, 0, 0, 0), (1, 9, 0, 5, 0, 0, 0)], **late)),
            ("no channels", INVALID, dict(clips=[ok[0], (0, 0, 0, 5, 0, 0, 5), (1, 9, 0, 5, 0, 0, 0)], **late)),
            ("lengths that wrap", INVALID, dict(clips=[(1, 0, 0, M - 1, 0, 0, 2)], **late)),
            ("a total that wraps", INVALID, dict(clips=[(1, 0, 0, M - 8, 0, 0, 0), (1, 0, 0, 0, 0, 0, 100)], **late)),
            ("A's piece past its samples", OUT_OF_RANGE, dict(clips=[ok[0], (1, 0, 911, 90, 0, 0, 1)], **late)),
            ("A's from past its samples", OUT_OF_RANGE, dict(clips=[(1, 0, M - 1, 2, 0, 0, 1)], **late)),
            ("A's lanes past its lanes", OUT_OF_RANGE, dict(clips=[(2, 3, 0, 5, 0, 0, 1)], **late)),
            ("A's first lane past its lanes", OUT_OF_RANGE, dict(clips=[(1, 4, 0, 5, 0, 0, 1)], **late)),
            ("B's piece past its samples", OUT_OF_RANGE, dict(clips=[(1, 0, 0, 1, 0, 1999, 2)], **late)),
            ("B's lanes past its lanes", OUT_OF_RANGE, dict(clips=[(3, 0, 0, 1, 4, 0, 2)], **late)),
            ("capacity below the total", TOO_SMALL, dict(out_capacity=103, out=A[0])),
            ("out inside A", INVALID, dict(out=A[0] + 16)),
            ("out ends in B", INVALID, dict(out=B[0] - 16)),
            ("A's last sample under out's first", INVALID, dict(out=A[0] + (3 * 1001 + 1000) * 4 - 4 & ~15)),
            ("more than 2^31 - 1 units", INVALID, dict(a=(A[0], 4, 1 << 50, 1 << 50), out=1 << 60, clips=[(4, 0, 0, (1 << 31) * 2048, 0, 0, 0)]))):
        kw = dict(kw)
        st, _, _ = fv.clips_split_check(kw.pop("a", A), kw.pop("b", B), False, kw.pop("clips", ok), out=kw.pop("out", OUT), **kw)
        assert st == status, what
    # the same call with a host output: no alignment rule
    assert fv.clips_split_check(A, B, False, ok, out=OUT + 8, device_out=False)[0] == 0
    # the output may touch a source's ends
    assert fv.clips_split_check(A, B, False, ok, out=A[0] + (3 * 1001 + 1000) * 4 + 12 & ~15)[0] == 0
    assert fv.clips_split_check(A, B, False, ok, out=B[0] - 104 * 4)[0] == 0
    # exactly 2^31 - 1 units pass
    one = [(1, 0, 0, ((1 << 31) - 1) * 8192, 0, 0, 0)]
    assert fv.clips_split_check((A[0], 1, 0, 1 << 50), B, False, one, out=1 << 60)[0] == 0
    assert fv.clips_split_check((A[0], 1, 0, 1 << 50), B, False, [(1, 0, 0, ((1 << 31) - 1) * 8192 + 1, 0, 0, 0)], out=1 << 60)[0] == INVALID


# ------------------------------------------------------------------ the table and the model
@pytest.fixture(scope="module", params=[False, True], ids=["f32", "pcm16"])
def table(request):
    t = sc.SplitTable(request.param)
    return t, sc.model_export_contiguous(t.src, t.clips, False)


def test_the_split_table_is_what_the_issue_asks_for(table):
    t, _ = table
    lens = (t.clips[:, 3] - t.clips[:, 2]).astype(np.int64)
    for i, n in enumerate(lens):
        assert set(sc.seams(n)) == set(t.sigma[t.base == i].tolist())
    n = int(lens.max())
    assert set(sc.seams(n)) == {0, 1, 3, n // 2, n - 3, n - 1, n, sc.T - 1, sc.T, sc.T + 1, 2 * sc.T} and n > 2 * sc.T
    assert sc.seams(2) == [0, 1, 2] and sc.seams(1) == [0, 1]
    by = 2 if t.pcm16 else 4
    every = {(x, y) for x in range(0, 16, by) for y in range(0, 16, by)}
    assert t.offsets_mod16() == every                                # every pair of offsets within 16 bytes
    r = t.rows.astype(np.int64)
    assert t.A.shape[0] != t.B.shape[0] != cc.N_LANES and t.a_stride != t.b_stride and t.a_stride % 2 == t.b_stride % 2 == 1
    assert np.all((r[:, 1] != r[:, 4]) | (r[:, 3] == 0) | (r[:, 6] == 0))       # a stream's lanes differ between A and B
    # everything around the pieces is the sentinel / NaN: the pieces hold exactly the rows' samples
    used_a, used_b = np.zeros(t.A.shape, bool), np.zeros(t.B.shape, bool)
    for C_, la, fa, na, lb, fb, nb in r:
        assert not used_a[la:la + C_, max(fa - 1, 0):fa + na + 1].any() and not used_b[lb:lb + C_, max(fb - 1, 0):fb + nb + 1].any()
        used_a[la:la + C_, fa:fa + na] = True
        used_b[lb:lb + C_, fb:fb + nb] = True
    for buf, used in ((t.A, used_a), (t.B, used_b)):
        rest = buf[~used]
        assert np.all(rest == cc.SENTINEL) if t.pcm16 else np.all(np.isnan(rest))
    assert r[:, 2].max() + 1 <= t.a_samples and r[:, 5].max() + 1 <= t.b_samples


def test_the_split_model_gives_the_contiguous_bits(table):
    t, want = table
    got = sc.model_export_split(t, t.rows, False)
    sc.compare_split(got, sc.expected_rows(want, t.base, t.rows, False), "the split model")
    if not t.pcm16:                                                   # equal formats: the source's bits
        for i, s in zip(t.base, got["samples"]):
            l0, _, a, b = (int(v) for v in t.clips[i])
            assert s.tobytes() == t.src[l0 + want["best_channel"][i], a:b].tobytes()


@pytest.mark.parametrize("mutation", ["seam", "tiles", "swapped"])
def test_a_wrong_split_model_fails_the_table(table, mutation):
    t, want = table
    got, exp = sc.model_export_split(t, t.rows, False, mutation=mutation), sc.expected_rows(want, t.base, t.rows, False)
    if mutation == "tiles" and t.pcm16:
        # PCM16 squares are multiples of 2^-30 below 1 and a clip has far fewer than 2^23 of them: every partial sum is exact in
        # f64, so no order of adding can show.  It is the f32 table that tells the tile orders apart
        sc.compare_split(got, exp, mutation)
        return
    with pytest.raises(AssertionError):
        sc.compare_split(got, exp, mutation)


# ------------------------------------------------------------------ fvad_vad_batch_hold_from
RATE, F, CHUNK = 48000, 960, 24000           # 25 frames per chunk: every chunk edge is a cut
PER = CHUNK // F
N_CHUNKS = 400                               # 200 s
KINDS = ["drift", "ties", "silence", "drift"]
OV = {"speech_threshold_factor": 3.0, "long_term_speech_avg_sec": 20.0, "max_speech_gap_sec": 1.5}
START_BUFFER = 2 * RATE                      # VADMachine.zig:312-317
CLOSED = 0


def _oracle_trace(ov, nch, band, ratio):
    """orc_vad over band [nch][n_frames] -> (segments, state_after [n_frames])"""
    L = orc.lib()
    cfg = voc.oracle_vad_config(ov)
    bf = np.ascontiguousarray(np.asarray(band, np.float32).T)
    r = np.ascontiguousarray(ratio, np.float32)
    v = L.orc_vad_create(C.byref(cfg), RATE, nch, F)
    try:
        L.orc_vad_run_frames(v, 0, bf.shape[0], orc.fptr(bf), orc.fptr(r))
        p = L.orc_vad_segments(v)
        segs = [(p[i].sample_from, p[i].sample_to) for i in range(L.orc_vad_n_segments(v))]
        nt = L.orc_vad_n_trace(v)
        addr = C.cast(L.orc_vad_traces(v), C.c_void_p).value
        tr = np.frombuffer((C.c_char * (nt * voc.TRACE_DT.itemsize)).from_address(addr), voc.TRACE_DT).copy()
    finally:
        L.orc_vad_destroy(v)
    return segs, tr["state_after"]


@pytest.fixture(scope="module")
def parts(pkg, fv):
    """a two-channel batch of four streams run chunk by chunk: after every cut c (in chunks) the hold_from values and the number
    of segments reported so far; the final segments; and the oracle's machines over the same band sums"""
    nch, nf = 2, N_CHUNKS * PER
    band = np.stack([voc.long_script(k, nf, nch, F, 40 + s) for s, k in enumerate(KINDS)])       # [S][nch][nf]
    rms = np.stack([voc.long_rms(k, N_CHUNKS, nch, 40 + s) for s, k in enumerate(KINDS)])        # [S][nch][n_chunks]
    S = len(KINDS)
    vb = fv.VadBatch(S, n_channels=nch, fft_size=F, overrides=OV)
    try:
        fresh = vb.hold_from()
        b2, r2 = band.reshape(S * nch, nf), rms.reshape(S * nch, N_CHUNKS)
        holds, counts = [], []
        for c in range(N_CHUNKS):
            segs = vb.run_part(b2[:, c * PER:(c + 1) * PER], r2[:, c:c + 1], c * PER, chunk_size=CHUNK)
            holds.append(vb.hold_from())
            counts.append([len(s) for s in segs])
    finally:
        vb.close()
    oracle = []
    for s in range(S):
        ratio = pkg.simulator.frame_ratios(rms[s].T, nf, fft_size=F, chunk=CHUNK)
        oracle.append(_oracle_trace(OV, nch, band[s], ratio))
    return {"fresh": fresh, "holds": np.array(holds, np.int64), "counts": np.array(counts), "segs": segs, "oracle": oracle, "S": S}


def _closed_value(c):
    return c - min(START_BUFFER, c)


def _check_rule(p, hold_of):
    """the issue's three statements at every cut and stream, for hold_of(cut index k, stream) -> the value under test"""
    for s in range(p["S"]):
        segs, state = p["oracle"][s]
        for k in range(N_CHUNKS):
            c = (k + 1) * CHUNK                                       # the cut, in samples
            h = hold_of(k, s)
            later = segs[p["counts"][k][s]:]                          # reported only after the cut
            assert all(a >= h for a, _ in later), ("a later segment starts below hold_from", s, k)
            if state[(k + 1) * PER - 1] == CLOSED:
                assert h == _closed_value(c), ("a closed machine", s, k)
            for a, _ in later:
                if a < c - START_BUFFER:
                    assert a == h, ("a segment open across the cut", s, k)


def test_hold_from_at_every_cut(parts):
    p = parts
    assert p["fresh"] == [0] * p["S"]                                 # a batch that has run nothing
    for s in range(p["S"]):
        assert [x[:2] for x in p["segs"][s]] == p["oracle"][s][0]     # (the machines under test are the oracle's)
    _check_rule(p, lambda k, s: p["holds"][k][s])
    # the scenarios hold what the statements are about: segments, cuts with the machine closed and cuts with a segment open whose
    # start lies more than the pre-roll back
    n_open = sum(1 for s in range(p["S"]) for k in range(N_CHUNKS)
                 for a, _ in p["oracle"][s][0][p["counts"][k][s]:] if a < (k + 1) * CHUNK - START_BUFFER)
    n_closed = sum(int(p["oracle"][s][1][(k + 1) * PER - 1] == CLOSED) for s in range(p["S"]) for k in range(N_CHUNKS))
    assert sum(len(x) for x in p["segs"]) >= 6 and n_open >= 10 and n_closed >= 100
    assert all(h == _closed_value((k + 1) * CHUNK) for k, h in enumerate(p["holds"][:, KINDS.index("silence")]))


@pytest.mark.parametrize("rule", ["always c - start_buffer", "always 0"])
def test_a_wrong_hold_rule_fails(parts, rule):
    wrong = (lambda k, s: _closed_value((k + 1) * CHUNK)) if rule.startswith("always c") else (lambda k, s: 0)
    with pytest.raises(AssertionError):
        _check_rule(parts, wrong)


def test_hold_from_argument_rules(fv):
    vb = fv.VadSweep(2, [{}, OV], n_channels=1, fft_size=F)
    try:
        assert vb.hold_from(0) == [0, 0] and vb.hold_from(1) == [0, 0]
        out = (C.c_uint64 * 2)()
        assert fv.lib().fvad_vad_batch_hold_from(vb.h, 2, out) == INVALID                  # no such config
        assert fv.lib().fvad_vad_batch_hold_from(vb.h, 0, None) == INVALID
        assert fv.lib().fvad_vad_batch_hold_from(None, 0, out) == INVALID
        with pytest.raises(fv.FvadError) as e:
            vb.hold_from(5)
        assert e.value.status == INVALID and "device run" in str(e.value)
    finally:
        vb.close()
