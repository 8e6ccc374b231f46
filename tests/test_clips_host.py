"""The host side of the batch Recorder (fvad_clips_plan, fvad_clips_from_segments; no GPU), and the proof that the case table
of clip_cases.py bites: three wrong versions of the numpy model each fail it."""
import numpy as np
import pytest

import clip_cases as cc

INVALID, TOO_SMALL = -100, -106


def test_plan_offsets_are_aligned_and_totals_add_up(fv):
    clips, _ = cc.case_table()
    for pcm16 in (False, True):
        offsets, total = fv.clips_plan(clips, pcm16)
        want, want_total = cc.plan(clips, pcm16)
        assert np.array_equal(offsets, want) and total == want_total
        assert np.all(offsets * (2 if pcm16 else 4) % 16 == 0)                     # every slot starts on a 16-byte boundary
        lens = (clips[:, 3] - clips[:, 2]).astype(np.int64)
        assert np.all(np.diff(offsets.astype(np.int64)) >= lens[:-1]) and total >= int(offsets[-1]) + int(lens[-1])
        assert total - lens.sum() < len(clips) * (8 if pcm16 else 4)               # the padding is below one 16-byte step per clip
    # a clip whose length is a multiple of 16 bytes is followed at once; one sample more costs a whole step
    assert list(fv.clips_plan([(0, 1, 0, 8), (0, 1, 0, 9), (0, 1, 5, 6)], False)[0]) == [0, 8, 20] and fv.clips_plan([(0, 1, 0, 8)], False)[1] == 8
    assert list(fv.clips_plan([(0, 1, 0, 8), (0, 1, 0, 9), (0, 1, 5, 6)], True)[0]) == [0, 8, 24]


def test_plan_allows_overlapping_and_duplicate_clips(fv):
    clips = [(3, 2, 100, 200), (3, 2, 150, 260), (3, 2, 100, 200), (0, 1, 100, 200)]
    offsets, total = fv.clips_plan(clips, False)
    assert list(offsets) == [0, 100, 212, 312] and total == 412


def test_plan_argument_rules(fv):
    assert fv.clips_plan(np.zeros((0, 4), np.uint64))[1] == 0                      # no clips: nothing to pack
    for bad in ([(0, 1, 10, 10)], [(0, 1, 11, 10)], [(0, 0, 0, 10)], [(0, 1, 0, 5), (0, 1, 7, 7)]):
        with pytest.raises(fv.FvadError) as e:
            fv.clips_plan(bad)
        assert e.value.status == INVALID
    one = np.array([[0, 1, 0, 5]], np.uint64)
    offs, total = np.zeros(1, np.uint64), fv.C.c_uint64(0)
    u64p = fv.C.POINTER(fv.C.c_uint64)
    L = fv.lib()
    assert L.fvad_clips_plan(one.ctypes.data_as(u64p), 1, 7, offs.ctypes.data_as(u64p), fv.C.byref(total)) == INVALID   # no such format
    assert L.fvad_clips_plan(one.ctypes.data_as(u64p), 1, 0, offs.ctypes.data_as(u64p), None) == INVALID
    assert L.fvad_clips_plan(None, 1, 0, offs.ctypes.data_as(u64p), fv.C.byref(total)) == INVALID
    assert L.fvad_clips_plan(one.ctypes.data_as(u64p), 1, 0, None, fv.C.byref(total)) == INVALID
    assert L.fvad_clips_plan(None, 0, 1, None, fv.C.byref(total)) == 0 and total.value == 0


def test_plan_refuses_a_total_that_does_not_fit_64_bits(fv):
    """a running total within 16 bytes of 2^64 is refused at the next clip, whatever its length; it must not wrap to a small total"""
    M = 1 << 64
    for pcm16, per16 in ((False, 4), (True, 8)):
        near = (0, 1, 0, M - per16 - 2)            # its slot ends at M - per16: the largest total that is accepted
        offsets, total = fv.clips_plan([near], pcm16)
        assert total == M - per16 and list(offsets) == [0]
        for more in ((0, 1, 0, 1), (0, 1, 0, per16), (0, 1, 0, 100)):
            with pytest.raises(fv.FvadError) as e:
                fv.clips_plan([near, more], pcm16)
            assert e.value.status == INVALID
        with pytest.raises(fv.FvadError) as e:      # one clip alone whose slot would pass 2^64
            fv.clips_plan([(0, 1, 0, M - per16)], pcm16)
        assert e.value.status == INVALID


def test_from_segments_keeps_what_the_data_reaches(fv):
    segs = [(100, 5000, 0.0, 0.0), (7000, 24000, 0.0, 0.0), (30000, 48001, 0.0, 0.0)]
    # sample_to exactly at n_available is kept, one past it is not: the reference never finalises such a recording
    clips, skipped = fv.clips_from_segments(segs, 4, 2, 48001)
    assert clips.tolist() == [[4, 2, 100, 5000], [4, 2, 7000, 24000], [4, 2, 30000, 48001]] and skipped == 0
    clips, skipped = fv.clips_from_segments(segs, 4, 2, 48000)
    assert clips.tolist() == [[4, 2, 100, 5000], [4, 2, 7000, 24000]] and skipped == 1
    clips, skipped = fv.clips_from_segments(segs, 0, 1, 24000)
    assert clips.tolist() == [[0, 1, 100, 5000], [0, 1, 7000, 24000]] and skipped == 1
    clips, skipped = fv.clips_from_segments(segs, 0, 1, 0)
    assert clips.shape == (0, 4) and skipped == 3
    clips, skipped = fv.clips_from_segments([], 0, 1, 48000)                       # empty lists
    assert clips.shape == (0, 4) and skipped == 0


def test_from_segments_argument_rules(fv):
    segs = [(100, 5000, 0.0, 0.0), (7000, 24000, 0.0, 0.0), (30000, 48000, 0.0, 0.0)]
    with pytest.raises(fv.FvadError) as e:                                         # cap too small
        fv.clips_from_segments(segs, 0, 1, 48000, cap=2)
    assert e.value.status == TOO_SMALL
    arr = (fv.SpeechSegment * 3)()
    for i, s in enumerate(segs):
        arr[i].sample_from, arr[i].sample_to = s[0], s[1]
    rows = np.full((2, 4), 77, np.uint64)
    n, skipped = fv.sz(), fv.sz()
    L, u64p = fv.lib(), fv.C.POINTER(fv.C.c_uint64)
    assert L.fvad_clips_from_segments(arr, 3, 0, 1, 30000, rows.ctypes.data_as(u64p), 2, fv.C.byref(n), fv.C.byref(skipped)) == 0
    assert (n.value, skipped.value) == (2, 1)                                      # the skipped one needs no room
    assert L.fvad_clips_from_segments(arr, 3, 0, 1, 48000, rows.ctypes.data_as(u64p), 2, fv.C.byref(n), fv.C.byref(skipped)) == TOO_SMALL
    assert (n.value, skipped.value) == (3, 0) and rows.tolist() == [[0, 1, 100, 5000], [0, 1, 7000, 24000]]   # what is needed; the first two written
    assert L.fvad_clips_from_segments(arr, 3, 0, 1, 48000, None, 0, fv.C.byref(n), fv.C.byref(skipped)) == TOO_SMALL and n.value == 3   # counting only
    assert L.fvad_clips_from_segments(arr, 3, 0, 0, 48000, rows.ctypes.data_as(u64p), 2, fv.C.byref(n), fv.C.byref(skipped)) == INVALID  # no channels
    assert L.fvad_clips_from_segments(None, 3, 0, 1, 48000, rows.ctypes.data_as(u64p), 2, fv.C.byref(n), fv.C.byref(skipped)) == INVALID
    assert L.fvad_clips_from_segments(arr, 3, 0, 1, 48000, rows.ctypes.data_as(u64p), 2, None, fv.C.byref(skipped)) == INVALID
    arr[1].sample_to = arr[1].sample_from                                          # not a segment
    assert L.fvad_clips_from_segments(arr, 3, 0, 1, 48000, rows.ctypes.data_as(u64p), 2, fv.C.byref(n), fv.C.byref(skipped)) == INVALID


@pytest.fixture(scope="module", params=[False, True], ids=["f32", "pcm16"])
def table(request):
    clips, names = cc.case_table()
    return cc.mask_outside(cc.make_source(request.param), clips), clips, names


def test_the_case_table_is_what_the_issue_asks_for(table):
    src, clips, names = table
    lens = (clips[:, 3] - clips[:, 2]).astype(np.int64)
    T = cc.TILE
    assert {1, 2, 3, 4, 5, 7, 8, 9, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 3} <= set(lens.tolist())
    assert {int(a) % 8 for a in clips[:, 2]} == set(range(8))
    assert clips[names["first"], 2] == 0 and clips[names["last"], 3] == cc.N_SAMPLES
    assert {int(c) for c in clips[:, 1]} == {1, 2, 3, 5} and clips[:, 0].min() > 0
    assert len({tuple(c) for c in clips.tolist()}) < len(clips)                    # a duplicate
    assert src.shape == (cc.N_LANES, cc.N_SAMPLES) and cc.N_SAMPLES <= 200000
    # the model on the table: the scaled channel wins in every position, ties go to the lower index, silence is +0.0
    m = cc.model_export(src, clips, False)
    for s, (l0, C_) in cc.STREAMS.items():
        for p in range(C_):
            assert m["best_channel"][names[f"scaled-{s}-{p}"]] == p
        i = names[f"tie-{s}"]
        assert m["best_channel"][i] == (0 if C_ <= 2 else 1)
        assert C_ == 1 or m["runner_up_rms"][i] == m["best_rms"][i]
    i = names["silence"]
    assert m["best_channel"][i] == 0 and m["best_rms"][i].tobytes() == m["runner_up_rms"][i].tobytes() == np.float32(0.0).tobytes()
    cc.compare(m, cc.model_export(src, clips, False), "the model against itself")


@pytest.mark.parametrize("mutation", ["le", "late", "lane"])
@pytest.mark.parametrize("out_pcm16", [False, True], ids=["to-f32", "to-pcm16"])
def test_a_wrong_model_fails_the_case_table(table, mutation, out_pcm16):
    src, clips, _ = table
    want = cc.model_export(src, clips, out_pcm16)
    with pytest.raises(AssertionError):
        cc.compare(cc.model_export(src, clips, out_pcm16, mutation=mutation), want, mutation)
