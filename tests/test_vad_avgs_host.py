"""The averages' tables of the device VAD machines (context option vad_avgs), the parts that need no GPU: the shared chain of
csrc/vad_avgs.h (fvad_vad_avg_chain) against the oracle's rolling average bit for bit, the keys a batch derives (shared and
unique keys, sized batches, after retain_configs), the harness's option checks and the entry points' argument rules."""
import ctypes as C

import numpy as np
import pytest

import vad_avgs_cases as A
import vad_oracle_cases as V


@pytest.fixture(scope="module")
def drift():
    """vad_oracle_cases' drift stream, 120 s at 1024 points (5625 frames)"""
    return V.long_script("drift", 5625, 1, 1024, 3)[0]


@pytest.mark.parametrize("n", A.HOST_LENS)
def test_shared_chain_is_the_oracles_rolling_average(fv, drift, n):
    x = drift[:max(3 * n + 5, 700)]
    want = A.oracle_avgs(x, n)
    got = fv.avg_chain(x, n)
    assert (A.bits(got) == A.bits(want)).all(), n
    # from a later frame on, the earlier inputs read from the ring as it was then: a part shorter than the ring, one that ends
    # on the frame that fills it, and one across a wrap
    for first in sorted({1, n - 1, n, n + 1, 2 * n + 3} - {0}):
        ring = np.zeros(n, np.float32)
        for j in range(first):
            ring[j % n] = x[j]
        for count in (1, max(n - 1, 1), len(x) - first):
            part = fv.avg_chain(x[first:first + count], n, first, ring)
            assert (A.bits(part) == A.bits(want[first:first + count])).all(), (n, first, count)


def test_chain_argument_rules(fv):
    lib = fv.lib()
    out = (C.c_double * 4)()
    x = (C.c_float * 4)(1, 2, 3, 4)
    assert lib.fvad_vad_avg_chain(x, 4, 0, 0, None, out) == fv.FVAD_ERR_INVALID_ARGUMENT      # an empty ring
    assert lib.fvad_vad_avg_chain(x, 4, 2, 3, None, out) == fv.FVAD_ERR_INVALID_ARGUMENT      # history without the ring
    assert lib.fvad_vad_avg_chain(None, 0, 0, 3, None, None) == fv.FVAD_OK


def lens(F, c, rate=48000):
    """(short_len, ratio_len) of config overrides c as VADMachine.zig:75-106 computes them (defaults 0.2 s and 0.5 s)"""
    return (max(1, V.ring_len(rate, F, c.get("short_term_speech_avg_sec", 0.2))), V.ring_len(rate, F, c.get("channel_vol_ratio_avg_sec", 0.5)))


def test_keys_shared_and_unique(fv):
    cfgs = A.shared_grid()
    sw = fv.VadSweep(2, cfgs)
    try:
        st, cr, st_key, cr_key = sw.avg_keys()
        _, band_of = sw.bands()
        assert len(st) == 8 and len(cr) == 2 and len(cfgs) == 128
        for c, cfg in enumerate(cfgs):
            assert st[st_key[c]] == (band_of[c], lens(1024, cfg)[0]) and cr[cr_key[c]] == (0, lens(1024, cfg)[1]), c
        # first-seen config order: the keys' first configs are increasing
        assert [st_key.index(j) for j in range(len(st))] == sorted(st_key.index(j) for j in range(len(st)))
        assert len(set(st)) == len(st) and len(set(cr)) == len(cr)
        assert sw.avgs_form() == 0 and sw.avgs_bytes() == 0
    finally:
        sw.close()
    cfgs = A.unique_grid(12)
    sw = fv.VadSweep(1, cfgs)
    try:
        st, cr, st_key, cr_key = sw.avg_keys()
        assert st_key == list(range(12)) and cr_key == list(range(12))
        assert st == [(0, lens(1024, c)[0]) for c in cfgs] and cr == [(0, lens(1024, c)[1]) for c in cfgs]
    finally:
        sw.close()
    one = fv.VadSweep(1, [{"short_term_speech_avg_sec": 0.0}])   # the @max(1, ...) clamp of the short window
    try:
        assert one.avg_keys()[0] == [(0, 1)]
    finally:
        one.close()


def test_keys_of_a_sized_batch_and_after_retain(fv):
    cfgs = [{"short_term_speech_avg_sec": [0.2, 0.5][i % 2], "speech_min_freq": [300.0, 600.0][(i // 2) % 2]} for i in range(12)]
    sizes = [[512, 2048, 1024][i % 3] for i in range(12)]
    sw = fv.VadSweepSized(2, cfgs, sizes)
    try:
        def check(cfgs, sizes):
            st, cr, st_key, cr_key = sw.avg_keys()
            bands, band_of = sw.bands()
            for c, (cfg, F) in enumerate(zip(cfgs, sizes)):
                assert bands[band_of[c]][0] == F
                assert st[st_key[c]] == (band_of[c], lens(F, cfg)[0]), c
                assert cr[cr_key[c]] == (sw.sizes.index(F), lens(F, cfg)[1]), c
            assert len(set(st)) == len(st) == len({(band_of[c], lens(F, cfg)[0]) for c, (cfg, F) in enumerate(zip(cfgs, sizes))})
            assert len(set(cr)) == len(cr) == len(set(sizes))
            return st, cr
        st, cr = check(cfgs, sizes)
        assert len(st) == 12 and len(cr) == 3      # (size, band, short window) are all distinct here; one ratio window per size
        # drop every config at 2048 points (a size, its bands and its keys disappear) and the only config of one more key
        keep = [c for c in range(12) if sizes[c] != 2048 and c != 3]
        sw.retain(None, keep)
        st2, cr2 = check([cfgs[c] for c in keep], [sizes[c] for c in keep])
        assert len(st2) == len(keep) and len(cr2) == 2
        fresh = fv.VadSweepSized(2, [cfgs[c] for c in keep], [sizes[c] for c in keep])
        try:
            assert fresh.avg_keys() == sw.avg_keys()
        finally:
            fresh.close()
    finally:
        sw.close()


def test_key_call_argument_rules(fv):
    lib = fv.lib()
    sw = fv.VadSweep(1, A.unique_grid(3))
    try:
        n_st, n_cr = C.c_size_t(), C.c_size_t()
        buf = (C.c_uint32 * 6)()
        assert lib.fvad_vad_batch_avg_keys(None, None, None, 0, C.byref(n_st), C.byref(n_cr), None, None) == fv.FVAD_ERR_INVALID_ARGUMENT
        assert lib.fvad_vad_batch_avg_keys(sw.h, None, None, 0, C.byref(n_st), C.byref(n_cr), None, None) == fv.FVAD_ERR_BUFFER_TOO_SMALL
        assert (n_st.value, n_cr.value) == (3, 3)
        assert lib.fvad_vad_batch_avg_keys(sw.h, buf, buf, 2, C.byref(n_st), C.byref(n_cr), None, None) == fv.FVAD_ERR_BUFFER_TOO_SMALL
        f = C.c_int(7)
        assert lib.fvad_vad_batch_avgs_form(sw.h, C.byref(f)) == fv.FVAD_OK and f.value == 0
        assert lib.fvad_vad_batch_avgs_form(None, C.byref(f)) == fv.FVAD_ERR_INVALID_ARGUMENT
        assert lib.fvad_vad_batch_avgs_bytes(None) == 0
        # no context: what the other device calls say without one
        nf, nc = (C.c_size_t * 1)(10), (C.c_size_t * 1)(1)
        rc = lib.fvad_vad_batch_averages_device(None, sw.h, None, 16, nf, None, 1, nc, 24000, 0, None, None, 16)
        assert rc in (fv.FVAD_ERR_NO_DEVICE, fv.FVAD_ERR_INVALID_ARGUMENT)
    finally:
        sw.close()


def test_harness_option_rules(pkg):
    sim = pkg.simulator
    assert sim.VAD_AVGS == ("ring", "table")
    for chain in (None, "lane"):
        with pytest.raises(ValueError) as e:
            sim._check_vad_chain(chain, "table")
        assert "vad_avgs" in str(e.value) and "vad_chain" in str(e.value)
    with pytest.raises(ValueError):
        sim._check_vad_chain("coop", "bogus")
    sim._check_vad_chain("coop", "table")
    sim._check_vad_chain("lane", "ring")
    sim._check_vad_chain(None, None)
    # before anything is read or any device touched
    with pytest.raises(ValueError) as e:
        sim.run_sweep("/nonexistent/plan.json", vad_chain="lane", vad_avgs="table")
    assert "vad_avgs" in str(e.value)
    with pytest.raises(ValueError) as e:
        sim.run_grid("/nonexistent/plan.json", {"base": {}, "axes": {}}, vad_avgs="table")
    assert "vad_avgs" in str(e.value)
    a = sim.arg_parser().parse_args(["-i", "plan.json", "--vad-chain", "coop", "--vad-avgs", "table"])
    assert a.vad_avgs == "table"
    with pytest.raises(SystemExit):
        sim.arg_parser().parse_args(["-i", "plan.json", "--vad-avgs", "lds"])


def test_option_setter_restores_both_options(pkg):
    class Ctx:
        def __init__(self):
            self.set, self.log = {"vad_chain": "lane"}, []

        def option_set(self, name):
            return self.set.get(name)

        def set_option(self, name, value):
            self.set[name] = value
            self.log.append((name, value))

    mine, theirs = Ctx(), Ctx()
    ch = pkg.simulator._VadChain("coop", "table")
    ch.apply(mine, True)
    ch.apply(theirs, False)
    ch.apply(None, False)
    assert mine.set == theirs.set == {"vad_chain": "coop", "vad_avgs": "table"}
    ch.close()
    assert theirs.set == {"vad_chain": "lane", "vad_avgs": None} and mine.set["vad_avgs"] == "table"
    only = Ctx()
    ch = pkg.simulator._VadChain("coop")
    ch.apply(only, False)
    assert only.log == [("vad_chain", "coop")]
    ch.close()
