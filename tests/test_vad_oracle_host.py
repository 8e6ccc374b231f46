"""The VAD sweep stack on the host against the CPU oracle, bit for bit, over the config space the sweeps exist to explore: the
speech-band bins (orc_fft_freq_to_bin), the ring lengths (exact and one f32 ulp below an integer frame count, the @max clamps),
the frame ratios of frames that cross two or three chunks, the machines with their lazily exact long-term average (rings of 1,
2, 63-65, 4096, 8437 and 16875 slots, ties, thresholds <= 0, silence), parts and mixed frame sizes, and the Evaluator statistics
(orc_stats_from_segments, orc_stats_aggregate).  The yardstick is always orc_vad / orc_pipeline / orc_stats, never the library's
own host path (vad_oracle_cases.py builds both sides' inputs).  No GPU needed."""

import numpy as np
import pytest

import orc
import vad_oracle_cases as V
from test_vad_score_host import make_labels


@pytest.fixture(scope="module")
def cases(pkg, weights7):
    """one orc_pipeline run per CASES entry (on up to 16 threads)"""
    return dict(zip(V.CASES, V.oracle_cases(pkg, weights7)))


def sweep_vs_oracle(fv, case, cfgs):
    """VadSweep on the oracle's band sums and chunk RMS, orc_vad on the same band sums and the oracle's frame ratios ->
    (sweep, [(oracle segments, oracle audit)] per config)"""
    rate, nch, F, chunk = case["rate"], case["nch"], case["F"], case["chunk"]
    sw = fv.VadSweep(1, cfgs, n_channels=nch, sample_rate=rate, fft_size=F)
    bins, band_of = sw.bands()
    band = V.band_blocks(case["bins"], bins)
    rms = np.ascontiguousarray(case["rms"].T)
    sw.run(band, rms, n_threads=8, chunk_size=chunk)
    want = V.oracle_machines([(c, rate, nch, F, band[band_of[i]], case["ratio"]) for i, c in enumerate(cfgs)])
    return sw, want


def assert_machine(sw, s, c, want, what):
    segs, audit = want
    assert V.seg_bits(sw.segments(c)[s]) == V.seg_bits(segs), what
    assert V.audit_bits(sw.audit(s, c)) == V.audit_bits(audit), (what, sw.audit(s, c), audit)


# ------------------------------------------------------------------ b. bins


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_sweep_bins_equal_oracle_freq_to_bin(fv, case):
    rate, nch, F = case
    edges = V.band_edges(rate, F)
    ratio_sec = max(0.5, V.sec_for_ring(rate, F, 1)[0])   # (a channel-ratio ring of one slot at least)
    cfgs = [{"speech_min_freq": min(a, b), "speech_max_freq": max(a, b), "channel_vol_ratio_avg_sec": ratio_sec} for a in edges for b in edges]
    sw = fv.VadSweep(1, cfgs, n_channels=nch, sample_rate=rate, fft_size=F)
    bins, band_of = sw.bands()
    for i, c in enumerate(cfgs):
        want = (V.freq_to_bin(rate, F, c["speech_min_freq"]), V.freq_to_bin(rate, F, c["speech_max_freq"]))
        assert bins[band_of[i]] == want, (c, bins[band_of[i]], want)
    # a half bin on an even k: Zig's @round goes away from zero, round-half-even would stay on k
    k = 2 if F > 8 else 0
    e = V.half_bin_edge(rate, F, k)
    if np.float32(np.float32(e) / np.float32(np.float32(rate) / np.float32(F))) == np.float32(k + 0.5):
        assert V.freq_to_bin(rate, F, e) == k + 1
    sw.close()


PIPELINE_CASES = [c for c in V.CASES if c[0] == 48000]   # the reference pipeline takes 48 kHz only (VADPipeline.zig:54-57)


@pytest.mark.parametrize("case", PIPELINE_CASES, ids=[V.CASE_IDS[V.CASES.index(c)] for c in PIPELINE_CASES])
def test_pipeline_band_volumes_and_segments_equal_sweep(fv, pkg, weights7, cases, case):
    """one config straight through orc_pipeline: its band volumes are orc_band_sum over the sweep's (lo, hi), its segments the
    sweep's machine on them"""
    o = cases[case]
    rate, nch, F = case
    edges = V.band_edges(rate, F)
    cfg = {"speech_min_freq": edges[2], "speech_max_freq": edges[3],   # non-integer Hz
           "speech_threshold_factor": 3.0, "min_consecutive_sec_to_open": 0.0, "min_vad_duration_sec": 0.0, "max_speech_gap_sec": 0.5,
           "channel_vol_ratio_avg_sec": V.sec_for_ring(rate, F, 2)[0]}
    p = orc.Pipeline(weights7, n_channels=nch, sample_rate=rate, fft_size=F, vad_overrides=cfg)
    p.push(o["pcm"])
    sw = fv.VadSweep(1, [cfg], n_channels=nch, sample_rate=rate, fft_size=F)
    (lo, hi), = sw.bands()[0]
    band = V.band_sums(o["bins"], lo, hi)
    assert np.array_equal(p.band_volumes().view(np.uint32), np.ascontiguousarray(band.T).view(np.uint32))
    sw.run(np.ascontiguousarray(band[None]), np.ascontiguousarray(o["rms"].T), chunk_size=o["chunk"])
    assert V.seg_bits(sw.segments(0)[0]) == V.seg_bits(p.segments())
    assert len(p.segments()) >= 1
    sw.close()


# ------------------------------------------------------------------ c. machines on the oracle's inputs


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_sweep_machines_equal_oracle_on_pipeline_inputs(fv, pkg, cases, case):
    o = cases[case]
    rate, nch, F = case
    # the frame ratios: simulator.frame_ratios (which test d uses) is the oracle's, frames across two or three chunks included
    ratio = pkg.simulator.frame_ratios(o["rms"], len(o["ratio"]), fft_size=F, chunk=o["chunk"])
    assert np.array_equal(ratio.view(np.uint32), o["ratio"].view(np.uint32))
    cfgs = V.case_configs(rate, F, seed=F + nch)
    sw, want = sweep_vs_oracle(fv, o, cfgs)
    n_segs = 0
    for c, w in enumerate(want):
        assert_machine(sw, 0, c, w, (case, c, cfgs[c]))
        n_segs += len(w[0])
    assert n_segs >= 3
    # the scorer on these machines
    rng = np.random.default_rng(F)
    dur = o["pcm"].shape[1] / rate
    labels = [make_labels(rng, dur, max(2, int(dur / 6)), "mixed") + V.gap_labels(want[1][0], rate)]
    assert_scores(fv, sw, [[w[0] for w in want]], labels, rate)
    sw.close()


def test_frame_ratios_across_three_chunks(pkg, cases):
    """16 kHz, F = 16384: 8000-sample chunks, so most frames take three chunks' ratios"""
    o = cases[(16000, 2, 16384)]
    assert o["chunk"] == 8000
    assert sum(1 for k in range(len(o["ratio"])) if (k + 1) * 16384 // 8000 - k * 16384 // 8000 >= 2) > 10
    got = pkg.simulator.frame_ratios(o["rms"], len(o["ratio"]), fft_size=16384, chunk=8000)
    assert np.array_equal(got.view(np.uint32), o["ratio"].view(np.uint32))


# ------------------------------------------------------------------ e. scoring


def assert_scores(fv, sw, segs, labels, rate):
    """segs[s][c]: the oracle's segments of machine (s, c); every StatConfig of STAT_CFGS, every field as uint32, and the
    per-config aggregate over the streams"""
    S, NC = len(segs), len(segs[0])
    for sc in V.STAT_CFGS:
        sw.set_references(labels, sc)
        sw.score(8)
        for c in range(NC):
            got = sw.config_stats(c)
            want = np.stack([V.oracle_stats(segs[s][c], labels[s], rate, sc) for s in range(S)])
            V.assert_stats_bits(got, want, (c, sc))
            V.assert_stats_bits(V.agg_array(fv.stats_aggregate_array(np.ascontiguousarray(got))), V.oracle_aggregate(want), ("aggregate", c, sc))


# ------------------------------------------------------------------ d. long synthetic streams


@pytest.fixture(scope="module")
def long_case(pkg):
    """four 10-minute streams (drift, ties, silence, drift) at 512 / 1024 / 2048 points, stereo, and every long config's oracle
    machine on them"""
    nch, n_chunks = 2, 1200
    band, rms, ratio = V.long_inputs(pkg, nch, n_chunks)
    cfgs = {F: V.long_configs(F) for F in V.LONG_SIZES}
    jobs = [(c, V.LONG_RATE, nch, F, band[F][s], ratio[F][s]) for F in V.LONG_SIZES for s in range(len(V.LONG_KINDS))
            for c in cfgs[F]]
    res = iter(V.oracle_machines(jobs))
    want = {F: [[next(res) for _ in cfgs[F]] for _ in V.LONG_KINDS] for F in V.LONG_SIZES}
    return {"nch": nch, "n_chunks": n_chunks, "band": band, "rms": rms, "ratio": ratio, "cfgs": cfgs, "want": want}


def long_rms_lanes(L):
    return np.ascontiguousarray(L["rms"].reshape(-1, L["n_chunks"]))


@pytest.mark.parametrize("F", V.LONG_SIZES)
def test_long_streams_equal_oracle(fv, long_case, F):
    L = long_case
    cfgs, S = L["cfgs"][F], len(V.LONG_KINDS)
    sw = fv.VadSweep(S, cfgs, n_channels=L["nch"], fft_size=F)
    assert len(sw.bands()[0]) == 1
    band = np.ascontiguousarray(L["band"][F].reshape(1, S * L["nch"], -1))
    sw.run(band, long_rms_lanes(L), n_threads=8)
    lazy = 0
    for s in range(S):
        for c in range(len(cfgs)):
            assert_machine(sw, s, c, L["want"][F][s][c], (F, V.LONG_KINDS[s], cfgs[c]))
            if V.ring_len(V.LONG_RATE, F, cfgs[c]["long_term_speech_avg_sec"] if "long_term_speech_avg_sec" in cfgs[c] else 180.0) >= 4096:
                lazy += sw.lazy_stats(s, c)[1]
    assert lazy > 100000   # the lazy bound, not the eager chain, decided most frames of the long rings
    assert sum(len(L["want"][F][s][c][0]) for s in range(S) for c in range(len(cfgs))) >= 50
    # the scorer: labels of their own per stream, gaps of exactly fill_gaps inside the drift stream's first config's segments
    rng = np.random.default_rng(F)
    dur = L["n_chunks"] * V.LONG_CHUNK / V.LONG_RATE
    labels = [make_labels(rng, dur, 40, "empty" if V.LONG_KINDS[s] == "silence" else "mixed") + V.gap_labels(L["want"][F][s][0][0], V.LONG_RATE)
              for s in range(S)]
    assert_scores(fv, sw, [[w[0] for w in L["want"][F][s]] for s in range(S)], labels, V.LONG_RATE)
    sw.close()


def test_long_streams_sized_and_in_parts_equal_oracle(fv, long_case):
    """the sizes mixed in one VadSweepSized, one call and parts split at random chunk boundaries (multiples of 32 chunks: where
    a chunk and a frame of every size start)"""
    L = long_case
    S, nch = len(V.LONG_KINDS), L["nch"]
    order = [(F, c) for c in range(max(len(L["cfgs"][F]) for F in V.LONG_SIZES)) for F in V.LONG_SIZES if c < len(L["cfgs"][F])]
    cfgs = [L["cfgs"][F][c] for F, c in order]
    sizes = [F for F, _ in order]
    rms = long_rms_lanes(L)

    def blocks(sw, f0=0, f1=None):
        bands, _ = sw.bands()
        stride = max(L["band"][F].shape[2] for F in V.LONG_SIZES)
        out = np.zeros((len(bands), S * nch, stride), np.float32)
        for j, (F, _, _) in enumerate(bands):
            b = L["band"][F].reshape(S * nch, -1)
            out[j, :, :b.shape[1]] = b
        return out

    def check(sw):
        for i, (F, c) in enumerate(order):
            for s in range(S):
                assert_machine(sw, s, i, L["want"][F][s][c], (F, V.LONG_KINDS[s], cfgs[i]))

    one = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    band = blocks(one)
    one.run(band, rms, [L["n_chunks"] * V.LONG_CHUNK // F for F in one.sizes], n_threads=8)
    check(one)
    one.close()
    rng = np.random.default_rng(5)
    cuts = sorted(set(int(x) * 32 for x in rng.integers(1, L["n_chunks"] // 32, 4))) + [L["n_chunks"]]
    parts = fv.VadSweepSized(S, cfgs, sizes, n_channels=nch)
    c0 = 0
    for c1 in cuts:
        s0 = c0 * V.LONG_CHUNK
        nf = [(c1 - c0) * V.LONG_CHUNK // F for F in parts.sizes]
        bands, _ = parts.bands()
        stride = max(nf)
        pb = np.zeros((len(bands), S * nch, stride), np.float32)
        for j, (F, _, _) in enumerate(bands):
            pb[j, :, :nf[parts.sizes.index(F)]] = L["band"][F].reshape(S * nch, -1)[:, s0 // F: s0 // F + nf[parts.sizes.index(F)]]
        parts.run(pb, np.ascontiguousarray(rms[:, c0:c1]), nf, first_sample=s0, n_threads=8)
        c0 = c1
    check(parts)
    parts.close()


# ------------------------------------------------------------------ f. refusals


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_empty_channel_ratio_ring_is_refused(fv, case):
    """the oracle has no @max on the channel-ratio ring (VADMachine.zig:101-105); a ring of 0 slots is a documented deviation:
    the library refuses the config"""
    rate, nch, F = case
    below_one = V.sec_for_ring(rate, F, 1)[1]
    assert V.ring_len(rate, F, below_one) == 0
    for cfgs in ([{"channel_vol_ratio_avg_sec": below_one}], [{}, {"channel_vol_ratio_avg_sec": 0.0}]):
        with pytest.raises(fv.FvadError) as e:
            fv.VadSweep(1, cfgs, n_channels=nch, sample_rate=rate, fft_size=F)
        assert e.value.status == fv.FVAD_ERR_INVALID_ARGUMENT
