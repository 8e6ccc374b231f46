"""The device VAD machines (kernels_vad.hip: both lane maps, both ring forms, the sized form, parts with segment overflow) and the
device scorer against the CPU oracle directly, bit for bit, on the inputs of test_vad_oracle_host.py: the oracle's band sums and
frame ratios of every (rate, channels, FFT size) case, 5-minute synthetic streams with rings of 1 .. 16875 slots, ties and
silence at 1, 2 and 5 channels, and two-hour streams at 512 and 1024 points."""
import numpy as np
import pytest

import vad_oracle_cases as V
from test_vad_oracle_host import cases  # noqa: F401  (the module-scoped oracle pipeline runs)
from test_vad_score_host import make_labels

pytestmark = pytest.mark.gpu


def upload(ctx, arr):
    d = ctx.device_alloc(arr.nbytes)
    ctx.to_device(d, arr)
    return d


def assert_machine(sw, s, c, want, what):
    segs, audit = want
    assert V.seg_bits(sw.segments(c)[s]) == V.seg_bits(segs), what
    assert V.audit_bits(sw.audit(s, c)) == V.audit_bits(audit), (what, sw.audit(s, c), audit)


def assert_audits(sw, s, c, want, what):
    assert V.audit_bits(sw.audit(s, c)) == V.audit_bits(want[1]), (what, sw.audit(s, c), want[1])


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_device_equals_oracle_on_case_inputs(fv, gpu_ctx, cases, case):  # noqa: F811
    ctx = gpu_ctx
    o = cases[case]
    rate, nch, F = case
    chunk = o["chunk"]
    cfgs = V.case_configs(rate, F, seed=F + nch)
    probe = fv.VadSweep(1, cfgs, n_channels=nch, sample_rate=rate, fft_size=F)
    bins, band_of = probe.bands()
    probe.close()
    band = V.band_blocks(o["bins"], bins)
    rms = np.ascontiguousarray(o["rms"].T)
    nf, nc = band.shape[2], rms.shape[1]
    want = V.oracle_machines([(c, rate, nch, F, band[band_of[i]], o["ratio"]) for i, c in enumerate(cfgs)])
    # parts start where a chunk and a frame start: every lcm(chunk, F) samples
    step = np.lcm(chunk, F) // chunk
    rng = np.random.default_rng(F)
    cuts = sorted(set(int(x) * step for x in rng.integers(1, max(2, nc // step), 3) if 0 < x * step < nc)) + [nc]
    for lane_map in ("stream", "config"):
        ctx.set_option("vad_lane_map", lane_map)
        try:
            sw = fv.VadSweep(1, cfgs, n_channels=nch, sample_rate=rate, fft_size=F)
            d = upload(ctx, band)
            try:
                sw.run_device(ctx, d, nf, [nf], rms, [nc], chunk_size=chunk)
            finally:
                ctx.device_free(d)
            for c in range(len(cfgs)):
                assert_machine(sw, 0, c, want[c], (case, lane_map, c, cfgs[c]))
            sw.close()
            parts = fv.VadSweep(1, cfgs, n_channels=nch, sample_rate=rate, fft_size=F)
            c0 = 0
            for c1 in cuts:
                f0, f1 = c0 * chunk // F, min(nf, c1 * chunk // F)
                pb = np.ascontiguousarray(band[:, :, f0:max(f1, f0 + 1)])
                d = upload(ctx, pb)
                try:
                    parts.run_device_part(ctx, d, pb.shape[2], [f1 - f0], np.ascontiguousarray(rms[:, c0:c1]), [c1 - c0], f0, chunk_size=chunk)
                finally:
                    ctx.device_free(d)
                c0 = c1
            for c in range(len(cfgs)):
                assert_machine(parts, 0, c, want[c], (case, lane_map, "parts", cuts, c, cfgs[c]))
            parts.close()
        finally:
            ctx.set_option("vad_lane_map", None)


@pytest.fixture(scope="module", params=[1, 2, 5], ids=["1ch", "2ch", "5ch"])
def long_dev(request, pkg):
    """5-minute synthetic streams at 512 / 1024 / 2048 points (a 16875-slot ring turns over 1.7 times), the long configs plus
    short-term windows of 3 s at 512 points (282 slots: the rings leave LDS for global memory), and their oracle machines"""
    nch, n_chunks = request.param, 600
    band, rms, ratio = V.long_inputs(pkg, nch, n_chunks, seed=10 * nch)
    cfgs, sizes = [], []
    for F in V.LONG_SIZES:
        for c in V.long_configs(F):
            cfgs.append(c)
            sizes.append(F)
    for lt in (30.0, V.sec_for_ring(V.LONG_RATE, 512, 4096)[0]):
        cfgs.append({"short_term_speech_avg_sec": 3.0, "long_term_speech_avg_sec": lt, "speech_threshold_factor": 2.0})
        sizes.append(512)
    S = len(V.LONG_KINDS)
    jobs = [(c, V.LONG_RATE, nch, F, band[F][s], ratio[F][s]) for s in range(S) for c, F in zip(cfgs, sizes)]
    res = iter(V.oracle_machines(jobs))
    want = [[next(res) for _ in cfgs] for _ in range(S)]
    rng = np.random.default_rng(nch)
    dur = n_chunks * V.LONG_CHUNK / V.LONG_RATE
    labels = [make_labels(rng, dur, 40, "empty" if k == "silence" else "mixed") + V.gap_labels(want[s][0][0], V.LONG_RATE)
              for s, k in enumerate(V.LONG_KINDS)]
    return {"nch": nch, "n_chunks": n_chunks, "band": band, "rms": np.ascontiguousarray(rms.reshape(-1, n_chunks)), "cfgs": cfgs,
            "sizes": sizes, "want": want, "labels": labels}


def sized_blocks(sw, L, S, f0=None, nf=None):
    """the band blocks of a sized sweep in bands() order, [n_bands][lanes][stride], frames [f0[F], f0[F] + nf[F])"""
    bands, _ = sw.bands()
    nch = L["nch"]
    stride = max(nf.values()) if nf else max(L["band"][F].shape[2] for F in V.LONG_SIZES)
    out = np.zeros((len(bands), S * nch, max(stride, 1)), np.float32)
    for j, (F, _, _) in enumerate(bands):
        b = L["band"][F].reshape(S * nch, -1)
        a = f0[F] if f0 else 0
        n = nf[F] if nf else b.shape[1]
        out[j, :, :n] = b[:, a:a + n]
    return out


def test_device_long_streams_equal_oracle(fv, gpu_ctx, long_dev):
    """one launch; both lane maps at two channels (a tie-heavy stream runs the exact chain on most frames, so each launch is
    slow)"""
    ctx, L = gpu_ctx, long_dev
    S, NC, nc = len(V.LONG_KINDS), len(L["cfgs"]), L["n_chunks"]
    for lane_map in (("stream", "config") if L["nch"] == 2 else ("stream",)):
        ctx.set_option("vad_lane_map", lane_map)
        try:
            sw = fv.VadSweepSized(S, L["cfgs"], L["sizes"], n_channels=L["nch"])
            band = sized_blocks(sw, L, S)
            d = upload(ctx, band)
            try:
                sw.run_device(ctx, d, band.shape[2], [[nc * V.LONG_CHUNK // F] * S for F in sw.sizes], L["rms"], [nc] * S)
            finally:
                ctx.device_free(d)
            lazy = 0
            for s in range(S):
                for c in range(NC):
                    assert_machine(sw, s, c, L["want"][s][c], (lane_map, V.LONG_KINDS[s], L["sizes"][c], L["cfgs"][c]))
                    lazy += sw.lazy_stats(s, c)[1]
            assert lazy > 20000
            sw.close()
        finally:
            ctx.set_option("vad_lane_map", None)


def run_parts(fv, ctx, L, S, keep, cuts):
    sw = fv.VadSweepSized(S, L["cfgs"], L["sizes"], n_channels=L["nch"])
    sw.keep_segments(keep)
    if not keep:
        sw.set_references(L["labels"], V.STAT_CFGS[1])
    c0 = 0
    for c1 in cuts:
        s0 = c0 * V.LONG_CHUNK
        nf = {F: (c1 - c0) * V.LONG_CHUNK // F for F in sw.sizes}
        pb = sized_blocks(sw, L, S, {F: s0 // F for F in sw.sizes}, nf)
        d = upload(ctx, pb)
        try:
            sw.run_device_part(ctx, d, pb.shape[2], [[nf[F]] * S for F in sw.sizes], np.ascontiguousarray(L["rms"][:, c0:c1]),
                               [c1 - c0] * S, s0)
        finally:
            ctx.device_free(d)
        c0 = c1
    return sw


def test_device_parts_overflow_and_scores_equal_oracle(fv, gpu_ctx, long_dev):
    """parts at random chunk boundaries where a frame of every size starts (multiples of 32 chunks), two segments of room per
    machine (every busy machine overflows), then (at two channels) the segments left on the device scored there"""
    ctx, L = gpu_ctx, long_dev
    S, NC, nc = len(V.LONG_KINDS), len(L["cfgs"]), L["n_chunks"]
    rng = np.random.default_rng(L["nch"])
    cuts = sorted(set(int(x) * 32 for x in rng.integers(1, nc // 32, 5))) + [nc]
    ctx.set_option("vad_seg_cap", "2")
    try:
        sw = run_parts(fv, ctx, L, S, True, cuts)
        for s in range(S):
            for c in range(NC):
                assert_machine(sw, s, c, L["want"][s][c], ("parts", cuts, V.LONG_KINDS[s], L["sizes"][c], L["cfgs"][c]))
        sw.close()
        if L["nch"] != 2:
            return
        sw = run_parts(fv, ctx, L, S, False, cuts)
        sw.score_device(ctx)
        for c in range(NC):
            want = np.stack([V.oracle_stats(L["want"][s][c][0], L["labels"][s], V.LONG_RATE, V.STAT_CFGS[1]) for s in range(S)])
            V.assert_stats_bits(sw.config_stats(c), want, (c, L["cfgs"][c]))
            for s in range(S):
                assert_audits(sw, s, c, L["want"][s][c], ("score_device", s, c))
        sw.close()
    finally:
        ctx.set_option("vad_seg_cap", None)


@pytest.mark.parametrize("F", [512, 1024])
def test_two_hour_stream_equals_oracle(fv, pkg, gpu_ctx, F):
    """two hours of drift and ties, one channel: a 180 s long-term ring (16875 slots at 512 points, 8437 at 1024) among 5 configs"""
    ctx = gpu_ctx
    n_chunks = 14400
    nf = n_chunks * V.LONG_CHUNK // F
    band = np.concatenate([V.long_script("drift", nf // 2, 1, F, 3), V.long_script("ties", nf - nf // 2, 1, F, 4)], axis=1)
    rms = np.full((1, n_chunks), 0.1, np.float32)
    ratio = pkg.simulator.frame_ratios(rms.T, nf, fft_size=F, chunk=V.LONG_CHUNK)
    one = V.sec_for_ring(V.LONG_RATE, F, 1)[0]
    cfgs = [{}, {"has_initial_long_term_avg": 0, "speech_threshold_factor": 4.0},
            {"speech_threshold_factor": 1.0, "short_term_speech_avg_sec": one, "long_term_speech_avg_sec": V.sec_for_ring(V.LONG_RATE, F, 4096)[1]},
            {"long_term_speech_avg_sec": 30.0, "speech_threshold_factor": 3.0, "short_term_speech_avg_sec": 3.0},
            {"initial_long_term_avg": 0.0, "speech_threshold_factor": 0.0}]
    want = V.oracle_machines([(c, V.LONG_RATE, 1, F, band, ratio) for c in cfgs])
    sw = fv.VadSweep(1, cfgs, fft_size=F)
    blk = np.ascontiguousarray(band[None])
    d = upload(ctx, blk)
    try:
        sw.run_device(ctx, d, nf, [nf], rms, [n_chunks])
    finally:
        ctx.device_free(d)
    for c in range(len(cfgs)):
        assert_machine(sw, 0, c, want[c], (F, cfgs[c]))
    assert sum(len(w[0]) for w in want) >= 20
    sw.close()
