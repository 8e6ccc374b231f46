"""The frame ratios of a device part as the host computes them from the shared header (vad_ratio.h, through
fvad_vad_batch_frame_ratios) against the oracle's VADMetadata chains (orc_meta_push), bit for bit, and the argument rules of the
calls for device parts that do not wait (fvad_vad_batch_run_device_part_async, _part_wait, _frame_ratios_device) that need no
device."""
import numpy as np
import pytest

import vad_oracle_cases as V

# vad_oracle_cases' (rate, channels, FFT size) table -- frames inside one chunk, across two, across three, sizes that do not divide
# the chunk -- and five channels at the smallest and the largest size
CASES = V.CASES + [(48000, 5, 254), (48000, 5, 16384)]
CASE_IDS = ["%dk-%dch-F%d" % (r // 1000, c, f) for r, c, f in CASES]


def rms_table(rng, n_chunks, nch):
    """chunk RMS [n_chunks][nch]: noise, with rows of zeros (max 0: ratio 0), a zero channel (min 0), equal channels (ratio 1),
    every channel above 1 (vol_min stays 1) and tiny values"""
    rms = rng.uniform(0.001, 0.6, (n_chunks, nch)).astype(np.float32)
    kinds = (np.arange(n_chunks) + int(rng.integers(0, 7))) % 7   # every kind in any seven chunks (5, 6: plain noise)
    rms[kinds == 0] = 0.0
    rms[kinds == 1, 0] = 0.0
    rms[kinds == 2] = rms[kinds == 2][:, :1]
    rms[kinds == 3] += np.float32(1.5)
    rms[kinds == 4] *= np.float32(1e-30)
    return rms


def part_starts(chunk, F, n_chunks):
    """chunks where a part may start: where a chunk and a frame start (every lcm(chunk, F) samples)"""
    step = int(np.lcm(chunk, F)) // chunk
    return [k * step for k in range(3) if k * step < n_chunks]


def case_tables(rate, nch, F, seed=0):
    chunk = V.chunk_of(rate)
    step = int(np.lcm(chunk, F)) // chunk
    n_chunks = [2 * step + 7, step + 7]   # two streams, the second one shorter
    rng = np.random.default_rng(seed + F + nch)
    return chunk, n_chunks, [rms_table(rng, k, nch) for k in n_chunks]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lanes_of(tables, start, width):
    """[streams * channels][width] from chunk `start` on, zero past a stream's end"""
    nch = tables[0].shape[1]
    out = np.zeros((len(tables) * nch, max(width, 1)), np.float32)
    for s, t in enumerate(tables):
        part = t[start:start + width].T
        out[s * nch:(s + 1) * nch, :part.shape[1]] = part
    return out


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_ratios_equal_oracle_chain(fv, case):
    rate, nch, F = case
    chunk, n_chunks, tables = case_tables(rate, nch, F)
    whole = [V.oracle_frame_ratios(t, k * chunk // F, F, chunk) for t, k in zip(tables, n_chunks)]
    sw = fv.VadSweep(2, V.case_configs(rate, F, seed=1)[:2], n_channels=nch, sample_rate=rate, fft_size=F)
    try:
        for start in part_starts(chunk, F, max(n_chunks)):
            f0 = start * chunk // F
            nc = [max(0, k - start) for k in n_chunks]
            nf = [max(0, k * chunk // F - f0) for k in n_chunks]
            got = sw.frame_ratios(lanes_of(tables, start, max(nc)), nf, nc, first_sample=start * chunk, chunk_size=chunk)
            for s in range(2):
                assert np.array_equal(bits(got[s, :nf[s]]), bits(whole[s][f0:f0 + nf[s]])), (case, start, s)
    finally:
        sw.close()


def test_host_ratios_of_a_sized_batch(fv):
    """three frame sizes in one batch: row (size, stream), every size's frames of the part"""
    rate, nch, sizes = 48000, 3, [512, 2048, 1000]
    chunk = V.chunk_of(rate)
    rng = np.random.default_rng(5)
    n_chunks = [96 + 5, 64]
    tables = [rms_table(rng, k, nch) for k in n_chunks]
    sw = fv.VadSweepSized(2, [{}, {}, {}], sizes, n_channels=nch, sample_rate=rate)
    try:
        assert sw.sizes == sizes
        for start in (0, 32, 64):   # lcm(24000, 512, 2048, 1000) = 32 chunks
            nc = [max(0, k - start) for k in n_chunks]
            nf = [[max(0, k * chunk // F - start * chunk // F) for k in n_chunks] for F in sizes]
            got = sw.frame_ratios(lanes_of(tables, start, max(nc)), nf, nc, first_sample=start * chunk, chunk_size=chunk)
            for g, F in enumerate(sizes):
                for s in range(2):
                    want = V.oracle_frame_ratios(tables[s], n_chunks[s] * chunk // F, F, chunk)[start * chunk // F:]
                    assert np.array_equal(bits(got[g * 2 + s, :nf[g][s]]), bits(want[:nf[g][s]])), (start, F, s)
    finally:
        sw.close()


def test_symbols_and_rules_without_a_device(fv):
    lib = fv.lib()
    for name in ("fvad_vad_batch_run_device_part_async", "fvad_vad_batch_part_wait", "fvad_vad_batch_frame_ratios_device",
                 "fvad_vad_batch_frame_ratios"):
        assert hasattr(lib, name), name
    INV = fv.FVAD_ERR_INVALID_ARGUMENT
    sw = fv.VadSweep(2, [{}, {"speech_threshold_factor": 3.0}])
    try:
        nf, nc = (fv.sz * 2)(375, 375), (fv.sz * 2)(16, 16)
        r = np.full((2, 16), 0.1, np.float32)
        out = np.zeros((2, 375), np.float32)
        # nothing in flight: nothing to wait for, with or without a context
        assert lib.fvad_vad_batch_part_wait(None, sw.h) == 0
        assert lib.fvad_vad_batch_part_wait(None, None) == INV
        # without a context the device calls say what fvad_ctx_create would have said (no device) or refuse the argument
        no_ctx = (fv.FVAD_ERR_NO_DEVICE, INV)
        assert lib.fvad_vad_batch_run_device_part_async(None, sw.h, None, 375, nf, None, 16, nc, 24000, 0) in no_ctx
        assert lib.fvad_vad_batch_frame_ratios_device(None, sw.h, None, 16, nf, nc, 24000, 0, None, 375) in no_ctx
        # the host twin's rules
        f = lib.fvad_vad_batch_frame_ratios
        assert f(sw.h, fv.fptr(r), 16, nf, nc, 24000, 0, fv.fptr(out), 375) == 0
        assert f(None, fv.fptr(r), 16, nf, nc, 24000, 0, fv.fptr(out), 375) == INV
        assert f(sw.h, None, 16, nf, nc, 24000, 0, fv.fptr(out), 375) == INV
        assert f(sw.h, fv.fptr(r), 16, None, nc, 24000, 0, fv.fptr(out), 375) == INV
        assert f(sw.h, fv.fptr(r), 16, nf, None, 24000, 0, fv.fptr(out), 375) == INV
        assert f(sw.h, fv.fptr(r), 16, nf, nc, 0, 0, fv.fptr(out), 375) == INV
        assert f(sw.h, fv.fptr(r), 16, nf, nc, 24000, 0, None, 375) == INV
        assert f(sw.h, fv.fptr(r), 16, nf, nc, 24000, 0, fv.fptr(out), 374) == INV          # ratio_stride < frames
        assert f(sw.h, fv.fptr(r), 15, nf, nc, 24000, 0, fv.fptr(out), 375) == INV          # rms_stride < chunks
        assert f(sw.h, fv.fptr(r), 16, (fv.sz * 2)(376, 375), nc, 24000, 0, fv.fptr(out), 376) == INV   # a frame without its chunk
        assert f(sw.h, fv.fptr(r), 16, nf, nc, 24000, 1024, fv.fptr(out), 375) == INV       # off a chunk boundary
        assert f(sw.h, fv.fptr(r), 16, nf, nc, 24000, 24000, fv.fptr(out), 375) == INV      # off a frame boundary
        assert f(sw.h, fv.fptr(r), 16, nf, nc, 24000, 16 * 24000, fv.fptr(out), 375) == 0
        assert np.all(out == 1.0)   # one channel: min == max
    finally:
        sw.close()


def test_overlap_needs_slices_and_the_device(pkg, tmp_path):
    sim = pkg.simulator
    grid = {"base": {}, "axes": {"speech_threshold_factor": [2.5, 4.0]}}
    for kw in (dict(), dict(slice_chunks=16, vad_on="host", score_on="host"), dict(slice_chunks=16, vad_on="device", score_on="host")):
        with pytest.raises(ValueError, match="overlap"):
            sim.run_grid(str(tmp_path / "no_plan.json"), grid, out=None, overlap=True, **kw)
