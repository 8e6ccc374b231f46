"""K1 (stft_kernel) and K3 (istft_kernel) on the GPU against float64, one kernel at a time, through fvad_engine_run's taps:
every workgroup form (three, two, one workgroup per chunk) and both thresholds between them, lanes that continue across launches
and across calls, PCM16, gain models whose bits do not depend on the launch size, the 48 kHz lerp bit for bit, canaries.
References, metric, gain models and tolerances: denoise_cases.py (k4_cases.GPU_FACTOR x the oracle's measured distance; nothing
here is derived from GPU output).  Every test prints its worst distance before it asserts (pytest -s)."""
import numpy as np
import pytest

import denoise_cases as dc
import k4_cases as k4
from test_k4_bands_gpu import CANARY

pytestmark = pytest.mark.gpu

# ragged lanes, 129 chunks: `first` / `last` descriptors fall inside a launch, and under every cap but 129 the 86-chunk lane (under
# caps 85, 2 and 1 the 40-chunk lane too) continues across launches of one call
LANES = (1, 2, 40, 86)
TOTAL = sum(LANES)
# max_chunks_per_launch -> launches (nn_dispatch.cpp run_chunks: lane-contiguous, `cap` chunks and a remainder) -> fft_parts
# (3 up to 85 chunks, 2 up to 128, then 1):  129 -> [129]: 1;  128 -> [128, 1]: 2, 3;  86 -> [86, 43]: 2, 3;  85 -> [85, 44]: 3, 3;
# 2 -> 64 x [2], [1]: 3;  1 -> 129 x [1]: 3
CAPS = (129, 128, 86, 85, 2, 1)
# the same lanes in two calls through lane_state: (chunks of each lane in the first call; the rest in the second), cap 86
CALL_SPLIT = (1, 1, 17, 67)

SPEC_TOL = k4.GPU_FACTOR * dc.ORACLE_SPEC_UNITS
FEAT_TOL = k4.GPU_FACTOR * dc.ORACLE_FEAT_UNITS
RMS_TOL = k4.GPU_FACTOR * dc.ORACLE_RMS_UNITS

_CACHE = {}


def case_lanes():
    if "lanes" not in _CACHE:
        _CACHE["lanes"] = [dc.make_lane(l, n) for l, n in enumerate(LANES)]
    return _CACHE["lanes"]


def case_ref_k1():
    """float64 K1 reference of every lane, computed once and left unchanged"""
    if "k1" not in _CACHE:
        _CACHE["k1"] = [dc.ref_lane_k1(x) for x in case_lanes()]
    return _CACHE["k1"]


KEYS = ("spectrogram", "features", "chunk_rms", "denoised")


def run(fv, ctx, lanes, cap, split=None, i16_out=False):
    """engine_run over the lanes with taps; split: chunks of each lane that go into a first call, the rest into a second one
    through the lane's state.  Returns one dict per lane (the calls' outputs joined)."""
    kw = dict(want_taps=True, want_denoised=True, want_denoised_i16=i16_out, max_chunks_per_launch=cap)
    if split is None:
        return ctx.engine_run(lanes, **kw)
    states = [ctx.lane_state() for _ in lanes]
    try:
        first = ctx.engine_run([x[: n * dc.CHUNK] for x, n in zip(lanes, split)], states=states, **kw)
        rest = [i for i, (x, n) in enumerate(zip(lanes, split)) if len(x) > n * dc.CHUNK]
        second = ctx.engine_run([lanes[i][split[i] * dc.CHUNK:] for i in rest], states=[states[i] for i in rest], **kw)
    finally:
        for st in states:
            fv.lib().fvad_lane_state_destroy(st)
    out = []
    for i, a in enumerate(first):
        parts = [a] + ([second[rest.index(i)]] if i in rest else [])
        out.append({k: np.concatenate([p[k] for p in parts]) for k in KEYS + (("denoised_i16",) if i16_out else ())})
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype != np.int16 else np.uint16)


def same_bits(a, b, keys, what):
    for l, (u, v) in enumerate(zip(a, b)):
        for k in keys:
            assert u[k].shape == v[k].shape and np.array_equal(bits(u[k]), bits(v[k])), f"{what}: lane {l}, {k} differs"


def k1_distances(outs, refs, what):
    """worst spectrogram / feature / RMS distance over the lanes; prints, then asserts"""
    ws = wf = wr = 0.0
    for l, (o, (X, _, rms)) in enumerate(zip(outs, refs)):
        assert o["spectrogram"].shape == X.shape and o["features"].shape == (X.shape[0], dc.ROWS, dc.NB)
        s, ps = dc.spec_units(o["spectrogram"], X)
        f, pf = dc.feat_units(o["features"][:, dc.WARM:], X)
        r, pr = dc.rms_units(o["chunk_rms"], rms)
        print(f"\n    {what}, lane {l}: spectrogram {s:.3g} (tolerance {SPEC_TOL:.3g}) at frame/bin {ps}; features {f:.3g} "
              f"(tolerance {FEAT_TOL:.3g}) at {pf}; rms {r:.3g} (tolerance {RMS_TOL:.5g}; tree bound {dc.RMS_TREE_UNITS:g}) at chunk {pr}")
        ws, wf, wr = max(ws, s), max(wf, f), max(wr, r)
    assert ws <= SPEC_TOL and wf <= FEAT_TOL and wr <= RMS_TOL, (what, ws, wf, wr)
    # the oracle-derived RMS tolerance is blind to a missing sample; the a-priori bound of a 96-long chain under an 8-level tree
    assert wr <= dc.RMS_TREE_UNITS, (what, wr, dc.RMS_TREE_UNITS)
    return ws, wf, wr


def assert_warmup_rows(outs, what):
    for l, o in enumerate(outs):
        f = bits(o["features"])
        assert not f[0, :dc.WARM].any(), f"{what}: lane {l}: rows 0..3 of the first chunk are not literal +0.0"
        assert np.array_equal(f[1:, :dc.WARM], f[:-1, dc.FRAMES:]), f"{what}: lane {l}: warm-up rows != the previous chunk's rows 50..53"


def test_forced_launch_sizes_cover_every_form():
    sizes = {n for cap in CAPS for n in dc.launch_sizes(TOTAL, cap)}
    assert {1, 2, 85, 86, 128, 129} <= sizes
    assert {cap: [dc.fft_parts(n) for n in dc.launch_sizes(TOTAL, cap)][:2] for cap in CAPS} == \
        {129: [1], 128: [2, 3], 86: [2, 3], 85: [3, 3], 2: [3, 3], 1: [3, 3]}
    assert sum(CALL_SPLIT) == 86 and all(0 < a <= b for a, b in zip(CALL_SPLIT, LANES))


# ------------------------------------------------------------------ a. K1

def test_k1_taps_and_rms_against_float64_at_every_launch_size(fv, gpu_ctx):
    lanes, refs = case_lanes(), case_ref_k1()
    base = None
    for cap in CAPS:
        outs = run(fv, gpu_ctx, lanes, cap)
        what = f"K1, launches of {cap}"
        assert [o["n_chunks"] for o in outs] == list(LANES)
        k1_distances(outs, refs, what)
        assert_warmup_rows(outs, what)
        if base is None:
            base = outs
        same_bits(outs, base, KEYS[:3], f"{what} against launches of {CAPS[0]}")
    # a lane that continues across two calls through lane_state (and across the launches of each call)
    outs = run(fv, gpu_ctx, lanes, 86, split=CALL_SPLIT)
    k1_distances(outs, refs, "K1, two calls")
    assert_warmup_rows(outs, "K1, two calls")
    same_bits(outs, base, KEYS[:3], "K1, two calls against one")
    _CACHE["features"] = [o["features"] for o in base]


def test_k1_pcm16_is_the_f32_run_on_s_over_32768(fv, gpu_ctx):
    lanes16 = [dc.to_pcm16(x) for x in case_lanes()]
    lanes16[3][:8] = [-32768, 32767, 0, 1, -1, 12345, -12345, 7]
    lanes32 = [dc.as_f32(s) for s in lanes16]
    refs = [dc.ref_lane_k1(s) for s in lanes16]
    for cap in (129, 86):
        a, b = run(fv, gpu_ctx, lanes16, cap), run(fv, gpu_ctx, lanes32, cap)
        same_bits(a, b, KEYS, f"PCM16 against f32, launches of {cap}")
        assert_warmup_rows(a, f"PCM16, launches of {cap}")
    k1_distances(a, refs, "K1, PCM16")
    a2, b2 = run(fv, gpu_ctx, lanes16, 85, split=CALL_SPLIT), run(fv, gpu_ctx, lanes32, 85, split=CALL_SPLIT)
    same_bits(a2, b2, KEYS, "PCM16 against f32, two calls")
    same_bits(a2, a, KEYS[:3], "PCM16 in two calls against one")


# ------------------------------------------------------------------ b. the premise of the gain models

def feature_taps(fv, gpu_ctx):
    if "features" not in _CACHE:
        _CACHE["features"] = [o["features"] for o in run(fv, gpu_ctx, case_lanes(), 129)]
    return _CACHE["features"]


@pytest.mark.parametrize("name", dc.MODELS)
def test_gain_models_give_the_same_bits_at_every_batch_size(fv, gpu_ctx, name):
    taps = feature_taps(fv, gpu_ctx)
    labels = [l for l, _ in dc.table()]
    idx = dc.lane_indices(3, LANES[3])
    pick = [idx.index(labels.index(n)) for n in ("flip tone b", "noise 1.0", "quiet bins")]
    f3 = np.ascontiguousarray(taps[3][pick])
    try:
        gpu_ctx.load_weights(dc.model_weights(name))
        one = np.concatenate([gpu_ctx.nsnet2_forward(f3[i: i + 1]) for i in range(3)])
        path_one = gpu_ctx.last_nn_path()
        many = gpu_ctx.nsnet2_forward(np.tile(f3, (700, 1, 1)))         # 2100 sequences: row-panel MFMA kernels, multi-wave recurrence
        path_many = gpu_ctx.last_nn_path()
        lane = gpu_ctx.nsnet2_forward(taps[3])                          # 86 sequences, as K3's reference takes them
    finally:
        gpu_ctx.load_synth(7)
    want = dc.closed_form_gains(name, f3)
    e = np.abs(one.astype(np.float64) - want).max()
    diff = {"2100 sequences": bits(many.reshape(700, 3, dc.ROWS, dc.NB)) != bits(one)[None], "86 sequences": bits(lane[pick]) != bits(one)}
    print(f"\n    {name}: {path_one} | {path_many}\n    gains {e:.3g} from the closed form (bound {dc.GAIN_ABS_TOL:.3g}); "
          + "; ".join(f"{k}: {int(v.sum())} values differ from one sequence's" for k, v in diff.items()))
    for k, v in diff.items():
        if v.any():
            i = tuple(int(t) for t in np.argwhere(v)[0])
            print(f"    {k}: first difference at {i}")
    assert path_one != path_many, (path_one, path_many)
    assert e <= dc.GAIN_ABS_TOL, (name, e)
    assert np.abs(many[-3:].astype(np.float64) - want).max() <= dc.GAIN_ABS_TOL
    assert not any(v.any() for v in diff.values()), name
    if name == "select_alternating":
        g = one[0, dc.WARM:]
        assert (g[1::2] > 0.999).all() and (g[2::2] < 0.001).all()


# ------------------------------------------------------------------ c. K3

def k3_distances(gpu_ctx, outs, name, what):
    """reference: the K1 spectrogram tap of the same call, the gains of (b) for the same feature tap (rows 4..53), carries in
    float64 from the lane's beginning.  The model `name` must be loaded.  Returns (worst, worst at seams, worst at run boundaries)."""
    tol = k4.GPU_FACTOR * dc.ORACLE_DEN_UNITS[name]
    w = ws = wb = 0.0
    for l, o in enumerate(outs):
        n = o["spectrogram"].shape[0]
        g = gpu_ctx.nsnet2_forward(o["features"])[:, dc.WARM:]
        r = dc.ref_k3(o["spectrogram"], g)
        u = dc.den_units(o["denoised"], r)
        i = int(np.argmax(u))
        seam, bound = float(u[dc.seam_mask(n)].max()), float(u[dc.run_boundary_mask(n)].max())
        print(f"\n    {what}, lane {l}: worst {u[i]:.3g} units (tolerance {tol:.3g}) at chunk {i // dc.CHUNK} sample {i % dc.CHUNK}; "
              f"chunk seams {seam:.3g}; run boundaries {bound:.3g}")
        w, ws, wb = max(w, float(u[i])), max(ws, seam), max(wb, bound)
    assert w <= tol, (what, w, tol)
    return w, ws, wb


@pytest.mark.parametrize("name", dc.MODELS)
def test_k3_against_float64_at_every_launch_size(fv, gpu_ctx, name):
    lanes = case_lanes()
    try:
        gpu_ctx.load_weights(dc.model_weights(name))
        base = run(fv, gpu_ctx, lanes, CAPS[0], i16_out=True)
        k3_distances(gpu_ctx, base, name, f"K3 under {name}, launches of {CAPS[0]}")
        for l, o in enumerate(base):        # the PCM16 copy
            q = np.rint(np.clip(o["denoised"] * np.float32(32768.0), -32768.0, 32767.0)).astype(np.int16)
            assert np.array_equal(o["denoised_i16"], q), (name, l)
        if name == "select_alternating":    # frame f's gains ~ 1, frame f + 1's ~ 0: a gain-row offset would be an O(1) error
            c = dc.lane_indices(3, LANES[3]).index([l for l, _ in dc.table()].index("flip tone b"))
            g = gpu_ctx.nsnet2_forward(base[3]["features"][c: c + 1])[0, dc.WARM:]
            assert (g[1::2] > 0.999).all() and (g[2::2] < 0.001).all()
            assert np.abs(base[3]["denoised"][c * dc.CHUNK: (c + 1) * dc.CHUNK]).max() > 0.1
        runs = [(f"launches of {cap}", run(fv, gpu_ctx, lanes, cap)) for cap in CAPS[1:]]
        runs.append(("two calls", run(fv, gpu_ctx, lanes, 86, split=CALL_SPLIT, i16_out=True)))
        for what, outs in runs:
            # the same bits whichever launch size produced them; where not, the distance of that run before the failure
            try:
                same_bits(outs, base, KEYS + (("denoised_i16",) if outs[0].get("denoised_i16") is not None else ()), f"K3 under {name}, {what}")
            except AssertionError:
                k3_distances(gpu_ctx, outs, name, f"K3 under {name}, {what}")
                raise
    finally:
        gpu_ctx.load_synth(7)


# ------------------------------------------------------------------ d. the 48 kHz lerp, bit for bit, on the product path

def test_lerp_48k_is_fused_bit_for_bit_through_the_engine(fv, gpu_ctx):
    lanes = case_lanes()
    for what, outs in (("one launch", run(fv, gpu_ctx, lanes, 129)), ("launches of 2", run(fv, gpu_ctx, lanes[:3], 2)),
                       ("two calls, launches of 85", run(fv, gpu_ctx, lanes, 85, split=CALL_SPLIT))):
        n_bad = 0
        for l, o in enumerate(outs):
            y = o["denoised"]
            assert np.abs(y).max() > 1e-3 and np.isfinite(y).all()
            want = dc.fused_lerp_rows(y)            # every m >= 1: chunk, launch and call boundaries are just samples
            got = y.reshape(-1, 3)[1:, :2]
            n_bad += int((bits(got) != bits(want)).sum())
            # t = 0: a = 0
            d0 = np.float64(np.float32(y[2] - np.float32(0.0)))
            first = [np.float32(d0 * np.float64(np.float32(j + 1) / np.float32(3))) for j in range(2)]
            assert bits(y[:2]).tolist() == bits(np.array(first, np.float32)).tolist(), (what, l)
        print(f"\n    lerp, {what}: {n_bad} interpolated samples differ from the fused lerp of their neighbours")
        assert n_bad == 0, what


# ------------------------------------------------------------------ e. canaries around device-resident outputs

def test_device_outputs_stay_inside_their_buffers(fv, gpu_ctx):
    # fvad_engine_enqueue_device packs its outputs: lane l's denoised samples at d_den + l * n_chunks * 24000 (lane_stride spaces
    # the INPUT lanes only), its RMS at d_rms + l * n_chunks, its band sums at d_band + l * n_frames.  The buffers here are as long
    # as a strided layout would need, full of canaries: every sample inside [0, n_chunks * 24000) of every lane is written, nothing
    # behind the packed lanes -- neither the 12345-sample tail of n_samples nor the gap up to lane_stride exists on the output
    # side, and a kernel that wrote them as if they did would land in the canaries.  The input's tail and gaps are NaN.
    n_ch, n_lanes = 3, 3
    n_samples, lane_stride = n_ch * dc.CHUNK + 12345, n_ch * dc.CHUNK + 12345 + 1003
    assert lane_stride % 4 == 0 and lane_stride > n_samples
    lanes = [dc.make_lane(l + 1, n_ch) for l in range(n_lanes)]
    host = np.full(n_lanes * lane_stride, np.nan, np.float32)
    for l, x in enumerate(lanes):
        host[l * lane_stride: l * lane_stride + n_ch * dc.CHUNK] = x
    n_den, n_frames = n_ch * dc.CHUNK, n_ch * dc.CHUNK // 1024
    sizes = {"pcm": host.size, "den": n_lanes * lane_stride, "band": n_lanes * (n_frames + 8), "rms": n_lanes * (n_ch + 5)}
    d = {k: gpu_ctx.device_alloc(4 * n) for k, n in sizes.items()}
    try:
        want = gpu_ctx.engine_run(lanes, want_denoised=True)
        for cap in (0, 2):      # one launch; launches that end inside lanes
            gpu_ctx.to_device(d["pcm"], host)
            for k in ("den", "band", "rms"):
                gpu_ctx.to_device(d[k], np.full(sizes[k], CANARY, np.uint32))
            gpu_ctx.enqueue_device(d["pcm"], n_lanes, lane_stride, n_samples, d["den"], d["band"], d["rms"], max_chunks_per_launch=cap)
            den, band, rms = (gpu_ctx.to_host(np.empty(sizes[k], np.uint32), d[k]) for k in ("den", "band", "rms"))
            for k, buf, used in (("den", den, n_lanes * n_den), ("band", band, n_lanes * n_frames), ("rms", rms, n_lanes * n_ch)):
                assert not (buf[:used] == CANARY).any(), f"{k}: a value inside the lanes was not written (launches of {cap})"
                assert (buf[used:] == CANARY).all(), f"{k}: a canary behind the packed lanes was overwritten (launches of {cap})"
            for l, o in enumerate(want):
                assert np.array_equal(den[l * n_den: (l + 1) * n_den], bits(o["denoised"])), (cap, l)
                assert np.array_equal(rms[l * n_ch: (l + 1) * n_ch], bits(o["chunk_rms"])), (cap, l)
                assert np.array_equal(band[l * n_frames: (l + 1) * n_frames], bits(o["band_sum"])), (cap, l)
    finally:
        for a in d.values():
            gpu_ctx.device_free(a)
