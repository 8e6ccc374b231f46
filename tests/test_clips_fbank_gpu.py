"""The filter-bank clip export on the GPU (fvad_clips_export_fbank(_device), csrc/kernels_clips_mel.hip with the conditioned form
on) against clip_fbank_cases.py's float64 model, in its units, on exactly the samples the kernel is given.

The arena, the device buffers and the canaries are test_clips_mel_gpu.py's: lanes filled with NaN (f32) or a loud sentinel
(PCM16) around every clip, NaN on every off-stride sample of the one-channel f32 clips, a canary in every float of the output
that is no feature.  Shapes are the smallest at which the kernel takes another path: clips of exactly win_length samples, of
win + hop q and +- 1, of 31, 32 and 33 frames (a tile holds 32) and of three and a half tiles."""
import ctypes as C

import numpy as np
import pytest

import clip_fbank_cases as fc
from test_clips_mel_gpu import CANARY, SLACK, Arena, Device

pytestmark = pytest.mark.gpu

INVALID, OUT_OF_RANGE, TOO_SMALL = -100, -6, -106
SHAPE_IDS = ["/".join(map(str, s)) for s in fc.SHAPES]
TIMED = ["clip_rms", "clip_pick", "clip_fbank", "clip_fbank_mean"]


def clip_lengths(shape):
    """stream lengths L: exactly win; win + hop q and +- 1; 31, 32 and 33 frames; three and a half tiles of frames"""
    win, _, hop, _ = shape
    F, q = fc.tile_frames(win, hop), 5
    assert F == fc.TILE_FRAMES
    return [win, win + hop * q, win + hop * q - 1, win + hop * q + 1, win + 30 * hop, win + 31 * hop, win + 32 * hop + hop // 2,
            win + (7 * F // 2 - 1) * hop + hop // 3]


class FbankArena(Arena):
    def fmodel(self, i, w, M, shape, **kw):
        it = self.items[i]
        ch, s = fc.clip_stream(it["lanes"], it["step"], it["skip"])
        return ch, fc.model(s, w, M, shape, **kw)


class FbankDevice(Device):
    def export(self, idx, step, w, M, shape, host=False, **kw):
        """-> the result with "feats": per clip [T][n_mels]; every float outside the features must still be the canary"""
        a = self.arena
        _, n_fft, hop, n_mels = shape
        args = (self.d_src, a.pcm16, a.n_lanes, a.stride, a.n_samples, a.rows[idx], w, M)
        kw = dict(dict(n_fft=n_fft, step=step, skips=a.skips(idx), hop=hop, scale=1.0, preemph=float(fc.PREEMPH), floor=float(fc.FLOOR)), **kw)
        if host:
            res = self.ctx.clips_export_fbank(*args, **kw)
            out = res["out"]
        else:
            self.fill()
            res = self.ctx.clips_export_fbank(*args, d_out=self.d_out, out_capacity=self.cap, **kw)
            out = self.ctx.to_host(np.zeros(self.cap + SLACK, np.float32), self.d_out)
            touched = np.zeros(self.cap + SLACK, bool)
            for T, o in zip(res["n_frames"].astype(np.int64), res["offsets"].astype(np.int64)):
                touched[o:o + T * n_mels] = True
            assert out[~touched].tobytes() == np.full(int((~touched).sum()), CANARY, np.float32).tobytes(), "a canary outside the features changed"
        res["feats"] = [out[o:o + T * n_mels].reshape(T, n_mels).copy() for T, o in zip(res["n_frames"].astype(np.int64), res["offsets"].astype(np.int64))]
        return res


def plan_total(fv, arena, idx, step, shape):
    lens = arena.rows[idx, 3] - arena.rows[idx, 2]
    return fv.clips_plan_fbank(lens, arena.skips(idx), step, shape[0], shape[2], shape[3])[2]


def check_against_model(arena, idx, res, w, M, shape, what, **kw):
    win, _, hop, _ = shape
    worst = 0.0
    for j, i in enumerate(idx):
        ch, (ref, U) = arena.fmodel(i, w, M, shape, **kw)
        assert int(res["best_channel"][j]) == ch == arena.items[i]["pick"], (what, i)
        assert int(res["n_frames"][j]) == ref.shape[0] == fc.n_frames(arena.items[i]["L"], win, hop), (what, i)
        got = res["feats"][j]
        assert np.isfinite(got).all(), (what, i)
        worst = max(worst, fc.distance(got, ref, U))
    print(f"{what}: worst distance {worst:.3f} units (tolerance {fc.TOL:.3f})")
    assert worst <= fc.TOL, (what, worst)


def means_f32(feats, F):
    """the stated order in numpy float32: within a tile of F frames over ascending t onto 0, the tiles' sums in tile order onto
    0, one division by f32(T)"""
    T, n_mels = feats.shape
    total = np.zeros(n_mels, np.float32)
    for t0 in range(0, T, F):
        s = np.zeros(n_mels, np.float32)
        for t in range(t0, min(t0 + F, T)):
            s = s + feats[t]
        total = total + s
    mean = total / np.float32(T)
    assert mean.dtype == np.float32
    return mean


# ------------------------------------------------------------------ every shape, at steps 1 and 3
@pytest.mark.parametrize("shape", fc.SHAPES, ids=SHAPE_IDS)
def test_shapes_against_the_model(fv, gpu_ctx, shape):
    win, n_fft, hop, n_mels = shape
    w, M = fc.window_for(shape), fc.matrix_for(shape)
    scale = fc.SCALES[fc.SHAPES.index(shape) % 2]
    ar = FbankArena(False, seed=win)
    for k, L in enumerate(clip_lengths(shape)):
        ar.add(L, 1, 0, C_=1 + k % 2, pick=k % 2, align=k % 4, signal=fc.mc.SIGNALS[k % len(fc.mc.SIGNALS)])
        ar.add(L, 3, k % 3, C_=1, align=(k + 1) % 4, signal=fc.mc.SIGNALS[(k + 3) % len(fc.mc.SIGNALS)], nan_between=True)
    ar.build()
    idx1, idx3 = list(range(0, len(ar.items), 2)), list(range(1, len(ar.items), 2))
    dev = FbankDevice(gpu_ctx, ar, plan_total(fv, ar, idx1, 1, shape) + plan_total(fv, ar, idx3, 3, shape))
    try:
        for idx, step in ((idx1, 1), (idx3, 3)):
            gpu_ctx.enable_timing(True)
            gpu_ctx.kernel_times()
            res = dev.export(idx, step, w, M, shape, scale=scale)
            names = list(gpu_ctx.kernel_times())
            gpu_ctx.enable_timing(False)
            assert names == TIMED, names
            check_against_model(ar, idx, res, w, M, shape, f"{SHAPE_IDS[fc.SHAPES.index(shape)]} step {step} x{scale:g}", scale=scale)
    finally:
        dev.close()


# ------------------------------------------------------------------ steps, skips, alignments, formats, channels
@pytest.fixture(scope="module", params=[False, True], ids=["from-f32", "from-pcm16"])
def steps_case(request, fv, gpu_ctx):
    """shape 400/512/160/80: steps 1, 3 and 16 with every skip, a clip start at each address modulo 16 bytes, one, two and five
    channels with the quietest in every position"""
    pcm16 = request.param
    ar = FbankArena(pcm16, seed=3)
    chans = [(1, 0), (2, 0), (2, 1)] + [(5, p) for p in range(5)]
    per16 = 8 if pcm16 else 4
    groups, k = {}, 0
    for step in (1, 3, 16):
        groups[step] = []
        for skip in range(step):
            for r in range(per16 if step < 16 else 1):
                C_, p = chans[k % len(chans)]
                L = 400 + 160 * (k % 3) + k % 7
                groups[step].append(ar.add(L, step, skip, C_=C_, pick=p, align=(k if step == 16 else r), signal=fc.mc.SIGNALS[k % 4]))
                k += 1
    ar.build()
    shape = fc.SHAPES[0]
    dev = FbankDevice(gpu_ctx, ar, max(plan_total(fv, ar, groups[s], s, shape) for s in groups))
    yield ar, dev, groups
    dev.close()


def test_steps_skips_alignments_formats_channels(gpu_ctx, steps_case):
    ar, dev, groups = steps_case
    shape = fc.SHAPES[0]
    w, M = fc.povey(400), fc.matrix_for(shape)
    for step, idx in groups.items():
        res = dev.export(idx, step, w, M, shape, scale=32768.0)
        check_against_model(ar, idx, res, w, M, shape, f"pcm16={ar.pcm16} step {step}", scale=32768.0)
        # the pick reports are fvad_clips_export's, bit for bit
        full = gpu_ctx.clips_export(dev.d_src, ar.pcm16, ar.n_lanes, ar.stride, ar.n_samples, ar.rows[idx])
        for f in ("best_channel", "best_rms", "runner_up_rms"):
            assert res[f].tobytes() == full[f].tobytes(), (step, f)


# ------------------------------------------------------------------ the conditioning's switches
@pytest.mark.parametrize("remove_dc,preemph", [(True, 0.97), (False, 0.97), (True, 0.0), (False, 0.0), (True, 1.0), (False, 1.0)])
def test_remove_dc_and_preemph_on_and_off(fv, gpu_ctx, remove_dc, preemph):
    for shape in (fc.SHAPES[0], fc.SHAPES[4]):
        win, n_fft, hop, n_mels = shape
        w, M = fc.window_for(shape), fc.matrix_for(shape)
        ar = FbankArena(False, seed=17)
        for k, name in enumerate(("noise0.3", "tone+noise", "noise0.01+dc0.1", "dc")):
            L = win + (3 + k) * hop + k
            if name == "noise0.01+dc0.1":   # (not one of the arena's own signals: placed by hand)
                i = ar.add(L, 3, k % 3, C_=1, align=k, signal="dc", nan_between=True)
                s = fc.signal(name, L, np.random.default_rng(5))
                ar.items[i]["lanes"][0][ar.items[i]["skip"]::3] = s
            else:
                ar.add(L, 3, k % 3, C_=1, align=k, signal=name, nan_between=True)
        ar.build()
        idx = list(range(len(ar.items)))
        dev = FbankDevice(gpu_ctx, ar, plan_total(fv, ar, idx, 3, shape))
        try:
            kw = dict(scale=32768.0, preemph=preemph, remove_dc=remove_dc)
            res = dev.export(idx, 3, w, M, shape, **kw)
            check_against_model(ar, idx, res, w, M, shape, f"{win}: remove_dc={remove_dc} preemph={preemph}", **kw)
        finally:
            dev.close()


# ------------------------------------------------------------------ invariants, bit for bit
@pytest.mark.parametrize("shape", [fc.SHAPES[0], fc.SHAPES[4]], ids=["400", "5"])
def test_invariants(gpu_ctx, shape):
    win, n_fft, hop, n_mels = shape
    w, M = fc.window_for(shape), fc.matrix_for(shape)
    step, k_shift = 3, 5
    ar = FbankArena(False, seed=9)
    base = ar.add(win + 75 * hop + 7, step, 1, C_=2, pick=1, align=1, signal="tone+noise")
    for L in clip_lengths(shape)[:6]:
        ar.add(L, step, L % 3, C_=1, align=L % 4, signal="noise0.3")
    ar.build()
    # the first clip again without its first k_shift hop step samples: the same lanes, a later start
    l0, C_, a, b = (int(v) for v in ar.rows[base])
    rows = np.concatenate([ar.rows, [[l0, C_, a + k_shift * hop * step, b]]]).astype(np.uint64)
    skips = np.concatenate([ar.skips(), [ar.items[base]["skip"]]]).astype(np.uint32)
    n = len(rows)
    ctx = gpu_ctx
    cap = 2 * sum(int(-(-(int(r[3] - r[2])) // step) // hop + 1) * n_mels + 4 for r in rows)
    d_src = ctx.device_alloc(ar.host.nbytes)
    ctx.to_device(d_src, np.ascontiguousarray(ar.host))
    d_out = ctx.device_alloc(cap * 4 + 64)

    def run(idx, host=False, off=0, cmn=False):
        kw = dict(n_fft=n_fft, step=step, skips=skips[idx], hop=hop, cmn=cmn)
        if host:
            res = ctx.clips_export_fbank(d_src, False, ar.n_lanes, ar.stride, ar.n_samples, rows[idx], w, M, **kw)
            out = res["out"]
        else:
            ctx.to_device(d_out, np.full(cap + 16, CANARY, np.float32))
            res = ctx.clips_export_fbank(d_src, False, ar.n_lanes, ar.stride, ar.n_samples, rows[idx], w, M, d_out=d_out + 16 * off, out_capacity=cap, **kw)
            out = ctx.to_host(np.zeros(cap + 16, np.float32), d_out)[4 * off:]
        return [out[o:o + T * n_mels].reshape(T, n_mels).copy() for T, o in zip(res["n_frames"].astype(np.int64), res["offsets"].astype(np.int64))], res

    try:
        every = list(range(n))
        feats, res = run(every)
        again, res2 = run(every)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(feats, again)) and res["means"].tobytes() == res2["means"].tobytes(), "two runs differ"
        rev, rr = run(every[::-1], off=1)   # reversed order, the output 16 bytes further on
        assert all(x.tobytes() == y.tobytes() for x, y in zip(feats, rev[::-1])), "the clip order changes a feature"
        assert rr["means"][::-1].tobytes() == res["means"].tobytes()
        for i in (0, 3, n - 1):
            alone, r1 = run([i])
            assert alone[0].tobytes() == feats[i].tobytes() and r1["means"][0].tobytes() == res["means"][i].tobytes(), ("a clip alone differs", i)
        hosted, rh = run(every, host=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(feats, hosted)), "the host form differs"
        for f in ("best_channel", "best_rms", "runner_up_rms", "n_frames", "means", "offsets"):
            assert rh[f].tobytes() == res[f].tobytes(), f
        # no reflection: EVERY frame of the shortened clip is frame t + k_shift of the full one, whatever tile it lands in
        full, short = feats[base], feats[n - 1]
        assert len(short) == len(full) - k_shift and len(short) > 2 * fc.tile_frames(win, hop)
        assert short.tobytes() == full[k_shift:].tobytes(), "a frame depends on where its tile starts"
        # means and cmn: numpy float32 in the stated order, bit for bit
        F = fc.tile_frames(win, hop)
        subbed, rc = run(every, cmn=True)
        assert rc["means"].tobytes() == res["means"].tobytes(), "cmn changes the means"
        for i in every:
            mean = means_f32(feats[i], F)
            assert res["means"][i].tobytes() == mean.tobytes(), ("means", i)
            assert subbed[i].tobytes() == (feats[i] - mean).tobytes(), ("cmn", i)
        ctx.enable_timing(True)
        ctx.kernel_times()
        run([0], cmn=True)
        names = list(ctx.kernel_times())
        ctx.enable_timing(False)
        assert names == TIMED + ["clip_fbank_sub"], names
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_out)


# ------------------------------------------------------------------ silence
@pytest.mark.parametrize("pcm16", [False, True])
def test_digital_silence_is_exactly_ln_of_the_floor(gpu_ctx, pcm16):
    shape = fc.SHAPES[0]
    w, M = fc.povey(400), fc.matrix_for(shape)
    n = 3 * 2000
    host = np.zeros((1, n), np.int16 if pcm16 else np.float32)
    rows = np.array([[0, 1, 1, n - 2]], np.uint64)
    d_src = gpu_ctx.device_alloc(host.nbytes)
    gpu_ctx.to_device(d_src, host)
    try:
        for floor in (float(fc.FLOOR), 1e-10, 2.5):
            res = gpu_ctx.clips_export_fbank(d_src, pcm16, 1, n, n, rows, w, M, step=3, skips=[1], floor=floor)
            want = np.float32(np.log(np.float64(np.float32(floor))))
            T = int(res["n_frames"][0])
            assert T == 1 + (1999 - 400) // 160 and res["out"][:T * 80].tobytes() == np.full(T * 80, want, np.float32).tobytes(), floor
    finally:
        gpu_ctx.device_free(d_src)


# ------------------------------------------------------------------ errors: every rule of the check, all canaries intact
def test_errors_come_back_before_any_launch(fv, gpu_ctx, steps_case):
    ar, dev, groups = steps_case
    shape = fc.SHAPES[0]
    w, M = fc.povey(400), fc.matrix_for(shape)
    idx = groups[3][:3]
    rows, skips = ar.rows[idx], ar.skips(idx)
    total = fv.clips_plan_fbank(rows[:, 3] - rows[:, 2], skips, 3, 400, 160, 80)[2]
    host_out = np.full(total + 8, CANARY, np.float32)
    bad_w, bad_m = w.copy(), M.copy()
    bad_w[0], bad_m[3, 7] = np.nan, np.inf

    def raw(host=False, d_src="own", src_format=None, n_lanes=None, stride=None, n_samples=None, rows=rows, out_format=0, out="own", cap=None,
            step=3, skips=skips, win=400, n_fft=512, hop=160, window=w, n_mels=80, matrix=M, scale=32768.0, preemph=0.97, remove_dc=1,
            floor=float(fc.FLOOR), cmn=0):
        r = np.ascontiguousarray(np.asarray(rows, np.uint64).reshape(-1, 4))
        k = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32))
        fn = fv.lib().fvad_clips_export_fbank if host else fv.lib().fvad_clips_export_fbank_device
        o = (host_out.ctypes.data if host else dev.d_out) if out == "own" else out
        return fn(gpu_ctx.h, fv.vp(dev.d_src if d_src == "own" else d_src), int(ar.pcm16) if src_format is None else src_format,
                  ar.n_lanes if n_lanes is None else n_lanes, ar.stride if stride is None else stride, ar.n_samples if n_samples is None else n_samples,
                  r.ctypes.data_as(C.POINTER(C.c_uint64)), len(r), out_format, fv.vp(o), (total if host else dev.cap) if cap is None else cap, None, None, None, None,
                  step, None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint32)), win, n_fft, hop, fv.fptr(window), n_mels, fv.fptr(matrix), scale,
                  preemph, remove_dc, floor, cmn, None, None)

    short = rows.copy()
    short[0, 3] = short[0, 2] + 3 * 399
    past = rows.copy()
    past[1, 0] = ar.n_lanes
    cases = [(dict(d_src=0), INVALID), (dict(out=0), INVALID), (dict(window=None), INVALID), (dict(matrix=None), INVALID), (dict(src_format=5), INVALID),
             (dict(out_format=1), INVALID), (dict(d_src=dev.d_src + 1), INVALID), (dict(stride=ar.n_samples - 1), INVALID),
             (dict(rows=[[0, 1, 9, 9]]), INVALID), (dict(rows=[[0, 0, 9, 4000]], skips=[0]), INVALID), (dict(step=0), INVALID), (dict(step=17), INVALID),
             (dict(n_fft=2), INVALID), (dict(n_fft=2050), INVALID), (dict(n_fft=511), INVALID), (dict(n_fft=398), INVALID), (dict(win=1), INVALID),
             (dict(hop=0), INVALID), (dict(hop=401), INVALID), (dict(n_mels=0), INVALID), (dict(n_mels=129), INVALID), (dict(skips=[3, 0, 0]), INVALID),
             (dict(rows=short), INVALID), (dict(window=bad_w), INVALID), (dict(matrix=bad_m), INVALID), (dict(scale=0.0), INVALID),
             (dict(scale=float("inf")), INVALID), (dict(preemph=1.5), INVALID), (dict(preemph=float("nan")), INVALID), (dict(remove_dc=2), INVALID),
             (dict(floor=0.0), INVALID), (dict(floor=float("nan")), INVALID), (dict(cmn=2), INVALID),
             (dict(n_samples=int(rows[:, 3].max()) - 1), OUT_OF_RANGE), (dict(rows=past), OUT_OF_RANGE), (dict(cap=total - 1), TOO_SMALL)]
    dev.fill()
    gpu_ctx.enable_timing(True)
    gpu_ctx.kernel_times()
    try:
        for kw, want in cases:
            for host in (False, True):
                assert raw(host=host, **kw) == want, (kw, host)
        assert raw(out=dev.d_out + 4) == INVALID   # the device output must be 16-byte aligned
        assert list(gpu_ctx.kernel_times()) == [], "a refused call launched a kernel"
    finally:
        gpu_ctx.enable_timing(False)
    assert dev.canaries_intact() and host_out.tobytes() == np.full(total + 8, CANARY, np.float32).tobytes()
    assert raw(rows=np.zeros((0, 4), np.uint64), skips=None) == 0 and dev.canaries_intact()   # no clips: nothing happens
    assert raw() == 0 and not dev.canaries_intact()


# ------------------------------------------------------------------ the log-mel export beside it
def test_the_mel_export_is_untouched_by_a_fbank_call(gpu_ctx, steps_case):
    ar, dev, groups = steps_case
    idx = groups[3]
    wm, Mm = fc.mc.hann(400), fc.mc.matrix_for(fc.mc.SHAPES[0])
    long_enough = [i for i in idx if ar.items[i]["L"] >= 201]
    args = (dev.d_src, ar.pcm16, ar.n_lanes, ar.stride, ar.n_samples, ar.rows[long_enough], wm, Mm)
    before = gpu_ctx.clips_export_mel(*args, step=3, skips=ar.skips(long_enough), hop=160, norm=(8.0, 4.0, 0.25))
    dev.export(idx, 3, fc.povey(400), fc.matrix_for(fc.SHAPES[0]), fc.SHAPES[0], cmn=True)
    after = gpu_ctx.clips_export_mel(*args, step=3, skips=ar.skips(long_enough), hop=160, norm=(8.0, 4.0, 0.25))
    for f in ("out", "feat_max", "n_frames", "offsets", "best_channel", "best_rms", "runner_up_rms"):
        assert before[f].tobytes() == after[f].tobytes(), f


# ------------------------------------------------------------------ the two families taking turns on one context
@pytest.mark.parametrize("mel_shape,shape", [((8, 4, 3), (6, 8, 4, 3)), ((400, 160, 80), (400, 512, 160, 80))], ids=["8", "400+512"])
def test_the_families_take_turns_on_one_context(fv, mel_shape, shape):
    """mel, fbank (cmn on), mel (norm on), fbank (cmn off), mel on one context -- the first pair transforms at the same n_fft and
    shares the context's cached tables, the second is the 400-point form beside the generic 512 -- each call byte for byte the same
    call made first on a context of its own: features, n_frames, feat_max / means and offsets.  Clips of L = win,
    win + 5 hop + 1 and 33 frames, from f32 and from PCM16 lanes, at step 1 and step 3"""
    win, n_fft, hop, n_mels = shape
    assert mel_shape[1:] == (hop, n_mels)
    wm, Mm = fc.mc.hann(mel_shape[0]), fc.mc.matrix_for(mel_shape)
    wf, Mf = fc.window_for(shape), fc.matrix_for(shape)
    arenas = []
    for pcm16 in (False, True):
        ar = FbankArena(pcm16, seed=21)
        for k, L in enumerate((win, win + 5 * hop + 1, win + 32 * hop)):
            ar.add(L, 1, 0, C_=1 + k % 2, pick=k % 2, align=k, signal=fc.mc.SIGNALS[k])
            ar.add(L, 3, k % 3, C_=1, align=k + 1, signal=fc.mc.SIGNALS[k + 3])
        arenas.append(ar.build())
    cap = sum((it["L"] // hop + 2) * n_mels + 4 for it in arenas[0].items)

    def call(kind, ctx):
        got = []
        for ar in arenas:
            dev = FbankDevice(ctx, ar, cap)
            try:
                for idx, step in ((list(range(0, len(ar.items), 2)), 1), (list(range(1, len(ar.items), 2)), 3)):
                    if kind.startswith("mel"):
                        r, own = Device.export(dev, idx, step, wm, Mm, hop, norm=(8.0, 4.0, 0.25) if kind == "mel+norm" else None), "feat_max"
                        assert [int(t) for t in r["n_frames"]] == [ar.items[i]["L"] // hop for i in idx]
                    else:
                        r, own = dev.export(idx, step, wf, Mf, shape, scale=32768.0, cmn=kind == "fbank+cmn"), "means"
                        assert [int(t) for t in r["n_frames"]] == [fc.n_frames(ar.items[i]["L"], win, hop) for i in idx]
                    got.append([f.tobytes() for f in r["feats"]] + [r[k].tobytes() for k in ("n_frames", own, "offsets")])
            finally:
                dev.close()
        return got

    first = {}
    for kind in ("mel", "fbank+cmn", "mel+norm", "fbank"):
        ctx = fv.Context(0)
        try:
            first[kind] = call(kind, ctx)
        finally:
            ctx.close()
    assert first["mel"] != first["mel+norm"] and first["fbank"] != first["fbank+cmn"]
    ctx = fv.Context(0)
    try:
        for turn, kind in enumerate(("mel", "fbank+cmn", "mel+norm", "fbank", "mel")):
            assert call(kind, ctx) == first[kind], (turn, kind)
    finally:
        ctx.close()
