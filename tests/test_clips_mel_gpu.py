"""The log-mel clip export on the GPU (fvad_clips_export_mel(_device), csrc/kernels_clips_mel.hip) against clip_mel_cases.py's
float64 model, in its units, on exactly the samples the kernel is given.

An `Arena` is a set of lanes filled with NaN (f32) or a loud sentinel (PCM16) in which every clip is placed with its own
channel count, start alignment, step and skip; its kept samples carry the signal, the samples between them NaN (one-channel
f32 clips: NaN on every off-stride sample proves that none reaches a feature) or independent noise (the clips whose channel is
picked by RMS, which is taken over EVERY sample).  Every device export goes into a canary-filled buffer with canaries in the
slot padding and behind the output.  Shapes are the smallest at which the kernels take another path: clips of exactly
n_fft / 2 + 1 samples, of 7, 8 and 9 frames (a wavefront of the 400-point form seats eight), of hop q and hop q +- 1 samples,
and one of three and a half tiles of frames."""
import ctypes as C

import numpy as np
import pytest

import clip_mel_cases as mc

pytestmark = pytest.mark.gpu

INVALID, OUT_OF_RANGE, TOO_SMALL = -100, -6, -106
CANARY = np.frombuffer(np.uint32(0x7FC0BEEF).tobytes(), np.float32)[0]
SENTINEL = np.int16(0x7A5A)
SLACK = 64
FORMS = [(mc.SHAPES[0], "auto"), (mc.SHAPES[0], "generic")] + [(s, "auto") for s in mc.SHAPES[1:]]
FORM_IDS = ["/".join(map(str, s)) + "-" + f for s, f in FORMS]


def clip_lengths(shape):
    """stream lengths L: exactly pad + 1; 7, 8 and 9 frames; hop q and hop q +- 1; three and a half tiles of frames"""
    n_fft, hop, _ = shape
    pad1, F = n_fft // 2 + 1, mc.tile_frames(n_fft, hop)
    q = max(8, -(-pad1 // hop) + 1)
    return [pad1, max(7 * hop, pad1), q * hop, q * hop - 1, q * hop + 1, max(9 * hop + hop // 2, pad1), (7 * F // 2) * hop + hop // 3]


class Arena:
    """lanes [n_lanes][stride] of one format and the clips placed in them"""

    def __init__(self, pcm16, seed=1):
        self.pcm16, self.rng = pcm16, np.random.default_rng(seed)
        self.items, self.at = [], 5   # (lane0, C, a, b, step, skip, pick)

    def add(self, L, step, skip, C_=1, pick=0, align=0, signal="noise0.3", nan_between=False):
        """a clip of C_ channels whose channel `pick` is the quietest; its first sample sits at `align` (mod 16 bytes, in samples);
        nan_between (f32, one channel): NaN on every off-stride sample"""
        per16 = 8 if self.pcm16 else 4
        a = self.at + (align - self.at) % per16
        n = skip + (L - 1) * step + 1 + int(self.rng.integers(0, step))
        s = mc.signal(signal, L, self.rng)
        scale = max(float(np.abs(s).max()), 1e-3)
        lanes = []
        for c in range(C_):
            g = 1.0 if c == pick else 2.0 + 0.5 * c
            x = (g * 0.7 * scale * self.rng.standard_normal(n)).astype(np.float32)
            if c == pick:
                if nan_between:
                    x[:] = np.nan
                x[skip::step] = s
            lanes.append(x)
        self.items.append(dict(C=C_, a=a, b=a + n, step=step, skip=skip, pick=pick, lanes=np.stack(lanes), L=L))
        self.at = a + n + 3
        return len(self.items) - 1

    def build(self):
        self.n_lanes = max(i["C"] for i in self.items) + 1
        self.n_samples = self.at + 7
        self.stride = self.n_samples + 5
        fill = SENTINEL if self.pcm16 else np.nan
        self.host = np.full((self.n_lanes, self.stride), fill, np.int16 if self.pcm16 else np.float32)
        rows = []
        for k, it in enumerate(self.items):
            l0 = k % (self.n_lanes - it["C"] + 1)
            x = it["lanes"]
            if self.pcm16:
                x = np.clip(np.rint(np.nan_to_num(x) * 8192.0), -32768, 32767).astype(np.int16)
                it["lanes"] = x
            self.host[l0:l0 + it["C"], it["a"]:it["b"]] = x
            rows.append((l0, it["C"], it["a"], it["b"]))
        self.rows = np.array(rows, np.uint64)
        return self

    def skips(self, idx=None):
        idx = range(len(self.items)) if idx is None else idx
        return np.array([self.items[i]["skip"] for i in idx], np.uint32)

    def model(self, i, w, M, hop, floor=mc.FLOOR):
        it = self.items[i]
        ch, s = mc.clip_stream(it["lanes"], it["step"], it["skip"])
        return ch, mc.model(s, w, M, hop, floor)


class Device:
    def __init__(self, ctx, arena, cap):
        self.ctx, self.arena, self.cap = ctx, arena, cap
        self.d_src = ctx.device_alloc(arena.host.nbytes)
        ctx.to_device(self.d_src, np.ascontiguousarray(arena.host))
        self.d_out = ctx.device_alloc((cap + SLACK) * 4)

    def close(self):
        # the sources are as they were
        back = self.ctx.to_host(np.zeros_like(self.arena.host), self.d_src)
        self.ctx.device_free(self.d_src)
        self.ctx.device_free(self.d_out)
        assert back.tobytes() == self.arena.host.tobytes()

    def fill(self):
        self.ctx.to_device(self.d_out, np.full(self.cap + SLACK, CANARY, np.float32))

    def canaries_intact(self):
        out = self.ctx.to_host(np.zeros(self.cap + SLACK, np.float32), self.d_out)
        return out.tobytes() == np.full(self.cap + SLACK, CANARY, np.float32).tobytes()

    def export(self, idx, step, w, M, hop, host=False, **kw):
        """-> the result with "feats": per clip [T][n_mels]; every float outside the features must still be the canary"""
        a = self.arena
        n_mels = M.shape[0]
        args = (self.d_src, a.pcm16, a.n_lanes, a.stride, a.n_samples, a.rows[idx], w, M)
        if host:
            res = self.ctx.clips_export_mel(*args, step=step, skips=a.skips(idx), hop=hop, **kw)
            out = res["out"]
        else:
            self.fill()
            res = self.ctx.clips_export_mel(*args, step=step, skips=a.skips(idx), hop=hop, d_out=self.d_out, out_capacity=self.cap, **kw)
            out = self.ctx.to_host(np.zeros(self.cap + SLACK, np.float32), self.d_out)
            touched = np.zeros(self.cap + SLACK, bool)
            for T, o in zip(res["n_frames"].astype(np.int64), res["offsets"].astype(np.int64)):
                touched[o:o + T * n_mels] = True
            assert out[~touched].tobytes() == np.full(int((~touched).sum()), CANARY, np.float32).tobytes(), "a canary outside the features changed"
        res["feats"] = [out[o:o + T * n_mels].reshape(T, n_mels).copy() for T, o in zip(res["n_frames"].astype(np.int64), res["offsets"].astype(np.int64))]
        return res


def with_form(ctx, form):
    ctx.set_option("clip_mel_fft", None if form == "auto" else form)


def check_against_model(arena, idx, res, w, M, hop, what, floor=mc.FLOOR):
    worst = 0.0
    for j, i in enumerate(idx):
        ch, (ref, U) = arena.model(i, w, M, hop, floor)
        assert int(res["best_channel"][j]) == ch == arena.items[i]["pick"], (what, i)
        assert int(res["n_frames"][j]) == ref.shape[0] == arena.items[i]["L"] // hop, (what, i)
        got = res["feats"][j]
        assert np.isfinite(got).all(), (what, i)
        d = mc.distance(got, ref, U)
        worst = max(worst, d)
        assert np.float32(res["feat_max"][j]).tobytes() == got.max().tobytes(), (what, i, "feat_max")
    print(f"{what}: worst distance {worst:.3f} units (tolerance {mc.TOL:.3f})")
    assert worst <= mc.TOL, (what, worst)


# ------------------------------------------------------------------ every shape and both transforms, at steps 1 and 3
@pytest.mark.parametrize("shape,form", FORMS, ids=FORM_IDS)
def test_shapes_against_the_model(gpu_ctx, shape, form):
    n_fft, hop, n_mels = shape
    w, M = mc.hann(n_fft), mc.matrix_for(shape)
    ar = Arena(False, seed=n_fft)
    signals = mc.SIGNALS
    for k, L in enumerate(clip_lengths(shape)):
        ar.add(L, 1, 0, C_=1 + k % 2, pick=k % 2, align=k % 4, signal=signals[k % len(signals)])
        ar.add(L, 3, k % 3, C_=1, align=(k + 1) % 4, signal=signals[(k + 3) % len(signals)], nan_between=True)
    ar.build()
    idx1, idx3 = list(range(0, len(ar.items), 2)), list(range(1, len(ar.items), 2))
    dev = Device(gpu_ctx, ar, fv_total(gpu_ctx, ar, idx1, 1, shape) + fv_total(gpu_ctx, ar, idx3, 3, shape))
    with_form(gpu_ctx, form)
    try:
        for idx, step in ((idx1, 1), (idx3, 3)):
            gpu_ctx.enable_timing(True)
            gpu_ctx.kernel_times()
            res = dev.export(idx, step, w, M, hop)
            names = list(gpu_ctx.kernel_times())
            gpu_ctx.enable_timing(False)
            assert names == ["clip_rms", "clip_pick", "clip_mel400" if (n_fft == 400 and form == "auto") else "clip_mel", "clip_mel_max"], names
            check_against_model(ar, idx, res, w, M, hop, f"{FORM_IDS[FORMS.index((shape, form))]} step {step}")
    finally:
        with_form(gpu_ctx, "auto")
        dev.close()


def fv_total(ctx, arena, idx, step, shape):
    from conftest import load_package
    fv = load_package().binding
    lens = arena.rows[idx, 3] - arena.rows[idx, 2]
    return fv.clips_plan_mel(lens, arena.skips(idx), step, *shape)[2]


# ------------------------------------------------------------------ steps, skips, alignments, formats, channels
@pytest.fixture(scope="module", params=[False, True], ids=["from-f32", "from-pcm16"])
def steps_case(request, gpu_ctx):
    """shape 400/160/80: steps 1, 3 and 16 with every skip, a clip start at each address modulo 16 bytes, one, two and five
    channels with the quietest in every position"""
    pcm16 = request.param
    ar = Arena(pcm16, seed=3)
    chans = [(1, 0), (2, 0), (2, 1)] + [(5, p) for p in range(5)]
    per16 = 8 if pcm16 else 4
    groups, k = {}, 0
    for step in (1, 3, 16):
        groups[step] = []
        for skip in range(step):
            for r in range(per16 if step < 16 else 1):
                C_, p = chans[k % len(chans)]
                L = 201 + 160 * (k % 3) + k % 7
                groups[step].append(ar.add(L, step, skip, C_=C_, pick=p, align=(k if step == 16 else r), signal=mc.SIGNALS[k % 4]))
                k += 1
    ar.build()
    shape = mc.SHAPES[0]
    dev = Device(gpu_ctx, ar, max(fv_total(gpu_ctx, ar, groups[s], s, shape) for s in groups))
    yield ar, dev, groups
    dev.close()


@pytest.mark.parametrize("form", ["auto", "generic"])
def test_steps_skips_alignments_formats_channels(gpu_ctx, steps_case, form):
    ar, dev, groups = steps_case
    shape = mc.SHAPES[0]
    w, M = mc.hann(400), mc.matrix_for(shape)
    with_form(gpu_ctx, form)
    try:
        for step, idx in groups.items():
            res = dev.export(idx, step, w, M, 160)
            check_against_model(ar, idx, res, w, M, 160, f"pcm16={ar.pcm16} {form} step {step}")
            # the pick reports are fvad_clips_export's, bit for bit
            full = gpu_ctx.clips_export(dev.d_src, ar.pcm16, ar.n_lanes, ar.stride, ar.n_samples, ar.rows[idx])
            for f in ("best_channel", "best_rms", "runner_up_rms"):
                assert res[f].tobytes() == full[f].tobytes(), (step, f)
    finally:
        with_form(gpu_ctx, "auto")


# ------------------------------------------------------------------ invariants, bit for bit
@pytest.mark.parametrize("shape,form", [(mc.SHAPES[0], "auto"), (mc.SHAPES[0], "generic"), (mc.SHAPES[4], "auto")], ids=["400-auto", "400-generic", "254"])
def test_invariants(gpu_ctx, shape, form):
    n_fft, hop, n_mels = shape
    w, M = mc.hann(n_fft), mc.matrix_for(shape)
    step, k_shift = 3, 5
    ar = Arena(False, seed=9)
    base = ar.add(75 * hop + 7, step, 1, C_=2, pick=1, align=1, signal="tone+noise")
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

    def run(idx, host=False, off=0):
        kw = dict(step=step, skips=skips[idx], hop=hop)
        if host:
            res = ctx.clips_export_mel(d_src, False, ar.n_lanes, ar.stride, ar.n_samples, rows[idx], w, M, **kw)
            out = res["out"]
        else:
            ctx.to_device(d_out, np.full(cap + 16, CANARY, np.float32))
            res = ctx.clips_export_mel(d_src, False, ar.n_lanes, ar.stride, ar.n_samples, rows[idx], w, M, d_out=d_out + 16 * off, out_capacity=cap, **kw)
            out = ctx.to_host(np.zeros(cap + 16, np.float32), d_out)[4 * off:]
        return [out[o:o + T * n_mels].reshape(T, n_mels).copy() for T, o in zip(res["n_frames"].astype(np.int64), res["offsets"].astype(np.int64))], res

    with_form(ctx, form)
    try:
        every = list(range(n))
        feats, res = run(every)
        again, res2 = run(every)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(feats, again)) and res["feat_max"].tobytes() == res2["feat_max"].tobytes(), "two runs differ"
        rev, _ = run(every[::-1], off=1)   # reversed order, the output 16 bytes further on
        assert all(x.tobytes() == y.tobytes() for x, y in zip(feats, rev[::-1])), "the clip order changes a feature"
        for i in (0, 3, n - 1):
            alone, r1 = run([i])
            assert alone[0].tobytes() == feats[i].tobytes() and r1["feat_max"][0].tobytes() == res["feat_max"][i].tobytes(), ("a clip alone differs", i)
        hosted, rh = run(every, host=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(feats, hosted)), "the host form differs"
        for f in ("best_channel", "best_rms", "runner_up_rms", "n_frames", "feat_max", "offsets"):
            assert rh[f].tobytes() == res[f].tobytes(), f
        # interior frames of the shortened clip are frames t + k_shift of the full one: those whose taps touch neither reflection
        full, short = feats[base], feats[n - 1]
        first = -(-(n_fft // 2) // hop)
        last = (len(short) * hop - n_fft // 2 - 1) // hop   # (the shortened clip ends where the full one does)
        assert last - first > mc.tile_frames(n_fft, hop), "the interior does not span a tile"
        assert short[first:last].tobytes() == full[first + k_shift:last + k_shift].tobytes(), "a frame depends on where its tile starts"
    finally:
        with_form(ctx, "auto")
        ctx.device_free(d_src)
        ctx.device_free(d_out)


# ------------------------------------------------------------------ normalisation, silence
def test_normalisation_is_the_numpy_float32_formula(gpu_ctx, steps_case):
    ar, dev, groups = steps_case
    w, M = mc.hann(400), mc.matrix_for(mc.SHAPES[0])
    idx = groups[3]
    raw = dev.export(idx, 3, w, M, 160)
    for norm in ((8.0, 4.0, 0.25), (3.5, -1.25, 0.1)):
        res = dev.export(idx, 3, w, M, 160, norm=norm)
        rng_, off, scale = (np.float32(v) for v in norm)
        assert res["feat_max"].tobytes() == raw["feat_max"].tobytes()
        for j in range(len(idx)):
            x = raw["feats"][j]
            want = (np.maximum(x, x.max() - rng_) + off) * scale
            assert want.dtype == np.float32 and res["feats"][j].tobytes() == want.tobytes(), (norm, j)
    gpu_ctx.enable_timing(True)
    gpu_ctx.kernel_times()
    dev.export(idx[:2], 3, w, M, 160, norm=(8.0, 4.0, 0.25))
    names = list(gpu_ctx.kernel_times())
    gpu_ctx.enable_timing(False)
    assert names[-1] == "clip_mel_norm" and names[-2] == "clip_mel_max", names


@pytest.mark.parametrize("form", ["auto", "generic"])
@pytest.mark.parametrize("pcm16", [False, True])
def test_digital_silence_is_exactly_log10_of_the_floor(gpu_ctx, form, pcm16):
    w, M = mc.hann(400), mc.matrix_for(mc.SHAPES[0])
    n = 3 * 2000
    host = np.zeros((1, n), np.int16 if pcm16 else np.float32)
    rows = np.array([[0, 1, 1, n - 2]], np.uint64)
    d_src = gpu_ctx.device_alloc(host.nbytes)
    gpu_ctx.to_device(d_src, host)
    with_form(gpu_ctx, form)
    try:
        for floor in (1e-10, 3e-7, 2.5):
            res = gpu_ctx.clips_export_mel(d_src, pcm16, 1, n, n, rows, w, M, step=3, skips=[1], hop=160, floor=floor)
            want = np.float32(np.log10(np.float64(np.float32(floor))))
            T = int(res["n_frames"][0])
            assert T == 1999 // 160 and res["out"][:T * 80].tobytes() == np.full(T * 80, want, np.float32).tobytes(), floor
            assert res["feat_max"][0].tobytes() == want.tobytes()
    finally:
        with_form(gpu_ctx, "auto")
        gpu_ctx.device_free(d_src)


# ------------------------------------------------------------------ errors: every rule of the check, all canaries intact
def test_errors_come_back_before_any_launch(fv, gpu_ctx, steps_case):
    ar, dev, groups = steps_case
    w, M = mc.hann(400), mc.matrix_for(mc.SHAPES[0])
    idx = groups[3][:3]
    rows, skips = ar.rows[idx], ar.skips(idx)
    total = fv.clips_plan_mel(rows[:, 3] - rows[:, 2], skips, 3, 400, 160, 80)[2]
    host_out = np.full(total + 8, CANARY, np.float32)
    bad_w, bad_m = w.copy(), M.copy()
    bad_w[0], bad_m[3, 7] = np.nan, np.inf
    norm_bad = np.array([8, np.inf, 0.25], np.float32)

    def raw(host=False, d_src="own", src_format=None, n_lanes=None, stride=None, n_samples=None, rows=rows, out_format=0, out="own", cap=None,
            step=3, skips=skips, n_fft=400, hop=160, window=w, n_mels=80, matrix=M, floor=1e-10, norm=None):
        r = np.ascontiguousarray(np.asarray(rows, np.uint64).reshape(-1, 4))
        k = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32))
        fn = fv.lib().fvad_clips_export_mel if host else fv.lib().fvad_clips_export_mel_device
        o = (host_out.ctypes.data if host else dev.d_out) if out == "own" else out
        return fn(gpu_ctx.h, fv.vp(dev.d_src if d_src == "own" else d_src), int(ar.pcm16) if src_format is None else src_format,
                  ar.n_lanes if n_lanes is None else n_lanes, ar.stride if stride is None else stride, ar.n_samples if n_samples is None else n_samples,
                  r.ctypes.data_as(C.POINTER(C.c_uint64)), len(r), out_format, fv.vp(o), (total if host else dev.cap) if cap is None else cap, None, None, None, None,
                  step, None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint32)), n_fft, hop, fv.fptr(window), n_mels, fv.fptr(matrix), floor,
                  fv.fptr(norm), None, None)

    short = rows.copy()
    short[0, 3] = short[0, 2] + 500
    past = rows.copy()
    past[1, 0] = ar.n_lanes
    cases = [(dict(d_src=0), INVALID), (dict(out=0), INVALID), (dict(window=None), INVALID), (dict(matrix=None), INVALID), (dict(src_format=5), INVALID),
             (dict(out_format=1), INVALID), (dict(d_src=dev.d_src + 1), INVALID), (dict(stride=ar.n_samples - 1), INVALID),
             (dict(rows=[[0, 1, 9, 9]]), INVALID), (dict(rows=[[0, 0, 9, 4000]], skips=[0]), INVALID), (dict(step=0), INVALID), (dict(step=17), INVALID),
             (dict(n_fft=2), INVALID), (dict(n_fft=2050), INVALID), (dict(n_fft=399), INVALID), (dict(hop=0), INVALID), (dict(hop=401), INVALID),
             (dict(n_mels=0), INVALID), (dict(n_mels=129), INVALID), (dict(skips=[3, 0, 0]), INVALID), (dict(rows=short), INVALID),
             (dict(window=bad_w), INVALID), (dict(matrix=bad_m), INVALID), (dict(floor=0.0), INVALID), (dict(floor=float("nan")), INVALID),
             (dict(norm=norm_bad), INVALID), (dict(n_samples=int(rows[:, 3].max()) - 1), OUT_OF_RANGE), (dict(rows=past), OUT_OF_RANGE),
             (dict(cap=total - 1), TOO_SMALL)]
    dev.fill()
    for kw, want in cases:
        for host in (False, True):
            assert raw(host=host, **kw) == want, (kw, host)
    assert raw(out=dev.d_out + 4) == INVALID   # the device output must be 16-byte aligned
    assert dev.canaries_intact() and host_out.tobytes() == np.full(total + 8, CANARY, np.float32).tobytes()
    assert raw(rows=np.zeros((0, 4), np.uint64), skips=None) == 0 and dev.canaries_intact()   # no clips: nothing happens
    assert raw() == 0 and not dev.canaries_intact()
    with pytest.raises(fv.FvadError):
        gpu_ctx.set_option("clip_mel_fft", "radix7")
