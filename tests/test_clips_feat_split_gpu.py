"""The split-source feature exports on the GPU (fvad_clips_export_split_mel*, fvad_clips_export_split_fbank*): every result
equal, bit for bit, to the contiguous export's over the same samples laid out contiguously on the same context, wherever the
seam is, and within the families' own tolerances of their float64 models (clip_mel_cases.TOL, clip_fbank_cases.TOL) on the
split model's stream (clip_feat_split_cases.py).

A `Layout` holds every clip twice: contiguous, and cut into a piece in buffer A and a piece in buffer B at piece offsets that
rotate through clip_split_cases.FEW_PAIRS.  Whatever is no clip sample is NaN (f32) or full scale (PCM16) in all three buffers,
one-channel clips carry the same on every off-stride sample, and every device export goes into a canary-filled buffer."""
import numpy as np
import pytest

import clip_fbank_cases as fc
import clip_feat_split_cases as sc
import clip_mel_cases as mc

pytestmark = pytest.mark.gpu

CANARY = np.frombuffer(np.uint32(0x7FC0BEEF).tobytes(), np.float32)[0]
SLACK = 64
REPORTS = ("n_frames", "offsets", "best_channel", "best_rms", "runner_up_rms")


class Family:
    """one family at one shape: how to call both forms, the float64 model and its tolerance"""

    def __init__(self, name, shape, form=None, scale=None):
        self.name, self.shape, self.form, self.scale = name, shape, form, scale
        if name == "mel":
            self.taps, self.hop, self.n_mels = shape
            self.n_fft, self.centred = self.taps, True
            self.w, self.M, self.tol, self.extra = mc.hann(self.taps), mc.matrix_for(shape), mc.TOL, "feat_max"
            self.min_L, self.floor = max(self.taps // 2 + 1, self.hop), mc.FLOOR
        else:
            self.taps, self.n_fft, self.hop, self.n_mels = shape
            self.centred = False
            self.w, self.M, self.tol, self.extra = fc.window_for(shape), fc.matrix_for(shape), fc.TOL, "means"
            self.min_L, self.floor = self.taps, fc.FLOOR
        self.tile_frames = mc.tile_frames(self.taps, self.hop)
        self.id = f"{name}-{'/'.join(map(str, shape))}" + (f"-{form}" if form else "")

    def L_of_frames(self, T, more=0):
        return max(T * self.hop + more if self.centred else (T - 1) * self.hop + self.taps + more, self.min_L)

    def n_frames(self, L):
        return L // self.hop if self.centred else 1 + (L - self.taps) // self.hop

    def kw(self, **kw):
        if self.name == "mel":
            return dict(hop=self.hop, floor=float(self.floor), **kw)
        return dict(n_fft=self.n_fft, hop=self.hop, scale=self.scale, floor=float(self.floor), **kw)

    def contiguous(self, ctx, d_src, lay, idx, step, **kw):
        f = ctx.clips_export_mel if self.name == "mel" else ctx.clips_export_fbank
        return f(d_src, lay.pcm16, lay.n_lanes, lay.stride, lay.n_samples, lay.rows[idx], self.w, self.M, step=step, skips=lay.skips(idx), **self.kw(**kw))

    def split(self, ctx, d_a, d_b, lay, idx, step, a=None, **kw):
        f = ctx.clips_export_split_mel if self.name == "mel" else ctx.clips_export_split_fbank
        return f(a or lay.a(d_a), lay.b(d_b), lay.pcm16, lay.split[idx], self.w, self.M, step=step, skips=lay.skips(idx), **self.kw(**kw))

    def model(self, stream):
        if self.name == "mel":
            return mc.model(stream, self.w, self.M, self.hop, self.floor)
        return fc.model(stream, self.w, self.M, self.shape, scale=self.scale, floor=self.floor)

    def label(self):
        return "clip_fbank" if self.name == "fbank" else "clip_mel400" if self.taps == 400 and self.form == "auto" else "clip_mel"


FAMILIES = [Family("mel", mc.SHAPES[0], "auto"), Family("mel", mc.SHAPES[0], "generic"), Family("mel", mc.SHAPES[2], "auto"),
            Family("fbank", fc.SHAPES[0], scale=32768.0), Family("fbank", fc.SHAPES[2], scale=32768.0)]
assert fc.window_for(fc.SHAPES[0]).tobytes() == fc.povey(400).tobytes() and fc.window_for(fc.SHAPES[2]).tobytes() == fc.hamming(6).tobytes()


class Device:
    def __init__(self, ctx, fam, lay, cap):
        self.ctx, self.fam, self.lay, self.cap = ctx, fam, lay, cap
        self.bufs = [(ctx.device_alloc(x.nbytes), np.ascontiguousarray(x)) for x in (lay.host, lay.A, lay.B)]
        for d, x in self.bufs:
            ctx.to_device(d, x)
        self.d_src, self.d_a, self.d_b = (d for d, _ in self.bufs)
        self.d_out = ctx.device_alloc((cap + SLACK) * 4)
        if fam.name == "mel":
            ctx.set_option("clip_mel_fft", None if fam.form == "auto" else fam.form)

    def close(self):
        self.ctx.set_option("clip_mel_fft", None)
        same = [self.ctx.to_host(np.zeros_like(x), d).tobytes() == x.tobytes() for d, x in self.bufs]
        for d, _ in self.bufs:
            self.ctx.device_free(d)
        self.ctx.device_free(self.d_out)
        assert all(same), "a source buffer changed"

    def fill(self):
        self.ctx.to_device(self.d_out, np.full(self.cap + SLACK, CANARY, np.float32))

    def canaries_intact(self):
        out = self.ctx.to_host(np.zeros(self.cap + SLACK, np.float32), self.d_out)
        return out.tobytes() == np.full(self.cap + SLACK, CANARY, np.float32).tobytes()

    def run(self, idx, step, split, host=False, off=0, **kw):
        """one export of clips idx -> the result with "feats": per clip [T][n_mels].  Device form: into the canary-filled buffer,
        `off` times 16 bytes in; every float outside the features must still be the canary"""
        fam, n_mels = self.fam, self.fam.n_mels
        call = (lambda **k: fam.split(self.ctx, self.d_a, self.d_b, self.lay, idx, step, **k)) if split else \
               (lambda **k: fam.contiguous(self.ctx, self.d_src, self.lay, idx, step, **k))
        if host:
            res = call(**kw)
            out = res["out"]
        else:
            self.fill()
            res = call(d_out=self.d_out + 16 * off, out_capacity=self.cap - 4 * off, **kw)
            out = self.ctx.to_host(np.zeros(self.cap + SLACK, np.float32), self.d_out)
            touched = np.zeros(self.cap + SLACK, bool)
            for T, o in zip(res["n_frames"].astype(np.int64), res["offsets"].astype(np.int64)):
                touched[4 * off + o:4 * off + o + T * n_mels] = True
            assert out[~touched].tobytes() == np.full(int((~touched).sum()), CANARY, np.float32).tobytes(), "a canary outside the features changed"
            out = out[4 * off:]
        res["feats"] = [out[o:o + T * n_mels].reshape(T, n_mels).copy() for T, o in zip(res["n_frames"].astype(np.int64), res["offsets"].astype(np.int64))]
        return res


def assert_same(got, want, fam, what):
    """a split call's results are the contiguous call's, bit for bit"""
    for f in REPORTS + (fam.extra,):
        assert got[f].tobytes() == want[f].tobytes(), (what, f)
    assert got["total"] == want["total"], what
    for j, (x, y) in enumerate(zip(got["feats"], want["feats"])):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, "the features of clip", j)


def assert_model(fam, lay, idx, res, what):
    worst = 0.0
    for j, i in enumerate(idx):
        ch, s = lay.stream(i)
        ref, U = fam.model(s)
        assert int(res["best_channel"][j]) == ch and int(res["n_frames"][j]) == ref.shape[0] == fam.n_frames(len(s)), (what, i)
        got = res["feats"][j]
        assert np.isfinite(got).all(), (what, i, "a canary reached a feature")
        worst = max(worst, mc.distance(got, ref, U))
    print(f"{what}: worst distance {worst:.3f} units (tolerance {fam.tol:.3f})")
    assert worst <= fam.tol, (what, worst)


def plan_total(fv, fam, lay, idx, step):
    lens = lay.rows[idx, 3] - lay.rows[idx, 2]
    plan = fv.clips_plan_mel if fam.name == "mel" else fv.clips_plan_fbank
    return plan(lens, lay.skips(idx), step, fam.taps, fam.hop, fam.n_mels)[2]


def seam_layout(fam, pcm16, seed):
    """-> (layout, {step: clip indices}): the whole seam table on a clip of three and a half tiles of frames (step 3), of exactly
    the shortest legal length (step 3, two channels) and of 33 frames (step 1); steps 1, 3 and 16 with every skip at one mid seam
    per residue, with one, two and five channels; one clip whose pick is decided only across the seam"""
    rng = np.random.default_rng(seed)
    lay, groups, k = sc.Layout(pcm16), {1: [], 3: [], 16: []}, 0

    def table(L, step, skip, C_, pick, signal):
        nonlocal k
        canaries = C_ == 1
        lanes = sc.clip_lanes(rng, L, step, skip, C_, pick, signal, pcm16, canaries)
        for a_len in sc.seams(lanes.shape[1], skip, step, fam.taps, fam.hop, fam.centred, fam.tile_frames):
            groups[step].append(lay.add(lanes, a_len, skip, step, off=sc.FEW_PAIRS[k % len(sc.FEW_PAIRS)]))
            k += 1

    F = fam.tile_frames
    table(fam.L_of_frames(7 * F // 2, fam.hop // 3), 3, 1, 1, 0, "noise0.3")
    table(fam.min_L, 3, 2, 2, 1, "tone+noise")
    table(fam.L_of_frames(33, 1), 1, 0, 1, 0, "noise0.3")
    chans = [(1, 0), (2, 1), (5, 3)]
    for step in (1, 3, 16):
        for skip in range(step):
            C_, pick = chans[k % 3]
            L = fam.L_of_frames(3 if step == 16 else 9, 3 + skip % 2)
            lanes = sc.clip_lanes(rng, L, step, skip, C_, pick, mc.SIGNALS[k % 4], pcm16, C_ == 1)
            m = L // 2
            for a_len in (m * step + skip - 1, m * step + skip, m * step + skip + 1):
                groups[step].append(lay.add(lanes, a_len, skip, step, off=sc.FEW_PAIRS[k % len(sc.FEW_PAIRS)]))
                k += 1
    n = 2 + (fam.L_of_frames(5, 2) - 1) * 3 + 1
    groups[3].append(lay.add(sc.seam_pick_lanes(rng, n, n // 2 + 1, pcm16), n // 2 + 1, 2, 3, off=(1, 3), seam_pick=True))
    return lay.build(), groups


@pytest.mark.parametrize("pcm16", [False, True], ids=["from-f32", "from-pcm16"])
@pytest.mark.parametrize("fam", FAMILIES, ids=[f.id for f in FAMILIES])
def test_every_seam_gives_the_contiguous_bits(fv, gpu_ctx, fam, pcm16):
    lay, groups = seam_layout(fam, pcm16, seed=fam.taps + int(pcm16))
    dev = Device(gpu_ctx, fam, lay, max(plan_total(fv, fam, lay, idx, step) for step, idx in groups.items()) + 8)
    try:
        for step, idx in groups.items():
            want = dev.run(idx, step, split=False)
            gpu_ctx.enable_timing(True)
            gpu_ctx.kernel_times()
            got = dev.run(idx, step, split=True)
            names = list(gpu_ctx.kernel_times())
            gpu_ctx.enable_timing(False)
            assert names == ["clip_rms_split", "clip_pick", fam.label(), "clip_fbank_mean" if fam.name == "fbank" else "clip_mel_max"], names
            what = f"{fam.id} pcm16={pcm16} step {step}"
            assert_same(got, want, fam, what)
            assert_same(dev.run(idx, step, split=True, host=True), want, fam, what + " host form")
            assert_model(fam, lay, idx, got, what)
        # the pick that only the whole clip decides
        j = next(j for j, i in enumerate(groups[3]) if lay.items[i].get("seam_pick"))
        res3 = dev.run([groups[3][j]], 3, split=True)
        assert int(res3["best_channel"][0]) == 2
    finally:
        dev.close()


@pytest.mark.parametrize("fam", FAMILIES, ids=[f.id for f in FAMILIES])
def test_norm_order_alone_refusals_and_the_contiguous_call_around(fv, gpu_ctx, fam):
    """norm / cmn; invariant 2 (rows permuted, exported one at a time, the output elsewhere); invariant 3 (a refused call leaves
    the canary); invariant 4 (a contiguous call writes the same bytes before and after split calls)"""
    rng = np.random.default_rng(17)
    lay, step = sc.Layout(False), 3
    F = fam.tile_frames
    for k, (T, C_, pick) in enumerate([(9, 1, 0), (2 * F + 3, 2, 1), (F, 1, 0), (F + 1, 5, 2), (7, 2, 0), (1, 1, 0)]):
        L = fam.L_of_frames(T, k)
        skip = k % step
        lanes = sc.clip_lanes(rng, L, step, skip, C_, pick, mc.SIGNALS[k % 4], False, C_ == 1)
        a_len = [lanes.shape[1] // 2, 1, lanes.shape[1] - 1, lanes.shape[1] // 3, 0, lanes.shape[1]][k]
        lay.add(lanes, a_len, skip, step, off=sc.FEW_PAIRS[k])
    lay.build()
    idx = list(range(len(lay.items)))
    total = plan_total(fv, fam, lay, idx, step)
    dev = Device(gpu_ctx, fam, lay, total + 8)
    extra = dict(norm=(8.0, 4.0, 0.25)) if fam.name == "mel" else dict(cmn=True)
    try:
        before, before_n = dev.run(idx, step, split=False), dev.run(idx, step, split=False, **extra)
        got = dev.run(idx, step, split=True)
        assert_same(got, before, fam, f"{fam.id} plain")
        assert_model(fam, lay, idx, got, f"{fam.id} plain")
        got_n = dev.run(idx, step, split=True, **extra)
        assert_same(got_n, before_n, fam, f"{fam.id} {extra}")
        assert any(x.tobytes() != y.tobytes() for x, y in zip(got_n["feats"], got["feats"])), "the normalisation did nothing"
        assert_same(dev.run(idx, step, split=True, host=True, **extra), before_n, fam, f"{fam.id} {extra} host form")
        # invariant 2
        rev = dev.run(idx[::-1], step, split=True, off=1)
        for f in REPORTS[2:] + (fam.extra, "n_frames"):
            assert rev[f][::-1].tobytes() == got[f].tobytes(), f
        assert all(x.tobytes() == y.tobytes() for x, y in zip(rev["feats"][::-1], got["feats"])), "the row order changes a feature"
        for i in idx:
            alone = dev.run([i], step, split=True, **extra)
            assert alone["feats"][0].tobytes() == got_n["feats"][i].tobytes() and alone[fam.extra][0].tobytes() == got_n[fam.extra][i].tobytes(), ("alone", i)
        # invariant 3: the capacity one float short, a piece past its buffer, the output over piece B
        dev.fill()
        for kw in (dict(out_capacity=total - 1), dict(a=(dev.d_a, lay.a_lanes, lay.a_stride, 3)), dict(d_out=dev.d_b + 16)):
            with pytest.raises(fv.FvadError):
                fam.split(gpu_ctx, dev.d_a, dev.d_b, lay, idx, step, **dict(dict(d_out=dev.d_out, out_capacity=total), **kw))
            assert dev.canaries_intact(), kw
        assert gpu_ctx.to_host(np.zeros_like(lay.B), dev.d_b).tobytes() == np.ascontiguousarray(lay.B).tobytes()
        # invariant 4
        assert_same(dev.run(idx, step, split=False), before, fam, f"{fam.id} contiguous after split")
        assert_same(dev.run(idx, step, split=False, **extra), before_n, fam, f"{fam.id} contiguous {extra} after split")
    finally:
        dev.close()


@pytest.mark.parametrize("pcm16", [False, True], ids=["from-f32", "from-pcm16"])
@pytest.mark.parametrize("fam", [FAMILIES[0], FAMILIES[1], FAMILIES[3]], ids=[FAMILIES[i].id for i in (0, 1, 3)])
def test_digital_silence_across_the_seam_is_exactly_the_log_of_the_floor(fv, gpu_ctx, fam, pcm16):
    lay = sc.Layout(pcm16)
    n = 3 * 2000
    for a_len in (0, 1, 2999, 3000, n - 1, n):
        lay.add(np.zeros((1, n), np.int16 if pcm16 else np.float32), a_len, 1, 3)
    lay.build()
    idx = list(range(len(lay.items)))
    dev = Device(gpu_ctx, fam, lay, plan_total(fv, fam, lay, idx, 3) + 8)
    try:
        for floor in (1e-10, 3e-7, 2.5):
            fam_floor = fam.floor
            fam.floor = np.float32(floor)
            try:
                res = dev.run(idx, 3, split=True)
            finally:
                fam.floor = fam_floor
            log = np.log10 if fam.name == "mel" else np.log
            want = np.float32(log(np.float64(np.float32(floor))))
            for x in res["feats"]:
                assert x.shape[0] == fam.n_frames(2000) and x.tobytes() == np.full(x.shape, want, np.float32).tobytes(), floor
            if fam.name == "mel":
                assert res["feat_max"].tobytes() == np.full(len(idx), want, np.float32).tobytes()
    finally:
        dev.close()
