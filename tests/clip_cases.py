"""The float64 model and the case tables of the batch Recorder tests (fvad_clips_*; test_clips_host.py, test_clips_gpu.py).

The model is the statement of what fvad_clips_export computes, in numpy:
  * a clip (first_lane, n_channels, sample_from, sample_to) reads lanes first_lane .. first_lane + n_channels - 1 over
    [sample_from, sample_to);
  * rms of a channel = f32(sqrt(mean(f64(x)^2))), x the samples as f32 (PCM16: s / 32768, exact);
  * the pick is Recorder.findBestChannel's (Recorder.zig:113-129): strict `<` in channel order from 9999, the lowest index
    wins a tie; runner_up_rms = the smallest RMS among the other channels (best_rms for a mono clip);
  * the samples are the picked channel's, converted where the formats differ: PCM16 -> f32 is s / 32768, f32 -> PCM16 is
    rint(clamp(y * 32768, -32768, 32767)) in f32; equal formats are the source's bits;
  * slots start on 16-byte boundaries, in clip order.
`model_export(..., mutation=...)` states three wrong versions; test_clips_host.py shows that `compare` over the case table
fails each of them, i.e. that the table holds the clips that tell them apart (exact ties, clips whose neighbours differ, lanes
whose neighbours differ)."""
import numpy as np

TILE = 8192            # kClipTile of csrc/kernels.h: the samples of one (clip, channel) a workgroup handles
N_SAMPLES = 120000
SENTINEL = -32768      # PCM16 sources outside every clip (f32 sources: NaN); the data never takes this value
# streams of the source: (first_lane, n_channels); lane 0 belongs to no stream, so that no first_lane is 0
STREAMS = {"A": (1, 1), "B": (2, 2), "C": (4, 3), "D": (7, 5)}
N_LANES = 12
SCALE = np.float32(1.0 - 2.0 ** -10)


def zones(name):
    """a stream of C channels has C + 1 zones of equal length: in zone z < C every channel is the same signal (odd channels
    negated: the same RMS exactly) and channel z is that signal scaled by 1 - 2^-10; in zone C the channels are independent,
    except that two of them are an exact tie (see make_source) -> [(from, to)]"""
    C_ = STREAMS[name][1]
    n = N_SAMPLES // (C_ + 1)
    return [(z * n, (z + 1) * n) for z in range(C_ + 1)]


def make_source(pcm16, seed=5):
    """[N_LANES][N_SAMPLES] float32 or int16, before the sentinels are laid over what no clip covers.  Every signal is drawn in
    the source's own format, so that a negated copy is exact"""
    rng = np.random.default_rng(seed)

    def draw(n, gain=1.0):
        if pcm16:
            return rng.integers(int(-15000 * gain), int(15000 * gain), n).astype(np.int16)
        return rng.uniform(-0.45 * gain, 0.45 * gain, n).astype(np.float32)

    def scaled(x):
        return np.rint(x * float(SCALE)).astype(np.int16) if pcm16 else x * SCALE

    out = np.zeros((N_LANES, N_SAMPLES), np.int16 if pcm16 else np.float32)
    out[0] = draw(N_SAMPLES)
    for name, (l0, C_) in STREAMS.items():
        zs = zones(name)
        for z, (a, b) in enumerate(zs[:-1]):
            x = draw(b - a)
            for c in range(C_):
                out[l0 + c, a:b] = scaled(x) if c == z else (x if c % 2 == 0 else -x)
        a, b = zs[-1]
        for c in range(C_):
            out[l0 + c, a:b] = draw(b - a, 1.0 - 0.05 * c)
        if C_ == 2:
            out[l0 + 1, a:b] = -out[l0, a:b]                      # an exact tie: channel 0 stands
        elif C_ > 2:
            out[l0 + 1, a:b] = draw(b - a, 0.6)
            out[l0 + 2, a:b] = -out[l0 + 1, a:b]                  # the two quietest tie: channel 1 stands
    if not pcm16:
        # the f32 -> PCM16 rule's corners, in stream A's last zone: clamps on both sides and halfway cases of rint
        a = zones("A")[-1][0]
        out[1, a:a + 10] = np.array([1.0, -1.0, 1.5, -1.5, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768,
                                     32766.5 / 32768], np.float32)
    # digital silence on every channel of stream D
    l0, C_ = STREAMS["D"]
    out[l0:l0 + C_, SILENCE[0]:SILENCE[1]] = 0
    return out


SILENCE = (110000, 113000)


def case_table():
    """[(first_lane, n_channels, sample_from, sample_to)], and the names of the clips the tests single out"""
    clips, names = [], {}

    def add(stream, a, b, name=None):
        l0, C_ = STREAMS[stream]
        if name:
            names[name] = len(clips)
        clips.append((l0, C_, a, b))

    # lengths 1 .. 9, each start at another of the 8 sample alignments, mono and stereo (B's last zone: the exact tie)
    for s, base in (("A", zones("A")[1][0]), ("B", zones("B")[2][0])):
        for i, n in enumerate((1, 2, 3, 4, 5, 7, 8, 9)):
            add(s, base + 100 * i + i, base + 100 * i + i + n)
    # both sides of one tile and of two tiles, and three tiles plus 3, again over the 8 alignments
    for s, base in (("A", zones("A")[1][0] + 1000), ("B", zones("B")[0][0])):
        for i, n in enumerate((TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 3)):
            add(s, base + i + 1, base + i + 1 + n)
    # the source's first sample and its last
    add("A", 0, 5000, "first")
    add("D", N_SAMPLES - 3000, N_SAMPLES, "last")
    add("B", N_SAMPLES - 1, N_SAMPLES)
    # overlapping clips and duplicates
    z = zones("C")[3][0]
    add("C", z + 5, z + 9000, "dup")
    add("C", z + 4000, z + 12000)
    add("C", z + 5, z + 9000)
    # the scaled channel in every position 0 .. C - 1 (two tiles and a bit), and the ties of each stream's last zone
    for s in ("A", "B", "C", "D"):
        zs = zones(s)
        for p, (a, _) in enumerate(zs[:-1]):
            add(s, a + 13 + p, a + 13 + p + TILE + 809, f"scaled-{s}-{p}")
        add(s, zs[-1][0] + 3, zs[-1][0] + 3 + 2 * TILE + 5, f"tie-{s}")
    add("A", zones("A")[1][0], zones("A")[1][0] + 64, "corners")
    add("D", SILENCE[0], SILENCE[1], "silence")
    add("D", SILENCE[0] + 7, SILENCE[0] + 8)
    return np.array(clips, np.uint64), names


def mask_outside(src, clips):
    """the source with NaN (f32) or SENTINEL (PCM16) everywhere outside the clips' ranges"""
    covered = np.zeros(src.shape, bool)
    for l0, C_, a, b in np.asarray(clips, np.int64):
        covered[l0:l0 + C_, a:b] = True
    out = src.copy()
    out[~covered] = np.nan if src.dtype == np.float32 else SENTINEL
    return out


def as_f32(x):
    return x.astype(np.float32) * np.float32(1.0 / 32768.0) if x.dtype == np.int16 else x


def convert(x, out_pcm16):
    if (x.dtype == np.int16) == bool(out_pcm16):
        return x.copy()                                                    # equal formats: the bits
    if out_pcm16:
        with np.errstate(invalid="ignore"):   # (a mutated model may convert the NaN outside a clip)
            return np.rint(np.clip(x * np.float32(32768.0), np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)
    return as_f32(x)


def rms_f32(x):
    return np.float32(np.sqrt(np.mean(as_f32(x).astype(np.float64) ** 2)))


def plan(clips, out_pcm16):
    per16 = 8 if out_pcm16 else 4
    offsets, at = [], 0
    for _, _, a, b in np.asarray(clips, np.int64):
        offsets.append(at)
        at += (b - a + per16 - 1) // per16 * per16
    return np.array(offsets, np.uint64), at


def model_export(src, clips, out_pcm16, mutation=None):
    """-> dict(best_channel, best_rms, runner_up_rms, offsets, total, samples=[per clip]); mutation: None | "le" (the pick by
    <=) | "late" (the clip cut one sample late) | "lane" (RMS over the next lane)"""
    n_lanes, n = src.shape
    offsets, total = plan(clips, out_pcm16)
    best, brms, runner, samples = [], [], [], []
    for l0, C_, a, b in np.asarray(clips, np.int64):
        r = [rms_f32(src[(l0 + c + (1 if mutation == "lane" else 0)) % n_lanes, a:b]) for c in range(C_)]
        pick, vol = 0, np.float32(9999.0)
        for c in range(C_):
            if (r[c] <= vol) if mutation == "le" else (r[c] < vol):
                pick, vol = c, r[c]
        others = [r[c] for c in range(C_) if c != pick]
        best.append(pick)
        brms.append(r[pick])
        runner.append(min(others) if others else r[pick])
        d = 1 if mutation == "late" else 0
        samples.append(convert(src[l0 + pick, min(a + d, n - (b - a)):min(b + d, n)], out_pcm16))
    return {"best_channel": np.array(best, np.int32), "best_rms": np.array(brms, np.float32),
            "runner_up_rms": np.array(runner, np.float32), "offsets": offsets, "total": total, "samples": samples}


def within_one_ulp(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


def compare(got, want, what=""):
    """a result (the model's dict, or the library's with `samples` cut from its output) against the model's: picks, offsets and
    sample bits exact; both RMS within one f32 ulp of f32(sqrt(mean(f64(x)^2))) -- the products are exact in f64 and the f64 sum
    of at most a few 10^7 terms carries a relative error far below 2^-24, so only the final roundings can differ"""
    assert np.array_equal(got["best_channel"], want["best_channel"]), (what, "best_channel", np.flatnonzero(got["best_channel"] != want["best_channel"]))
    assert np.array_equal(got["offsets"], want["offsets"]) and got["total"] == want["total"], (what, "offsets")
    for k in ("best_rms", "runner_up_rms"):
        assert within_one_ulp(got[k], want[k]), (what, k, got[k], want[k])
    for i, (g, w) in enumerate(zip(got["samples"], want["samples"])):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, "samples of clip", i)
