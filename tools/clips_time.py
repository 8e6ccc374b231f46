"""Cost of getting a corpus's speech clips off the GPU, on config 4's corpus shape: S streams x H hours of synthetic
denoised-like audio resident on the device (seeded noise, generated there), C channels each, and per stream a seeded schedule
of clips (2.5 .. 12 s every 3 .. 60 s: about a fifth of the audio, the upper end of the 513 - 1447 s of speech per two-hour
stream the reference's README reports).  Three ways to the same clips -- the quietest channel of each, cut at its range:
  (a) what a caller without the batch Recorder has to do: copy every lane back (fvad_ctx_copy_to_host, one stream at a time
      into one reused buffer), cut the clips in numpy and pick by an f64 RMS per channel;
  (b) fvad_clips_export as f32;
  (c) fvad_clips_export as PCM16.
Protocol (tools/vad_sweep_time.py's): one warm-up of each, then the three alternated --reps times in one process, wall time as
median [min - max]; for (b) and (c) also the three kernels' device time by events (fvad_ctx_kernel_times) and, from the gather
kernel's bytes (read + written), its HBM rate.  The bytes each way copies over PCIe are printed beside the times.  (b)'s picks and
samples are checked against (a)'s once.
python tools/clips_time.py [--streams 21] [--hours 2] [--channels 1] [--reps 3]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402


def clip_schedule(S, C_, L, seed):
    """[n][4] uint64 clips (first_lane, n_channels, from, to), stream after stream, in time order"""
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(S):
        t = 0.0
        while True:
            t += rng.uniform(3.0, 60.0)
            n = rng.uniform(2.5, 12.0)
            a, b = int(t * 48000), int((t + n) * 48000)
            if b > L:
                break
            rows.append((s * C_, C_, a, b))
            t += n
    return np.array(rows, np.uint64)


def numpy_clips(ctx, audio, clips, C_, L, buf):
    """(a): every lane to the host, the clips cut and picked there -> (best channels, [clip samples], bytes copied)"""
    best, out, copied = [], [], 0
    by_stream = {}
    for i, c in enumerate(clips):
        by_stream.setdefault(int(c[0]) // C_, []).append(i)
    for s, idx in by_stream.items():
        ctx.to_host(buf, audio.data_ptr() + s * C_ * L * 4)
        copied += buf.nbytes
        for i in idx:
            a, b = int(clips[i][2]), int(clips[i][3])
            r = [np.float32(np.sqrt(np.mean(buf[c, a:b].astype(np.float64) ** 2))) for c in range(C_)]
            pick, vol = 0, np.float32(9999.0)
            for c in range(C_):
                if r[c] < vol:
                    pick, vol = c, r[c]
            best.append(pick)
            out.append(buf[pick, a:b].copy())
    return best, out, copied


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    a = ap.parse_args()
    import torch
    pkg = load_package()
    fv = pkg.binding
    ctx = fv.Context(0)
    S, C_ = a.streams, a.channels
    L = int(a.hours * 3600 * 48000) // 24000 * 24000
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    audio = torch.empty((S * C_, L), dtype=torch.float32, device=dev)
    for l in range(S * C_):   # channel c of a stream a little quieter than channel c - 1
        audio[l] = torch.randn(L, generator=g, device=dev) * (0.05 * (1.0 - 0.1 * (l % C_)))
    torch.cuda.synchronize()
    clips = clip_schedule(S, C_, L, a.seed)
    n_clip_samples = int((clips[:, 3] - clips[:, 2]).sum())
    print(f"{S} streams x {a.hours:g} h x {C_} channel(s): {S * C_ * L * 4 / 1e9:.2f} GB of f32 on the device; {len(clips)} clips, "
          f"{n_clip_samples / 48000 / S:.0f} s per stream, {n_clip_samples * 4 / 1e9:.2f} GB as f32", flush=True)
    buf = np.zeros((C_, L), np.float32)
    ctx.enable_timing(True)
    wall = {"a": [], "b": [], "c": []}
    kern = {"b": [], "c": []}
    copied = {}
    kept = {}
    for rep in range(-1, a.reps):   # (-1: the warm-up, not kept)
        for way in ("a", "b", "c"):
            ctx.kernel_times()
            t0 = time.perf_counter()
            if way == "a":
                best, out, copied["a"] = numpy_clips(ctx, audio, clips, C_, L, buf)
            else:
                res = ctx.clips_export(audio.data_ptr(), False, S * C_, L, L, clips, out_pcm16=(way == "c"))
                copied[way] = res["out"].nbytes
            t = time.perf_counter() - t0
            if rep >= 0:
                wall[way].append(t)
                if way != "a":
                    kt = ctx.kernel_times()
                    kern[way].append([kt.get(k, float("nan")) for k in ("clip_rms", "clip_pick", "clip_gather")])
            if rep == -1:
                kept[way] = (best, out) if way == "a" else res
    same = list(kept["b"]["best_channel"]) == kept["a"][0] and all(
        kept["b"]["out"][int(o):int(o) + len(x)].tobytes() == x.tobytes() for o, x in zip(kept["b"]["offsets"], kept["a"][1]))
    print(f"(b)'s picks and samples equal (a)'s: {same}")

    def mmm(v):
        return f"{np.median(v):9.3f} [{min(v):9.3f} - {max(v):9.3f}]"
    names = {"a": "(a) every lane to the host, numpy cut + f64 RMS pick", "b": "(b) fvad_clips_export f32", "c": "(c) fvad_clips_export PCM16"}
    for way in ("a", "b", "c"):
        print(f"{names[way]:55s}: wall {mmm(wall[way])} s | {copied[way] / 1e9:7.2f} GB over PCIe", flush=True)
    for way in ("b", "c"):
        k = np.array(kern[way])
        gather_bytes = n_clip_samples * (4 + (4 if way == "b" else 2))
        print(f"{names[way]:55s}: clip_rms {mmm(k[:, 0])} ms | clip_pick {mmm(k[:, 1])} ms | clip_gather {mmm(k[:, 2])} ms = "
              f"{gather_bytes / np.median(k[:, 2]) / 1e9:.2f} TB/s of HBM (read + written) | clip_rms reads "
              f"{n_clip_samples * C_ * 4 / np.median(k[:, 0]) / 1e9:.2f} TB/s")
    ctx.close()


if __name__ == "__main__":
    main()
