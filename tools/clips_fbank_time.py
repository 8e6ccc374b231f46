"""Cost of getting a corpus's Kaldi-style filter-bank features off the GPU, on tools/clips_mel_time.py's corpus: S mono streams x
H hours of synthetic denoised-like audio resident on the device (seeded noise, generated there) and per stream the seeded clip
schedule (2.5 .. 12 s every 3 .. 60 s).  The front end is the harness's (simulator.FBANK) on the lanes' samples = 2 (mod 3):
frames of 400 every 160 (snip_edges), DC removed, pre-emphasis 0.97, Povey window, 512-point transform, 80 Kaldi bands, ln.
  (a) what a caller had before: fvad_clips_export_strided as f32 (step 3, phase 2), then the same front end in numpy float32 on
      the host.  The numpy part runs over the first --numpy-clips clips and is SCALED to all of them by their frame counts (the
      export itself is timed whole); 0 runs it over every clip;
  (b) fvad_clips_export_fbank: wall, and clip_fbank by device events;
  (c) fvad_clips_export_mel at n_fft 512 (periodic Hann, hop 160, 80 Slaney bands): the same generic transform without the
      conditioning, what the conditioning and the snip_edges framing cost beside it.
Protocol (tools/clips_mel_time.py's): one warm-up of each, then the three alternated --reps times in one process, wall time as
median [min - max]; the kernels' device time by events (fvad_ctx_kernel_times).  (b)'s features are held against (a)'s on the clips
(a) computed.  Every GPU step runs under a time limit of its own (--step-limit seconds, SIGALRM).
python tools/clips_fbank_time.py [--streams 21] [--hours 2] [--reps 3] [--numpy-clips 300]"""
import argparse
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from conftest import load_package  # noqa: E402
from clips_time import clip_schedule  # noqa: E402

PHASE = 2


def numpy_features(s, w, M, p):
    """float32 throughout: snip_edges frames, DC removal, pre-emphasis, window, zero-padded rfft, power, bands, ln"""
    win, hop = p["win_length"], p["hop"]
    T = 1 + (len(s) - win) // hop
    x = (s * np.float32(p["scale"]))[np.arange(T)[:, None] * hop + np.arange(win)[None, :]]
    d = x - x.sum(axis=1, dtype=np.float32)[:, None] / np.float32(win)
    y = (d - np.float32(p["preemph"]) * np.concatenate([d[:, :1], d[:, :-1]], axis=1)) * w
    X = np.fft.rfft(y, n=p["n_fft"], axis=1)
    P = X.real * X.real + X.imag * X.imag
    return np.log(np.maximum(P.astype(np.float32) @ M.T, np.float32(p["floor"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--numpy-clips", type=int, default=300)
    ap.add_argument("--step-limit", type=int, default=120)
    a = ap.parse_args()
    import torch
    pkg = load_package()
    fv, p = pkg.binding, pkg.simulator.FBANK
    ctx = fv.Context(0)
    S, step, win, n_fft, hop, n_mels = a.streams, p["step"], p["win_length"], p["n_fft"], p["hop"], p["n_mels"]
    L = int(a.hours * 3600 * 48000) // 24000 * 24000
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    signal.alarm(a.step_limit)
    audio = torch.empty((S, L), dtype=torch.float32, device=dev)
    for l in range(S):
        audio[l] = torch.randn(L, generator=g, device=dev) * 0.05
    torch.cuda.synchronize()
    signal.alarm(0)
    clips = clip_schedule(S, 1, L, a.seed)
    skips = fv.clips_phase_skips(clips[:, 2], step, PHASE)
    frames, _, total = fv.clips_plan_fbank(clips[:, 3] - clips[:, 2], skips, step, win, hop, n_mels)
    n_frames = int(frames.sum())
    n_clip_samples = int((clips[:, 3] - clips[:, 2]).sum())
    n_np = len(clips) if a.numpy_clips <= 0 else min(a.numpy_clips, len(clips))
    scale = n_frames / float(frames[:n_np].sum())
    w = pkg.simulator.fbank_window()
    M = fv.mel_design_kaldi(p["sample_rate"], n_fft, n_mels, p["low_freq"], p["high_freq"])
    w_mel = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)).astype(np.float32)
    M_mel = fv.mel_design(16000, n_fft, n_mels, 0, 8000)
    print(f"{S} streams x {a.hours:g} h: {S * L * 4 / 1e9:.2f} GB of f32 on the device; {len(clips)} clips, {n_clip_samples / 48000 / S:.0f} s per stream, "
          f"{n_frames} frames, {total * 4 / 1e9:.3f} GB of features; (a)'s numpy part over the first {n_np} clips, SCALED by {scale:.2f}", flush=True)
    # the minima of clip_fbank for this clip set (computed, not measured): every 64-byte line of the clips' span once from HBM (a
    # kept sample every 12 bytes: every line holds one); per frame 5 f32 operations per tap of conditioning and windowing, 5 N log2 N
    # of a 256-point complex transform with its un-mixing, 3 per bin of power and 2 per (bin, band) of projection; per frame the LDS
    # traffic of the conditioning (read x twice, write and read d, write y), of the transform's passes (four radix-4 passes of 256
    # complex, read and written) and of the projection (every band reads every power)
    nb = n_fft // 2 + 1
    flops = n_frames * (5 * win + 5 * (n_fft // 2) * np.log2(n_fft // 2) + 8 * (n_fft // 2) + 3 * nb + 2 * nb * n_mels)
    lds = n_frames * 4 * (5 * win + n_fft + 2 * 4 * n_fft + 2 * n_fft + 2 * nb + nb * n_mels)
    print(f"minima for this clip set: HBM {n_clip_samples * 4 / 1e9:.2f} GB in + {total * 4 / 1e9:.3f} GB out = {(n_clip_samples + total) * 4 / 8e12 * 1e3:.2f} ms at 8 TB/s; "
          f"vector {flops / 1e9:.1f} GFLOP = {flops / 78.6e12 * 1e3:.2f} ms at 78.6 TFLOP/s (f32, no FMA: contraction is off); "
          f"LDS {lds / 1e9:.1f} GB = {lds / (256 * 128 * 2.4e9) * 1e3:.2f} ms at 128 B/clk/CU, 256 CUs, 2.4 GHz", flush=True)
    ctx.enable_timing(True)
    ctx.set_option("clip_mel_fft", "generic")
    wall = {"a": [], "b": [], "c": []}
    parts = []
    kern = {"b": [], "c": []}
    copied, kept = {}, {}
    for rep in range(-1, a.reps):   # (-1: the warm-up, not kept)
        for way in ("a", "b", "c"):
            ctx.kernel_times()
            signal.alarm(a.step_limit)
            t0 = time.perf_counter()
            if way == "a":
                res = ctx.clips_export(audio.data_ptr(), False, S, L, L, clips, step=step, skips=skips)
                signal.alarm(0)
                t1 = time.perf_counter()
                feats = [numpy_features(res["out"][int(o):int(o) + int(n)], w, M, p) for o, n in zip(res["offsets"][:n_np], res["out_lens"][:n_np])]
                t2 = time.perf_counter()
                t = (t1 - t0) + (t2 - t1) * scale
                copied["a"] = res["out"].nbytes
                if rep >= 0:
                    parts.append((t1 - t0, (t2 - t1) * scale))
            elif way == "b":
                res = ctx.clips_export_fbank(audio.data_ptr(), False, S, L, L, clips, w, M, n_fft=n_fft, step=step, skips=skips, hop=hop, scale=p["scale"],
                                             preemph=p["preemph"], remove_dc=p["remove_dc"], floor=p["floor"])
                signal.alarm(0)
                t = time.perf_counter() - t0
                copied[way] = res["out"].nbytes
            else:
                res = ctx.clips_export_mel(audio.data_ptr(), False, S, L, L, clips, w_mel, M_mel, step=step, skips=skips, hop=hop, floor=1e-10)
                signal.alarm(0)
                t = time.perf_counter() - t0
                copied[way] = res["out"].nbytes
            if rep >= 0:
                wall[way].append(t)
                if way != "a":
                    kt = ctx.kernel_times()
                    kern[way].append([kt.get("clip_rms", np.nan), kt.get("clip_pick", np.nan), kt.get("clip_fbank" if way == "b" else "clip_mel", np.nan),
                                      kt.get("clip_fbank_mean" if way == "b" else "clip_mel_max", np.nan)])
            if rep == -1:
                kept[way] = feats if way == "a" else res
    ctx.set_option("clip_mel_fft", None)
    worst, r = 0.0, kept["b"]
    for j, f in enumerate(kept["a"]):
        o, T = int(r["offsets"][j]), int(r["n_frames"][j])
        got = r["out"][o:o + T * n_mels].reshape(T, n_mels)
        assert got.shape == f.shape
        worst = max(worst, float(np.abs(got - f).max()))
    print(f"(b)'s features against (a)'s numpy float32 ones over {n_np} clips: largest difference {worst:.2e} (ln units)")

    def mmm(v):
        return f"{np.median(v):9.3f} [{min(v):9.3f} - {max(v):9.3f}]"
    names = {"a": "(a) fvad_clips_export_strided f32 + numpy float32 front end (SCALED)", "b": "(b) fvad_clips_export_fbank",
             "c": "(c) fvad_clips_export_mel, n_fft 512, generic transform"}
    for way in ("a", "b", "c"):
        print(f"{names[way]:70s}: wall {mmm(wall[way])} s | {copied[way] / 1e9:7.3f} GB over PCIe", flush=True)
    q = np.array(parts)
    print(f"{'(a) its parts':70s}: export {mmm(q[:, 0])} s | numpy (SCALED) {mmm(q[:, 1])} s")
    for way in ("b", "c"):
        k = np.array(kern[way])
        main_k = np.median(k[:, 2])
        print(f"{names[way]:70s}: clip_rms {mmm(k[:, 0])} ms | clip_pick {mmm(k[:, 1])} ms | {'clip_fbank' if way == 'b' else 'clip_mel':10s} {mmm(k[:, 2])} ms | "
              f"{'clip_fbank_mean' if way == 'b' else 'clip_mel_max'} {mmm(k[:, 3])} ms || per frame {main_k * 1e6 / n_frames:.1f} ns")
    ctx.close()


if __name__ == "__main__":
    main()
