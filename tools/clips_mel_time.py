"""Cost of getting a corpus's log-mel features off the GPU, on tools/clips_time.py's corpus shape: S mono streams x H hours of
synthetic denoised-like audio resident on the device (seeded noise, generated there) and per stream the seeded clip schedule
(2.5 .. 12 s every 3 .. 60 s).  Three ways to the same features -- Whisper's front end on the lanes' samples = 2 (mod 3), the
network's own 16 kHz output: 400-point periodic Hann, hop 160, 80 Slaney bands, log10(max(., 1e-10)):
  (a) what a caller had before the feature export: fvad_clips_export_strided as f32 (step 3, phase 2), then the features in
      numpy float32 on the host (reflect-padded frames, single-precision rfft, power, matmul, log10).  The numpy part runs over
      the first --numpy-clips clips and is scaled to all of them by their frame counts (the export itself is timed whole); 0 runs
      it over every clip;
  (b) fvad_clips_export_mel (clip_mel_fft auto: the 400-point eight-frames-per-wavefront transform);
  (c) the same with clip_mel_fft=generic.
Protocol (tools/clips_time.py's): one warm-up of each, then the three alternated --reps times in one process, wall time as
median [min - max]; for (b) and (c) the kernels' device time by events (fvad_ctx_kernel_times).  The bytes each way copies over
PCIe are printed beside the times, and (b)'s features are held against (a)'s on the clips (a) computed.  Every GPU step runs under
a time limit of its own (--step-limit seconds, SIGALRM: a step that hangs ends the process instead of holding the device).
python tools/clips_mel_time.py [--streams 21] [--hours 2] [--reps 3] [--numpy-clips 500]"""
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

N_FFT, HOP, N_MELS, STEP, PHASE, FLOOR = 400, 160, 80, 3, 2, np.float32(1e-10)


def numpy_features(s, w, M):
    """float32 throughout: frames by reflection, rfft, power, mel, log10; the last frame of torch.stft(center=True) dropped"""
    T = len(s) // HOP
    x = np.pad(s, N_FFT // 2, mode="reflect")
    idx = np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]
    X = np.fft.rfft(x[idx] * w, axis=1)
    P = X.real * X.real + X.imag * X.imag
    return np.log10(np.maximum(P.astype(np.float32) @ M.T, FLOOR))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--numpy-clips", type=int, default=500)
    ap.add_argument("--step-limit", type=int, default=120)
    a = ap.parse_args()
    import torch
    pkg = load_package()
    fv = pkg.binding
    ctx = fv.Context(0)
    S = a.streams
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
    skips = fv.clips_phase_skips(clips[:, 2], STEP, PHASE)
    frames, _, total = fv.clips_plan_mel(clips[:, 3] - clips[:, 2], skips, STEP, N_FFT, HOP, N_MELS)
    n_frames = int(frames.sum())
    n_clip_samples = int((clips[:, 3] - clips[:, 2]).sum())
    n_np = len(clips) if a.numpy_clips <= 0 else min(a.numpy_clips, len(clips))
    scale = n_frames / float(frames[:n_np].sum())
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)).astype(np.float32)
    M = fv.mel_design(16000, N_FFT, N_MELS, 0, 8000)
    print(f"{S} streams x {a.hours:g} h: {S * L * 4 / 1e9:.2f} GB of f32 on the device; {len(clips)} clips, {n_clip_samples / 48000 / S:.0f} s per stream, "
          f"{n_frames} frames, {total * 4 / 1e9:.3f} GB of features; (a)'s numpy part over the first {n_np} clips, scaled by {scale:.2f}", flush=True)
    ctx.enable_timing(True)
    wall = {"a": [], "b": [], "c": []}
    parts = []
    kern = {"b": [], "c": []}
    copied, kept = {}, {}
    for rep in range(-1, a.reps):   # (-1: the warm-up, not kept)
        for way in ("a", "b", "c"):
            ctx.kernel_times()
            ctx.set_option("clip_mel_fft", "generic" if way == "c" else None)
            signal.alarm(a.step_limit)
            t0 = time.perf_counter()
            if way == "a":
                res = ctx.clips_export(audio.data_ptr(), False, S, L, L, clips, step=STEP, skips=skips)
                signal.alarm(0)
                t1 = time.perf_counter()
                feats = [numpy_features(res["out"][int(o):int(o) + int(n)], w, M) for o, n in zip(res["offsets"][:n_np], res["out_lens"][:n_np])]
                t2 = time.perf_counter()
                t = (t1 - t0) + (t2 - t1) * scale
                copied["a"] = res["out"].nbytes
                if rep >= 0:
                    parts.append((t1 - t0, (t2 - t1) * scale))
            else:
                res = ctx.clips_export_mel(audio.data_ptr(), False, S, L, L, clips, w, M, step=STEP, skips=skips, hop=HOP, floor=float(FLOOR))
                signal.alarm(0)
                t = time.perf_counter() - t0
                copied[way] = res["out"].nbytes
            if rep >= 0:
                wall[way].append(t)
                if way != "a":
                    kt = ctx.kernel_times()
                    kern[way].append([kt.get("clip_rms", np.nan), kt.get("clip_pick", np.nan), kt.get("clip_mel400" if way == "b" else "clip_mel", np.nan),
                                      kt.get("clip_mel_max", np.nan)])
            if rep == -1:
                kept[way] = feats if way == "a" else res
    ctx.set_option("clip_mel_fft", None)
    worst = 0.0
    for way in ("b", "c"):
        r = kept[way]
        for j, f in enumerate(kept["a"]):
            o, T = int(r["offsets"][j]), int(r["n_frames"][j])
            got = r["out"][o:o + T * N_MELS].reshape(T, N_MELS)
            assert got.shape == f.shape
            worst = max(worst, float(np.abs(got - f).max()))
    print(f"(b)'s and (c)'s features against (a)'s numpy float32 ones over {n_np} clips: largest difference {worst:.2e} (log10 units)")

    def mmm(v):
        return f"{np.median(v):9.3f} [{min(v):9.3f} - {max(v):9.3f}]"
    names = {"a": "(a) fvad_clips_export_strided f32 + numpy float32 features", "b": "(b) fvad_clips_export_mel", "c": "(c) fvad_clips_export_mel, clip_mel_fft=generic"}
    for way in ("a", "b", "c"):
        print(f"{names[way]:60s}: wall {mmm(wall[way])} s | {copied[way] / 1e9:7.3f} GB over PCIe", flush=True)
    p = np.array(parts)
    print(f"{'(a) its parts':60s}: export {mmm(p[:, 0])} s | numpy (scaled) {mmm(p[:, 1])} s")
    for way in ("b", "c"):
        k = np.array(kern[way])
        mel = np.median(k[:, 2])
        print(f"{names[way]:60s}: clip_rms {mmm(k[:, 0])} ms | clip_pick {mmm(k[:, 1])} ms | {'clip_mel400' if way == 'b' else 'clip_mel':11s} {mmm(k[:, 2])} ms | "
              f"clip_mel_max {mmm(k[:, 3])} ms || per frame {mel * 1e6 / n_frames:.1f} ns; the span's lines from HBM at {n_clip_samples * 4 / mel / 1e9:.2f} TB/s")
    ctx.close()


if __name__ == "__main__":
    main()
