"""Cost of getting a corpus's recogniser features off the GPU, on tools/clips_time.py's corpus shape: S mono streams x H hours of
synthetic denoised-like audio resident on the device (seeded noise, generated there) and per stream the seeded clip schedule
(2.5 .. 12 s every 3 .. 60 s), the front end on the lanes' samples = 2 (mod 3), the network's own 16 kHz output.  Three ways:
  (a) what a caller had before the feature exports: fvad_clips_export_strided as f32 (step 3, phase 2), then the same front end
      in numpy float32 on the host.  The numpy part runs over the first --numpy-clips clips and is scaled to all of them by
      their frame counts (the export itself is timed whole); 0 runs it over every clip;
--features logmel: Whisper's front end (400-point periodic Hann, hop 160, 80 Slaney bands, log10(max(., 1e-10)))
  (b) fvad_clips_export_mel (clip_mel_fft auto: the 400-point eight-frames-per-wavefront transform);
  (c) the same with clip_mel_fft=generic.
--features fbank: the harness's Kaldi front end (simulator.FBANK: frames of 400 every 160 (snip_edges), DC removed, pre-emphasis
0.97, Povey window, 512-point transform, 80 Kaldi bands, ln), everything with clip_mel_fft=generic
  (b) fvad_clips_export_fbank: wall, and clip_fbank by device events;
  (c) fvad_clips_export_mel at n_fft 512 (periodic Hann, hop 160, 80 Slaney bands): the same generic transform without the
      conditioning, what the conditioning and the snip_edges framing cost beside it.
Protocol (tools/clips_time.py's): one warm-up of each, then the three alternated --reps times in one process, wall time as
median [min - max]; for (b) and (c) the kernels' device time by events (fvad_ctx_kernel_times).  The bytes each way copies over
PCIe are printed beside the times, and the export's features are held against (a)'s on the clips (a) computed.  Every GPU step runs
under a time limit of its own (--step-limit seconds, SIGALRM: a step that hangs ends the process instead of holding the device).
python tools/clips_features_time.py --features logmel|fbank [--streams 21] [--hours 2] [--reps 3] [--numpy-clips 500|300]"""
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


def hann(n):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)


def numpy_logmel(s, w, M, p):
    """float32 throughout: frames by reflection, rfft, power, mel, log10; the last frame of torch.stft(center=True) dropped"""
    T = len(s) // HOP
    x = np.pad(s, N_FFT // 2, mode="reflect")
    idx = np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]
    X = np.fft.rfft(x[idx] * w, axis=1)
    P = X.real * X.real + X.imag * X.imag
    return np.log10(np.maximum(P.astype(np.float32) @ M.T, FLOOR))


def numpy_fbank(s, w, M, p):
    """float32 throughout: snip_edges frames, DC removal, pre-emphasis, window, zero-padded rfft, power, bands, ln"""
    win, hop = p["win_length"], p["hop"]
    T = 1 + (len(s) - win) // hop
    x = (s * np.float32(p["scale"]))[np.arange(T)[:, None] * hop + np.arange(win)[None, :]]
    d = x - x.sum(axis=1, dtype=np.float32)[:, None] / np.float32(win)
    y = (d - np.float32(p["preemph"]) * np.concatenate([d[:, :1], d[:, :-1]], axis=1)) * w
    X = np.fft.rfft(y, n=p["n_fft"], axis=1)
    P = X.real * X.real + X.imag * X.imag
    return np.log(np.maximum(P.astype(np.float32) @ M.T, np.float32(p["floor"])))


def fbank_minima(p, n_frames, n_clip_samples, total):
    """the minima of clip_fbank for this clip set (computed, not measured): every 64-byte line of the clips' span once from HBM (a
    kept sample every 12 bytes: every line holds one); per frame 5 f32 operations per tap of conditioning and windowing, 5 N log2 N
    of a 256-point complex transform with its un-mixing, 3 per bin of power and 2 per (bin, band) of projection; per frame the LDS
    traffic of the conditioning (read x twice, write and read d, write y), of the transform's passes (four radix-4 passes of 256
    complex, read and written) and of the projection (every band reads every power)"""
    win, n_fft, n_mels = p["win_length"], p["n_fft"], p["n_mels"]
    nb = n_fft // 2 + 1
    flops = n_frames * (5 * win + 5 * (n_fft // 2) * np.log2(n_fft // 2) + 8 * (n_fft // 2) + 3 * nb + 2 * nb * n_mels)
    lds = n_frames * 4 * (5 * win + n_fft + 2 * 4 * n_fft + 2 * n_fft + 2 * nb + nb * n_mels)
    print(f"minima for this clip set: HBM {n_clip_samples * 4 / 1e9:.2f} GB in + {total * 4 / 1e9:.3f} GB out = {(n_clip_samples + total) * 4 / 8e12 * 1e3:.2f} ms at 8 TB/s; "
          f"vector {flops / 1e9:.1f} GFLOP = {flops / 78.6e12 * 1e3:.2f} ms at 78.6 TFLOP/s (f32, no FMA: contraction is off); "
          f"LDS {lds / 1e9:.1f} GB = {lds / (256 * 128 * 2.4e9) * 1e3:.2f} ms at 128 B/clk/CU, 256 CUs, 2.4 GHz", flush=True)


def family(features, fv, sim):
    """what differs between the two tools this one replaced.  b, c: (row name, clip_mel_fft, the export's call, the two timed labels)"""
    if features == "logmel":
        w, M = hann(N_FFT), fv.mel_design(16000, N_FFT, N_MELS, 0, 8000)

        def mel(ctx, src, clips, skips):
            return ctx.clips_export_mel(*src, clips, w, M, step=STEP, skips=skips, hop=HOP, floor=float(FLOOR))
        return dict(p=None, step=STEP, hop=HOP, n_mels=N_MELS, plan=(fv.clips_plan_mel, N_FFT), numpy=numpy_logmel, w=w, M=M, numpy_clips=500,
                    scaled="scaled", width=60, label=11, held=("b", "c"), held_as="(b)'s and (c)'s", unit="log10", minima=None, hbm=True,
                    a="(a) fvad_clips_export_strided f32 + numpy float32 features",
                    b=("(b) fvad_clips_export_mel", None, mel, ("clip_mel400", "clip_mel_max")),
                    c=("(c) fvad_clips_export_mel, clip_mel_fft=generic", "generic", mel, ("clip_mel", "clip_mel_max")))
    p = sim.FBANK
    n_fft, n_mels = p["n_fft"], p["n_mels"]
    w, M = sim.fbank_window(), fv.mel_design_kaldi(p["sample_rate"], n_fft, n_mels, p["low_freq"], p["high_freq"])
    w_mel, M_mel = hann(n_fft), fv.mel_design(16000, n_fft, n_mels, 0, 8000)

    def fbank(ctx, src, clips, skips):
        return ctx.clips_export_fbank(*src, clips, w, M, n_fft=n_fft, step=p["step"], skips=skips, hop=p["hop"], scale=p["scale"],
                                      preemph=p["preemph"], remove_dc=p["remove_dc"], floor=p["floor"])

    def mel512(ctx, src, clips, skips):
        return ctx.clips_export_mel(*src, clips, w_mel, M_mel, step=p["step"], skips=skips, hop=p["hop"], floor=1e-10)
    return dict(p=p, step=p["step"], hop=p["hop"], n_mels=n_mels, plan=(fv.clips_plan_fbank, p["win_length"]), numpy=numpy_fbank, w=w, M=M,
                numpy_clips=300, scaled="SCALED", width=70, label=10, held=("b",), held_as="(b)'s", unit="ln", minima=fbank_minima, hbm=False,
                a="(a) fvad_clips_export_strided f32 + numpy float32 front end (SCALED)",
                b=("(b) fvad_clips_export_fbank", "generic", fbank, ("clip_fbank", "clip_fbank_mean")),
                c=("(c) fvad_clips_export_mel, n_fft 512, generic transform", "generic", mel512, ("clip_mel", "clip_mel_max")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", choices=("logmel", "fbank"), required=True)
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--numpy-clips", type=int, default=None)
    ap.add_argument("--step-limit", type=int, default=120)
    a = ap.parse_args()
    import torch
    pkg = load_package()
    fv = pkg.binding
    ctx = fv.Context(0)
    fam = family(a.features, fv, pkg.simulator)
    S, step, n_mels = a.streams, fam["step"], fam["n_mels"]
    numpy_clips = fam["numpy_clips"] if a.numpy_clips is None else a.numpy_clips
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
    src = (audio.data_ptr(), False, S, L, L)
    clips = clip_schedule(S, 1, L, a.seed)
    skips = fv.clips_phase_skips(clips[:, 2], step, PHASE)
    frames, _, total = fam["plan"][0](clips[:, 3] - clips[:, 2], skips, step, fam["plan"][1], fam["hop"], n_mels)
    n_frames = int(frames.sum())
    n_clip_samples = int((clips[:, 3] - clips[:, 2]).sum())
    n_np = len(clips) if numpy_clips <= 0 else min(numpy_clips, len(clips))
    scale = n_frames / float(frames[:n_np].sum())
    print(f"{S} streams x {a.hours:g} h: {S * L * 4 / 1e9:.2f} GB of f32 on the device; {len(clips)} clips, {n_clip_samples / 48000 / S:.0f} s per stream, "
          f"{n_frames} frames, {total * 4 / 1e9:.3f} GB of features; (a)'s numpy part over the first {n_np} clips, {fam['scaled']} by {scale:.2f}", flush=True)
    if fam["minima"]:
        fam["minima"](fam["p"], n_frames, n_clip_samples, total)
    ctx.enable_timing(True)
    wall = {"a": [], "b": [], "c": []}
    parts = []
    kern = {"b": [], "c": []}
    copied, kept = {}, {}
    for rep in range(-1, a.reps):   # (-1: the warm-up, not kept)
        for way in ("a", "b", "c"):
            ctx.kernel_times()
            ctx.set_option("clip_mel_fft", fam[way][1] if way != "a" else fam["b"][1])
            signal.alarm(a.step_limit)
            t0 = time.perf_counter()
            if way == "a":
                res = ctx.clips_export(*src, clips, step=step, skips=skips)
                signal.alarm(0)
                t1 = time.perf_counter()
                feats = [fam["numpy"](res["out"][int(o):int(o) + int(n)], fam["w"], fam["M"], fam["p"]) for o, n in zip(res["offsets"][:n_np], res["out_lens"][:n_np])]
                t2 = time.perf_counter()
                t = (t1 - t0) + (t2 - t1) * scale
                copied["a"] = res["out"].nbytes
                if rep >= 0:
                    parts.append((t1 - t0, (t2 - t1) * scale))
            else:
                res = fam[way][2](ctx, src, clips, skips)
                signal.alarm(0)
                t = time.perf_counter() - t0
                copied[way] = res["out"].nbytes
            if rep >= 0:
                wall[way].append(t)
                if way != "a":
                    kt = ctx.kernel_times()
                    kern[way].append([kt.get(k, np.nan) for k in ("clip_rms", "clip_pick") + fam[way][3]])
            if rep == -1:
                kept[way] = feats if way == "a" else res
    ctx.set_option("clip_mel_fft", None)
    worst = 0.0
    for way in fam["held"]:
        r = kept[way]
        for j, f in enumerate(kept["a"]):
            o, T = int(r["offsets"][j]), int(r["n_frames"][j])
            got = r["out"][o:o + T * n_mels].reshape(T, n_mels)
            assert got.shape == f.shape
            worst = max(worst, float(np.abs(got - f).max()))
    print(f"{fam['held_as']} features against (a)'s numpy float32 ones over {n_np} clips: largest difference {worst:.2e} ({fam['unit']} units)")

    def mmm(v):
        return f"{np.median(v):9.3f} [{min(v):9.3f} - {max(v):9.3f}]"
    W = fam["width"]
    names = {"a": fam["a"], "b": fam["b"][0], "c": fam["c"][0]}
    for way in ("a", "b", "c"):
        print(f"{names[way]:{W}s}: wall {mmm(wall[way])} s | {copied[way] / 1e9:7.3f} GB over PCIe", flush=True)
    q = np.array(parts)
    print(f"{'(a) its parts':{W}s}: export {mmm(q[:, 0])} s | numpy ({fam['scaled']}) {mmm(q[:, 1])} s")
    for way in ("b", "c"):
        k = np.array(kern[way])
        main_k, (first, second) = np.median(k[:, 2]), fam[way][3]
        hbm = f"; the span's lines from HBM at {n_clip_samples * 4 / main_k / 1e9:.2f} TB/s" if fam["hbm"] else ""
        print(f"{names[way]:{W}s}: clip_rms {mmm(k[:, 0])} ms | clip_pick {mmm(k[:, 1])} ms | {first:{fam['label']}s} {mmm(k[:, 2])} ms | "
              f"{second} {mmm(k[:, 3])} ms || per frame {main_k * 1e6 / n_frames:.1f} ns{hbm}")
    ctx.close()


if __name__ == "__main__":
    main()
