"""What exporting the speech clips at the denoiser's own 16 kHz saves (fvad_clips_export_strided with step 3) against
the full-rate export of the same clips, in one process.

Part 1, the export itself (tools/clips_time.py's corpus and seeded clip schedule: S streams x H hours of synthetic audio resident
on the device, clips of 2.5 .. 12 s every 3 .. 60 s): fvad_clips_export at step 1 and at step 3 (the skips of phase 2), as f32 and
as PCM16, alternated: one warm-up that is not kept, then --rounds rounds, median [min - max].  Per way: wall time, the bytes
copied over PCIe, the gather kernel's device time by events (clip_gather at step 1 -- the yardstick -- and clip_gather_strided
at step 3) and the HBM bytes it moves, computed from the shapes (every source sample of a clip read once; a third of them
written).  The step-3 samples are checked against the full-rate ones' [skip::3] once.

Part 2, run_clips (tools/clips_sliced_time.py's corpus: S mono streams of H hours as PCM16 WAV files): wall time with PCM16 clips
at 48000 and at 16000 (both kinds), unsliced and in slices of --slice-chunks chunks, alternated in the same way; the bytes of
WAV files each writes.  There is no pass / fail number.

python tools/clips_rate_time.py [--streams 21] [--hours 2] [--rounds 3] [--slice-chunks 1024] [--ingest device] [--no-harness] [--dir DIR]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_package  # noqa: E402
from clips_time import clip_schedule  # noqa: E402
from clips_sliced_time import write_corpus  # noqa: E402


def mmm(v):
    return f"{np.median(v):9.3f} [{min(v):9.3f} - {max(v):9.3f}]"


def export_part(pkg, a):
    import torch
    fv = pkg.binding
    ctx = fv.Context(0)
    S = a.streams
    L = int(a.hours * 3600 * 48000) // 24000 * 24000
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    audio = torch.empty((S, L), dtype=torch.float32, device=dev)
    for l in range(S):
        audio[l] = torch.randn(L, generator=g, device=dev) * 0.05
    torch.cuda.synchronize()
    clips = clip_schedule(S, 1, L, a.seed)
    n = int((clips[:, 3] - clips[:, 2]).sum())
    skips = fv.clips_phase_skips(clips[:, 2], 3, 2)
    n3 = int(fv.clips_plan_strided(clips[:, 3] - clips[:, 2], skips, 3)[0].sum())
    print(f"{S} mono streams x {a.hours:g} h on the device; {len(clips)} clips, {n / 48000 / S:.0f} s per stream: {n} samples at 48 kHz, {n3} at 16 kHz", flush=True)
    ways = [(step, pcm16) for pcm16 in (False, True) for step in (1, 3)]
    name = {(step, pcm16): f"step {step} {'PCM16' if pcm16 else 'f32  '}" for step, pcm16 in ways}
    wall, kern, copied, kept = {w: [] for w in ways}, {w: [] for w in ways}, {}, {}
    ctx.enable_timing(True)
    for rnd in range(-1, a.rounds):   # (-1: the warm-up, not kept)
        for w in ways:
            step, pcm16 = w
            ctx.kernel_times()
            t0 = time.perf_counter()
            res = ctx.clips_export(audio.data_ptr(), False, S, L, L, clips, out_pcm16=pcm16, step=step, skips=skips if step != 1 else None)
            t = time.perf_counter() - t0
            kt = ctx.kernel_times()
            copied[w] = res["out"].nbytes
            if rnd >= 0:
                wall[w].append(t)
                kern[w].append(kt["clip_gather" if step == 1 else "clip_gather_strided"])
            else:
                kept[w] = res
    for pcm16 in (False, True):
        full, third = kept[(1, pcm16)], kept[(3, pcm16)]
        same = (full["best_channel"].tobytes() == third["best_channel"].tobytes() and full["best_rms"].tobytes() == third["best_rms"].tobytes() and all(
            third["out"][int(o3):int(o3) + int(n3_)].tobytes() == full["out"][int(o) + int(k):int(o) + int(b - a_):3].tobytes()
            for (_, _, a_, b), k, o, o3, n3_ in zip(clips, skips, full["offsets"], third["offsets"], third["out_lens"])))
        print(f"{'PCM16' if pcm16 else 'f32'}: the step-3 samples are the full-rate export's [skip::3], picks and RMS equal: {same}", flush=True)
    for w in ways:
        step, pcm16 = w
        ob = 2 if pcm16 else 4
        hbm = n * 4 + (n if step == 1 else n3) * ob
        base = np.median(kern[(1, pcm16)])
        print(f"{name[w]}: wall {mmm(wall[w])} s | {copied[w] / 1e9:6.2f} GB over PCIe | gather {mmm(kern[w])} ms ({np.median(kern[w]) / base:.2f}x of step 1) | "
              f"{hbm / 1e9:5.2f} GB of HBM read + written = {hbm / np.median(kern[w]) / 1e9:.2f} TB/s", flush=True)
    ctx.close()
    del audio
    torch.cuda.empty_cache()


def harness_part(pkg, a):
    fv, sim = pkg.binding, pkg.simulator
    root = a.dir or tempfile.mkdtemp(prefix="clips_rate_")
    os.makedirs(root, exist_ok=True)
    t0 = time.perf_counter()
    plan, L = write_corpus(pkg, root, a.streams, a.hours)
    print(f"{a.streams} mono streams x {L / 48000 / 3600:.2f} h as PCM16 WAV in {root} ({time.perf_counter() - t0:.0f} s to write)", flush=True)
    ctx = fv.Context(0)
    ctx.load_synth(7)
    ways = [(sl, rate) for sl in (None, a.slice_chunks) for rate in (48000, 16000)]
    name = {(sl, rate): f"{'unsliced' if sl is None else f'slices of {sl}':16s} {rate} Hz" for sl, rate in ways}
    wall, size = {w: [] for w in ways}, {}
    out = os.path.join(root, "out")
    with ctx.options(reproducible="1"):
        for rnd in range(-1, a.rounds):   # (-1: the warm-up, not kept)
            for w in ways:
                sl, rate = w
                shutil.rmtree(out, ignore_errors=True)
                t0 = time.perf_counter()
                sim.run_clips(plan, out, pcm16=True, ctx=ctx, ingest=a.ingest, slice_chunks=sl, denoised_rate=rate, original_rate=rate)
                t = time.perf_counter() - t0
                if rnd >= 0:
                    wall[w].append(t)
                wavs = [f for f in os.listdir(out) if f.endswith(".wav")]
                size[w] = (len(wavs), sum(os.path.getsize(os.path.join(out, f)) for f in wavs))
    for w in ways:
        base = np.median(wall[(w[0], 48000)])
        print(f"run_clips PCM16 {name[w]}: wall {mmm(wall[w])} s ({np.median(wall[w]) / base:.2f}x of 48000) | {size[w][0]} files, {size[w][1] / 1e9:.2f} GB", flush=True)
    ctx.close()
    if a.dir is None:
        shutil.rmtree(root, ignore_errors=True)
    else:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--slice-chunks", type=int, default=1024)
    ap.add_argument("--ingest", default="device", choices=("host", "device"))
    ap.add_argument("--no-harness", action="store_true")
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    pkg = load_package()
    export_part(pkg, a)
    if not a.no_harness:
        harness_part(pkg, a)


if __name__ == "__main__":
    main()
