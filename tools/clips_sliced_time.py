"""What slicing costs run_clips: the plan's speech clips exported from time slices (slice_chunks = N, the split-source Recorder and
the held tails) against the unsliced, device-resident run_clips on the same corpus -- S synthetic mono streams of H
hours as PCM16 WAV files (a 60 s synth.make_stream stream per seed, repeated to the length), written to --dir first.

The ways alternate in one process: one warm-up round that is not kept, then --rounds rounds, median [min - max].  Per way: wall
time of run_clips, the clip kernels' device time (clip_rms / clip_gather for the unsliced way, clip_rms_split / clip_gather_split
for the sliced ones, clip_pick for both; the sliced ones' include the carries), and the device memory of the audio each way
holds: the resident lanes (original + denoised, computed from shapes) for the unsliced way, the slice buffers (computed from
shapes) plus the held tails' peak (what run_clips reports) for the sliced ones.  The unsliced way is the yardstick; there is no
pass / fail number.  The first round also checks that every way wrote the same files.

python tools/clips_sliced_time.py [--streams 21] [--hours 2] [--slice-chunks 256,1024] [--rounds 3] [--ingest device] [--dir DIR]"""
import argparse
import filecmp
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402


def write_corpus(pkg, root, S, hours):
    fv, synth = pkg.binding, pkg.synth
    reps = max(1, int(round(hours * 60)))
    insts = []
    for s in range(S):
        pcm, labels = synth.make_stream(60.0, seed=500 + s)
        i16 = np.rint(np.clip(pcm, -1.0, 1.0) * 32767.0).astype(np.int16)
        fv.wav_write_i16(os.path.join(root, f"s{s}.wav"), np.tile(i16, reps))
        with open(os.path.join(root, f"s{s}.txt"), "w") as f:
            f.write(synth.labels_to_audacity([(a + 60.0 * r, b + 60.0 * r) for r in range(reps) for a, b in labels]))
        insts.append({"name": f"s{s}", "audio_path": f"s{s}.wav", "ref_path": f"s{s}.txt"})
    with open(os.path.join(root, "plan.json"), "w") as f:
        json.dump({"instances": insts, "config": {"vad_config": {}}}, f)
    return os.path.join(root, "plan.json"), reps * 60 * 48000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--slice-chunks", default="256,1024")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ingest", default="device", choices=("host", "device"))
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    pkg = load_package()
    fv, sim = pkg.binding, pkg.simulator
    root = a.dir or tempfile.mkdtemp(prefix="clips_sliced_")
    os.makedirs(root, exist_ok=True)
    t0 = time.perf_counter()
    plan, L = write_corpus(pkg, root, a.streams, a.hours)
    print(f"{a.streams} mono streams x {L / 48000 / 3600:.2f} h as PCM16 WAV in {root} ({time.perf_counter() - t0:.0f} s to write)", flush=True)
    ctx = fv.Context(0)
    ctx.load_synth(7)
    ctx.enable_timing(True)
    ways = [None] + [int(n) for n in a.slice_chunks.split(",") if n]
    name = {w: "unsliced" if w is None else f"slices of {w} chunks" for w in ways}
    wall, kern, mem, slices = {w: [] for w in ways}, {w: [] for w in ways}, {}, {}
    dirs = {w: os.path.join(root, "out-" + ("unsliced" if w is None else str(w))) for w in ways}
    S, H = a.streams, sim.SLICE_HALO_CHUNKS
    with ctx.options(reproducible="1"):
        for rnd in range(-1, a.rounds):   # (-1: the warm-up, not kept)
            for w in ways:
                shutil.rmtree(dirs[w], ignore_errors=True)
                ctx.kernel_times()
                info = {}
                t0 = time.perf_counter()
                sim.run_clips(plan, dirs[w], pcm16=True, ctx=ctx, ingest=a.ingest, slice_chunks=w, info=info)
                t = time.perf_counter() - t0
                kt = ctx.kernel_times()
                if rnd >= 0:
                    wall[w].append(t)
                    kern[w].append(sum(v for k, v in kt.items() if k.startswith("clip_")))
                if w is None:
                    mem[w] = (2 * S * L * 4, 0)
                else:
                    mem[w] = (2 * S * (w + H) * 24000 * 4, info["held_peak_bytes"])
                    slices[w] = info["slices"]
            if rnd == -1:
                ref = sorted(os.listdir(dirs[None]))
                for w in ways[1:]:
                    same = sorted(os.listdir(dirs[w])) == ref and all(
                        filecmp.cmp(os.path.join(dirs[None], n), os.path.join(dirs[w], n), shallow=False) for n in ref if n.endswith(".wav"))
                    print(f"{name[w]}: {len(ref)} files, the WAV files equal the unsliced run's: {same}", flush=True)

    def mmm(v):
        return f"{np.median(v):8.3f} [{min(v):8.3f} - {max(v):8.3f}]"
    base = np.median(wall[None])
    for w in ways:
        audio, held = mem[w]
        print(f"{name[w]:24s}: wall {mmm(wall[w])} s ({np.median(wall[w]) / base:.2f}x) | clip kernels {mmm(kern[w])} ms | audio on the device "
              f"{audio / 2 ** 20:9.1f} MiB" + ("" if w is None else f" + held tails {held / 2 ** 20:.1f} MiB at most, {slices[w]} slices"), flush=True)
    ctx.close()
    if a.dir is None:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
