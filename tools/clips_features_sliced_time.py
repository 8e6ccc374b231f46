"""What the features cost a sliced run_clips, and what slicing costs a run_clips with features ("Features of a run
sliced in time"), on tools/clips_sliced_time.py's corpus: S synthetic mono streams of --harness-hours hours as PCM16 WAV files (a
60 s synth.make_stream stream per seed, repeated to the length), written to --dir first.  The ways:
  (a) run_clips(slice_chunks=N) without features -- what a sliced run could do before the split-source feature exports;
  (b) the same with features_sliced, per family: one fvad_clips_export_split_mel / _split_fbank per slice over the due clips;
  (c) the unsliced run_clips with features, per family: one fvad_clips_export_mel / _fbank over the resident lanes.
They alternate in one process: one warm-up round that is not kept, then --rounds rounds, median [min - max].  Per way: wall time
of run_clips; the device-event sums per kernel label over all of the run's calls (fvad_ctx_kernel_times, every label that starts
with clip_); the held tails' peak (what run_clips reports; sliced ways); and the bytes that cross PCIe towards the host, taken
from the files written (the clips' samples and the features).  There is no pass / fail number: the expectation is that the
feature kernels' summed time in (b) is (c)'s, the tiles being the same, and that the per-slice calls add their fixed costs.  The
first round also checks that (b) wrote (c)'s files.

python tools/clips_features_sliced_time.py [--streams 8] [--harness-hours 0.25] [--slice-chunks 256] [--rounds 3] [--ingest device] [--dir DIR]"""
import argparse
import filecmp
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from conftest import load_package  # noqa: E402
from clips_sliced_time import write_corpus  # noqa: E402

FAMILIES = ("logmel", "fbank")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--harness-hours", type=float, default=0.25)
    ap.add_argument("--slice-chunks", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ingest", default="device", choices=("host", "device"))
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    pkg = load_package()
    fv, sim = pkg.binding, pkg.simulator
    root = a.dir or tempfile.mkdtemp(prefix="clips_features_sliced_")
    os.makedirs(root, exist_ok=True)
    t0 = time.perf_counter()
    plan, L = write_corpus(pkg, root, a.streams, a.harness_hours)
    print(f"{a.streams} mono streams x {L / 48000 / 3600:.2f} h as PCM16 WAV in {root} ({time.perf_counter() - t0:.0f} s to write); "
          f"slices of {a.slice_chunks} chunks", flush=True)
    ctx = fv.Context(0)
    ctx.load_synth(7)
    ctx.enable_timing(True)
    N = a.slice_chunks
    ways = [("(a) sliced, no features", dict(slice_chunks=N))]
    ways += [(f"(b) sliced, {f}", dict(slice_chunks=N, features=f, features_sliced=True)) for f in FAMILIES]
    ways += [(f"(c) unsliced, {f}", dict(features=f)) for f in FAMILIES]
    wall, kern = {n: [] for n, _ in ways}, {n: [] for n, _ in ways}
    held, slices, pcie = {}, {}, {}
    dirs = {n: os.path.join(root, "out-" + n[:3].strip("() ") + "-" + n.split()[-1]) for n, _ in ways}
    with ctx.options(reproducible="1"):
        for rnd in range(-1, a.rounds):   # (-1: the warm-up, not kept)
            for name, kw in ways:
                shutil.rmtree(dirs[name], ignore_errors=True)
                ctx.kernel_times()
                info = {}
                t0 = time.perf_counter()
                sim.run_clips(plan, dirs[name], pcm16=True, ctx=ctx, ingest=a.ingest, info=info, **kw)
                t = time.perf_counter() - t0
                kt = ctx.kernel_times()
                if rnd >= 0:
                    wall[name].append(t)
                    kern[name].append({k: v for k, v in kt.items() if k.startswith("clip_")})
                held[name], slices[name] = info.get("held_peak_bytes"), info.get("slices")
                files = os.listdir(dirs[name])
                pcie[name] = (sum(os.path.getsize(os.path.join(dirs[name], f)) - 44 for f in files if f.endswith(".wav")),
                              sum(np.load(os.path.join(dirs[name], f), mmap_mode="r").nbytes for f in files if f.endswith(".npy")))
            if rnd == -1:
                for f in FAMILIES:
                    b, c = dirs[f"(b) sliced, {f}"], dirs[f"(c) unsliced, {f}"]
                    ref = sorted(os.listdir(c))
                    same = sorted(os.listdir(b)) == ref and all(filecmp.cmp(os.path.join(b, n), os.path.join(c, n), shallow=False)
                                                                for n in ref if not n.endswith(".json"))
                    print(f"{f}: {len(ref)} files, the sliced run's WAV and .npy files equal the unsliced run's: {same}", flush=True)

    def mmm(v):
        return f"{np.median(v):8.3f} [{min(v):8.3f} - {max(v):8.3f}]"
    for name, _ in ways:
        clips_b, feat_b = pcie[name]
        tail = "" if held[name] is None else f" | held tails {held[name] / 2 ** 20:.1f} MiB at most, {slices[name]} slices"
        print(f"{name:22s}: wall {mmm(wall[name])} s | to the host {clips_b / 1e6:.1f} MB of clips + {feat_b / 1e6:.1f} MB of features{tail}", flush=True)
        labels = sorted({k for r in kern[name] for k in r})
        print(" " * 24 + " | ".join(f"{k} {mmm([r.get(k, 0.0) for r in kern[name]])} ms" for k in labels), flush=True)
    ctx.close()
    if a.dir is None:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
