"""simulator.run_grid over several contexts: the instances of a plan dealt round-robin to one context and one host thread per
share ("Grids over several devices").
  On a plan of --streams mono PCM16 streams of --hours hours (synthetic noise with speech-like bursts and their labels), times
  run_grid with the context lists [0], [0, 0] and, where more GPUs are visible, [0 .. n-1] (caller-owned contexts, synthetic
  weights, reproducible = 1) on two grids: --configs configs unsliced, and --halving-configs configs sliced in
  --slice-chunks-chunk slices with successive halving (eta --eta, --rungs rungs).  One warm-up run of every list, then
  --repeats rounds that alternate the lists; per list the median and [min - max] of the wall time, the median stage times
  (summed over the shares), the median wall time of each share and device_bytes_per_share.  Every timed run's statistics
  must equal the [0] run's bit for bit (reproducible contexts); a difference ends the tool with an error.
  On one GPU, [0, 0] only shows whether two contexts overlap one context's machines with the other's denoising.
python tools/vad_grid_devices_time.py [--streams 8] [--hours 2] [--configs 1024] [--halving-configs 16384] [--eta 4] [--rungs 2]
                                      [--slice-chunks 1024] [--repeats 3] [--plan-dir DIR] [--skip-unsliced] [--skip-halving]"""
import argparse
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


def write_mono_corpus(fv, d, n_streams, hours, seed):
    """mono PCM16 streams: noise with bursts of louder noise (their labels); returns the plan path"""
    rng = np.random.default_rng(seed)
    n = int(hours * 3600 * 48000)
    insts = []
    for i in range(n_streams):
        t_on, labels, x = np.zeros(n // 1024 + 1, np.float32), [], rng.uniform(0, 3)
        while x < n / 48000:
            dur = rng.uniform(0.5, 5.0)
            labels.append((x, min(x + dur, n / 48000)))
            t_on[int(x * 48000 / 1024):int((x + dur) * 48000 / 1024)] = 1
            x += dur + rng.uniform(1.0, 15.0)
        pcm = rng.standard_normal((1, n), dtype=np.float32)
        pcm *= 0.01 + 0.2 * np.repeat(t_on, 1024)[:n]
        fv.wav_write(os.path.join(d, f"s{i}.wav"), pcm, pcm16=True)
        del pcm
        with open(os.path.join(d, f"s{i}.txt"), "w") as f:
            f.writelines(f"{a:.4f}\t{b:.4f}\tspeech\n" for a, b in labels)
        insts.append({"name": f"s{i}", "audio_path": f"s{i}.wav", "ref_path": f"s{i}.txt"})
    with open(os.path.join(d, "plan.json"), "w") as f:
        json.dump({"instances": insts}, f)
    return os.path.join(d, "plan.json")


def grid_of(n_configs):
    """a grid of n_configs configs (a power of two from 16 on) over four axes"""
    k = int(round(np.log2(n_configs)))
    assert 2 ** k == n_configs and k >= 4
    a = [2 ** (k // 4 + (1 if j < k % 4 else 0)) for j in range(4)]
    return {"base": {},
            "axes": {"speech_threshold_factor": np.linspace(1.5, 12.0, a[0]).round(3).tolist(),
                     "long_term_speech_avg_sec": np.linspace(10.0, 300.0, a[1]).round(1).tolist(),
                     "min_vad_duration_sec": np.linspace(0.1, 1.5, a[2]).round(3).tolist(),
                     "max_speech_gap_sec": np.linspace(0.25, 4.0, a[3]).round(3).tolist()}}


def fmt(xs):
    return f"{np.median(xs):7.2f} s [{min(xs):.2f} - {max(xs):.2f}]"


def time_lists(sim, plan, grid, lists, kw, repeats, label):
    print(f"{label}", flush=True)
    ref = None
    runs = {name: [] for name in lists}
    for rnd in range(repeats + 1):   # round 0: the warm-up
        for name, ctxs in lists.items():
            t0 = time.perf_counter()
            r = sim.run_grid(plan, grid, ctx=ctxs, out=None, **kw)
            wall = time.perf_counter() - t0
            if ref is None:
                ref = r["stats"]
            if not np.array_equal(r["stats"].view(np.uint32), ref.view(np.uint32)):
                raise SystemExit(f"{label}: the statistics of {name} (round {rnd}) differ from those of [0]")
            if rnd:
                runs[name].append((wall, r))
    for name, rs in runs.items():
        walls = [w for w, _ in rs]
        stages = {k: np.median([r["times"].get(k, 0.0) for _, r in rs]) for k in rs[0][1]["times"]}
        shares = [np.median([r["share_times"][s]["wall"] for _, r in rs]) for s in range(len(rs[0][1]["share_times"]))]
        dbs = rs[0][1]["device_bytes_per_share"]
        extra = ""
        if "survivors" in rs[0][1]:
            extra = f", {len(rs[0][1]['survivors'])} survivors"
        print(f"  {name:>14}: wall {fmt(walls)}; stages (summed over shares) "
              + ", ".join(f"{k} {v:.2f} s" for k, v in stages.items())
              + "; per share " + ", ".join(f"{w:.2f}" for w in shares) + " s"
              + ("; device_bytes per share " + ", ".join(f"{b / 2**20:.0f}" for b in dbs) + " MiB" if dbs[0] is not None else "")
              + extra, flush=True)
    print(f"  statistics of every timed run equal to [0]'s: yes", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--configs", type=int, default=1024)
    ap.add_argument("--halving-configs", type=int, default=16384)
    ap.add_argument("--eta", type=int, default=4)
    ap.add_argument("--rungs", type=int, default=2)
    ap.add_argument("--slice-chunks", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--plan-dir", default=None, help="write (or reuse) the corpus here instead of a temporary directory")
    ap.add_argument("--skip-unsliced", action="store_true")
    ap.add_argument("--skip-halving", action="store_true")
    a = ap.parse_args()
    import torch
    n_gpus = torch.cuda.device_count()
    pkg = load_package()
    fv, sim = pkg.binding, pkg.simulator
    d = a.plan_dir or tempfile.mkdtemp(prefix="grid_devices_")
    ctxs = []
    try:
        plan = os.path.join(d, "plan.json")
        if not os.path.exists(plan):
            t0 = time.perf_counter()
            os.makedirs(d, exist_ok=True)
            plan = write_mono_corpus(fv, d, a.streams, a.hours, a.seed)
            print(f"corpus written in {time.perf_counter() - t0:.1f} s", flush=True)
        n_ctx = max(2, n_gpus)
        for dev in [0, 0] + list(range(1, n_gpus)):
            c = fv.Context(dev)
            c.load_synth(7)
            c.set_option("reproducible", "1")
            ctxs.append(c)
        lists = {"[0]": [ctxs[0]], "[0, 0]": ctxs[:2]}
        if n_gpus > 1:
            lists[f"[0 .. {n_gpus - 1}]"] = [ctxs[0]] + ctxs[2:]
        print(f"{a.streams} mono PCM16 streams x {a.hours:g} h, {n_gpus} GPU(s) visible, {n_ctx} context(s), reproducible; "
              f"median and [min - max] of {a.repeats} runs after one warm-up, the lists alternating", flush=True)
        if not a.skip_unsliced:
            time_lists(sim, plan, grid_of(a.configs), lists, dict(vad_on="device", score_on="device"), a.repeats,
                       f"[1] {a.configs} configs, unsliced, device machines and scoring")
        if not a.skip_halving:
            time_lists(sim, plan, grid_of(a.halving_configs), lists,
                       dict(vad_on="device", score_on="device", slice_chunks=a.slice_chunks, halving_eta=a.eta,
                            halving_rungs=a.rungs), a.repeats,
                       f"[2] {a.halving_configs} configs, {a.slice_chunks}-chunk slices, halving eta {a.eta}, {a.rungs} rungs")
    finally:
        for c in ctxs:
            c.close()
        if not a.plan_dir:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
