"""simulator.run_grid in time slices with and without overlap ("Machines beside the next slice's denoising"):
  overlap=True runs a slice's VAD machines on the context's second stream beside the next slice's reading and denoising.
  On vad_grid_devices_time.py's corpus (--streams mono PCM16 streams of --hours hours, synthetic weights, reproducible = 1) and
  its two grids, both in --slice-chunks-chunk slices -- --configs configs, and --halving-configs configs with successive halving
  (eta --eta, --rungs rungs) -- times run_grid with overlap off and on, alternated: one warm-up each, then --repeats rounds;
  per mode the median and [min - max] of the wall time, the median stage times, device_bytes, and fvad_ctx_ws_fallbacks
  before and after.  With overlap on it also prints the bound the design can reach, max(denoise + bands, machines) plus the
  first slice's denoising and the last slice's machines (estimated as one slice's share of each, from the overlap-off stage
  times).  Every timed run's statistics must equal the first run's bit for bit; a difference ends the tool with an error.
  Copied into a checkout whose run_grid has no overlap argument (the parent commit: the yardstick of the timing claim), it
  times that checkout's sliced run_grid alone.
python tools/vad_overlap_time.py [--streams 8] [--hours 2] [--configs 1024] [--halving-configs 16384] [--eta 4] [--rungs 2]
                                 [--slice-chunks 1024] [--repeats 3] [--plan-dir DIR] [--skip-plain] [--skip-halving]"""
import argparse
import inspect
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
from vad_grid_devices_time import fmt, grid_of, write_mono_corpus  # noqa: E402


def time_modes(sim, ctx, plan, grid, modes, kw, repeats, label):
    print(label, flush=True)
    ref = None
    runs = {name: [] for name in modes}
    for rnd in range(repeats + 1):   # round 0: the warm-up
        for name, extra in modes.items():
            t0 = time.perf_counter()
            r = sim.run_grid(plan, grid, ctx=ctx, out=None, **kw, **extra)
            wall = time.perf_counter() - t0
            if ref is None:
                ref = r["stats"]
            if not np.array_equal(r["stats"].view(np.uint32), ref.view(np.uint32)):
                raise SystemExit(f"{label}: the statistics of {name} (round {rnd}) differ from the first run's")
            if rnd:
                runs[name].append((wall, r))
    med = {}
    for name, rs in runs.items():
        walls = [w for w, _ in rs]
        st = {k: float(np.median([r["times"].get(k, 0.0) for _, r in rs])) for k in rs[0][1]["times"]}
        med[name] = (float(np.median(walls)), min(walls), st, rs[0][1]["slices"])
        extra = f", {len(rs[0][1]['survivors'])} survivors" if "survivors" in rs[0][1] else ""
        print(f"  {name:>11}: wall {fmt(walls)}; stages " + ", ".join(f"{k} {v:.2f} s" for k, v in st.items())
              + f"; {rs[0][1]['slices']} slices; device_bytes {rs[0][1]['device_bytes'] / 2**20:.0f} MiB" + extra, flush=True)
    if "overlap on" in med and "overlap off" in med:
        _, _, st, n = med["overlap off"]
        front, back = st["denoise"] + st["bands"], st["machines"]
        bound = max(front, back) + front / n + back / n + st["scoring"] + st.get("retain", 0.0)
        print(f"  bound max(denoise + bands, machines) + one slice of each + scoring and retain: {bound:.2f} s; "
              f"overlap on reaches {med['overlap on'][0]:.2f} s, off {med['overlap off'][0]:.2f} s (min {med['overlap off'][1]:.2f} s)",
              flush=True)
    print("  statistics of every timed run equal to the first run's: yes", flush=True)


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
    ap.add_argument("--skip-plain", action="store_true")
    ap.add_argument("--skip-halving", action="store_true")
    a = ap.parse_args()
    pkg = load_package()
    fv, sim = pkg.binding, pkg.simulator
    modes = {"overlap off": {}}
    if "overlap" in inspect.signature(sim.run_grid).parameters:
        modes["overlap on"] = {"overlap": True}
    else:
        print("this checkout's run_grid has no overlap argument: its sliced run alone", flush=True)
    d = a.plan_dir or tempfile.mkdtemp(prefix="overlap_")
    ctx = None
    try:
        plan = os.path.join(d, "plan.json")
        if not os.path.exists(plan):
            t0 = time.perf_counter()
            os.makedirs(d, exist_ok=True)
            plan = write_mono_corpus(fv, d, a.streams, a.hours, a.seed)
            print(f"corpus written in {time.perf_counter() - t0:.1f} s", flush=True)
        ctx = fv.Context(0)
        ctx.load_synth(7)
        ctx.set_option("reproducible", "1")
        print(f"{a.streams} mono PCM16 streams x {a.hours:g} h, one context, reproducible; median and [min - max] of {a.repeats} "
              f"runs after one warm-up, the modes alternating; fvad_ctx_ws_fallbacks before: {ctx.ws_fallbacks()}", flush=True)
        kw = dict(vad_on="device", score_on="device", slice_chunks=a.slice_chunks)
        if not a.skip_plain:
            time_modes(sim, ctx, plan, grid_of(a.configs), modes, kw, a.repeats, f"[1] {a.configs} configs, {a.slice_chunks}-chunk slices")
        if not a.skip_halving:
            time_modes(sim, ctx, plan, grid_of(a.halving_configs), modes, dict(kw, halving_eta=a.eta, halving_rungs=a.rungs), a.repeats,
                       f"[2] {a.halving_configs} configs, {a.slice_chunks}-chunk slices, halving eta {a.eta}, {a.rungs} rungs")
        print(f"fvad_ctx_ws_fallbacks after: {ctx.ws_fallbacks()}", flush=True)
    finally:
        if ctx is not None:
            ctx.close()
        if not a.plan_dir:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
