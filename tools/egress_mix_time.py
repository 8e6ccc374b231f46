"""Writing the residual beside the denoised recording ("The original beside the denoised"): fvad_egress_mix into mapped
files against fvad_egress, the single-source way of the parent commit, in one process on the same lanes.
  2 x --streams mono f32 lanes of --hours hours of synthetic noise on the device, one set standing in for the original audio and
  one for the denoised (config 4's corpus shape, 21 x 2 h, twice; fewer if host memory or the free space of --dir does not allow,
  said so).  After one warm-up of each way, the ways alternate --repeats times; printed per way: the median [min - max] wall time,
  the PCIe bytes it moves, the kernel's device-event time summed over the call's batches and its HBM bytes (lane bytes read +
  file bytes written) per second --
    (mix) run_denoise's export step for the kind "residual", as pcm16 and as f32: every file created at its final size with its
          header and mapped (simulator._DenoisedFile), one fvad_egress_mix with the weights (1, -1) and the harness's pairing
          (orig_zeros = fvad_nsnet2_delay(48000)) over all of them, the maps dropped;
    (one) the same step for the denoised kind: one fvad_egress over the denoised lanes;
  and the ratios (mix) / (one) of wall and kernel time beside the ratio of the HBM bytes the two kernels move.
  Files are removed after every way.  Neither way waits for the disk: both leave their pages to the page cache.
timeout 900 python tools/egress_mix_time.py [--streams 21] [--hours 2] [--repeats 3] [--dir DIR] [--json PATH]"""
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

COPY_RATE = 6.29e12   # bytes/s: the device copy rate DESIGN §3 measures against


def mem_available():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return None


def fmt(ts):
    return f"{np.median(ts):8.3f} s [{min(ts):.3f} - {max(ts):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a fresh temporary directory)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = load_package()
    fv, sim = pkg.binding, pkg.simulator
    n = int(a.hours * 3600 * 48000) // 24000 * 24000   # whole chunks, as the denoised lanes are
    work = tempfile.mkdtemp(prefix="egress_mix_time_", dir=a.dir)
    S = a.streams
    avail, free = mem_available(), shutil.disk_usage(work).free   # one set of f32 files at a time, in the page cache or on --dir's disk
    limits = [S] + ([int(0.45 * avail // (n * 4 + 1))] if avail is not None else []) + [int(0.8 * free // (n * 4 + 1))]
    if min(limits) < S:
        S = max(1, min(limits))
        print(f"host memory {0 if avail is None else avail / 1e9:.0f} GB available, {free / 1e9:.0f} GB free in {work}: timing {S} of {a.streams} streams", flush=True)
    ctx = fv.Context(0)
    D = fv.nsnet2_delay(48000)
    d_orig, d_den = ctx.device_alloc(S * n * 4), ctx.device_alloc(S * n * 4)
    insts = [{"name": f"s{i:02d}"} for i in range(S)]
    res = {"streams_asked": a.streams, "streams": S, "hours": a.hours, "n_frames": n, "repeats": a.repeats, "delay": D, "ways": {}}
    try:
        one = np.tile((np.random.default_rng(5).standard_normal(48000) * 0.2).astype(np.float32), -(-n // 48000))[:n]
        for i in range(S):   # (every lane its own device pages; the values repeat, the kernels do not care)
            ctx.to_device(d_orig + i * n * 4, np.roll(one, 997 * i))
            ctx.to_device(d_den + i * n * 4, np.roll(one, 997 * i + D) * np.float32(0.7))
        del one

        def way(kind, fmt_name):
            def run():
                out = os.path.join(work, f"{kind}-{fmt_name}")
                os.makedirs(out, exist_ok=True)
                files = [sim._DenoisedFile(out, inst, fmt_name, 1, n, kind=kind) for inst in insts]
                try:
                    if kind == "denoised":
                        ctx.egress([f.sink(0, n, i, 0) for i, f in enumerate(files)], d_lanes=d_den, n_lanes=S, lane_stride=n, n_samples=n,
                                   out=[f.map for f in files])
                    else:
                        w_orig, w_den = sim._kind_weights(kind, None)
                        ctx.egress_mix([f.sink_mix(0, n, i, 0, 0, min(D, n)) for i, f in enumerate(files)], w_orig, w_den, d_orig=d_orig, orig_stride=n,
                                       orig_samples=n, d_den=d_den, den_stride=n, den_samples=n, n_lanes=S, out=[f.map for f in files])
                finally:
                    for f in files:
                        f.close()
                return out
            return run

        B = {"pcm16": 2, "f32": 4}
        ways = {}
        for k in B:   # name -> (run, PCIe bytes, HBM bytes, the kernel's name)
            ways[f"mix: fvad_egress_mix residual -> {k}"] = (way("residual", k), S * n * B[k], S * (n * 4 + (n - min(D, n)) * 4 + n * B[k]), "egress_mix")
            ways[f"one: fvad_egress denoised -> {k}"] = (way("denoised", k), S * n * B[k], S * n * (4 + B[k]), "egress")
        walls, kernel = {k: [] for k in ways}, {k: [] for k in ways}
        print(f"2 x {S} x {n / 48000 / 3600:.2f} h mono f32 lanes, {2 * S * n * 4 / 1e9:.2f} GB on the device; files in {work}", flush=True)
        ctx.enable_timing(True)
        for rnd in range(a.repeats + 1):   # round 0: the warm-up
            for name, (fn, _, _, kname) in ways.items():
                ctx.kernel_times()
                t0 = time.perf_counter()
                made = fn()
                wall = time.perf_counter() - t0
                kt = ctx.kernel_times().get(kname, 0.0) * 1e-3
                if rnd:
                    walls[name].append(wall)
                    kernel[name].append(kt)
                    print(f"  round {rnd} ({name}) {wall:.3f} s, kernel {kt * 1e3:.2f} ms", flush=True)
                shutil.rmtree(made)
        ctx.enable_timing(False)
        for name, (_, pcie, hbm, kname) in ways.items():
            k = float(np.median(kernel[name]))
            print(f"  ({name:40s}) {fmt(walls[name])}   PCIe {pcie / 1e9:7.2f} GB   {kname} kernel {k * 1e3:8.2f} ms "
                  f"[{min(kernel[name]) * 1e3:.2f} - {max(kernel[name]) * 1e3:.2f}], {hbm / 1e9:.2f} GB of HBM traffic = {hbm / k / 1e12:.2f} TB/s "
                  f"({100 * hbm / k / COPY_RATE:.0f}% of the {COPY_RATE / 1e12:.2f} TB/s copy rate)", flush=True)
            res["ways"][name] = {"wall_s": walls[name], "pcie_bytes": pcie, "kernel_s": kernel[name], "hbm_bytes": hbm}
        for k in B:
            m, o = f"mix: fvad_egress_mix residual -> {k}", f"one: fvad_egress denoised -> {k}"
            r = {"wall": float(np.median(walls[m]) / np.median(walls[o])), "kernel": float(np.median(kernel[m]) / np.median(kernel[o])),
                 "hbm_bytes": ways[m][2] / ways[o][2]}
            res[f"mix_over_one_{k}"] = r
            print(f"  (mix) / (one), {k}: wall {r['wall']:.2f}x, kernel {r['kernel']:.2f}x, HBM bytes {r['hbm_bytes']:.2f}x, by the medians", flush=True)
    finally:
        ctx.device_free(d_orig)
        ctx.device_free(d_den)
        ctx.close()
        shutil.rmtree(work, ignore_errors=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
