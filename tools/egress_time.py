"""Getting a denoised corpus off the device and into WAV files: fvad_egress into mapped files against the only way
there was before it, on synthetic lanes standing in for denoised audio.
  --streams mono f32 lanes of --hours hours on the device (config 4's corpus shape, 21 x 2 h; fewer if host memory or the free
  space of --dir does not allow, said so).  After one warm-up of each way, the ways alternate --repeats times; printed per way:
  the median [min - max] wall time and the PCIe bytes it moves --
    (a) run_denoise's export step, per format (pcm16, pcm24, f32): every file created at its final size with its header and
        mapped (simulator._DenoisedFile), one fvad_egress over all of them, the maps dropped;
    (b) the way before: the f32 lanes copied back (Context.to_host) and fvad_wav_write per stream, as f32 and as PCM16 (its
        libsndfile rule: other bytes than (a)'s PCM16, the same amount of work); there is no 24-bit form;
  the ratio (b) / (a) per format by the medians; and for (a) the `egress` kernel's device-event time summed over the call's
  batches and its HBM bytes (lane bytes read + file bytes written) per second, beside the 6.29 TB/s copy rate DESIGN uses.
  The f32 files of (a) and (b) are compared byte for byte once (filecmp); a difference ends the tool.  Files are removed after
  every way.  Neither way waits for the disk: both leave their pages to the page cache.
timeout 1100 python tools/egress_time.py [--streams 21] [--hours 2] [--repeats 3] [--dir DIR] [--json PATH]"""
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
    work = tempfile.mkdtemp(prefix="egress_time_", dir=a.dir)
    # way (b) holds the f32 copy of every lane and fvad_wav_write's image of one file; the f32 files of both ways lie side by
    # side once (the comparison), in the page cache or on the disk of --dir
    S = a.streams
    avail, free = mem_available(), shutil.disk_usage(work).free
    limits = [S] + ([int(0.45 * avail // (n * 4 * 2 + 1))] if avail is not None else []) + [int(0.8 * free // (n * 4 * 2 + 1))]
    if min(limits) < S:
        S = max(1, min(limits))
        print(f"host memory {0 if avail is None else avail / 1e9:.0f} GB available, {free / 1e9:.0f} GB free in {work}: timing {S} of {a.streams} streams", flush=True)
    ctx = fv.Context(0)
    d_lanes = ctx.device_alloc(S * n * 4)
    insts = [{"name": f"s{i:02d}"} for i in range(S)]
    res = {"streams_asked": a.streams, "streams": S, "hours": a.hours, "n_frames": n, "repeats": a.repeats, "ways": {}}
    try:
        one = np.tile((np.random.default_rng(5).standard_normal(48000) * 0.2).astype(np.float32), -(-n // 48000))[:n]
        for i in range(S):   # (every lane its own device pages; the values repeat, the kernel does not care)
            ctx.to_device(d_lanes + i * n * 4, np.roll(one, 997 * i))
        del one

        def way_a(fmt_name):
            def run():
                out = os.path.join(work, "a-" + fmt_name)
                os.makedirs(out, exist_ok=True)
                files = [sim._DenoisedFile(out, inst, fmt_name, 1, n) for inst in insts]
                try:
                    ctx.egress([f.sink(0, n, i, 0) for i, f in enumerate(files)], d_lanes=d_lanes, n_lanes=S, lane_stride=n, n_samples=n,
                               out=[f.map for f in files])
                finally:
                    for f in files:
                        f.close()
                return out
            return run

        def way_b(pcm16):
            def run():
                out = os.path.join(work, "b-" + ("pcm16" if pcm16 else "f32"))
                os.makedirs(out, exist_ok=True)
                host = ctx.to_host(np.empty((S, n), np.float32), d_lanes)
                for i, inst in enumerate(insts):
                    fv.wav_write(os.path.join(out, inst["name"] + "-denoised.wav"), host[i:i + 1], pcm16=pcm16)
                return out
            return run

        B = {"pcm16": 2, "pcm24": 3, "f32": 4}
        ways = {f"a: fvad_egress -> {k}": (way_a(k), S * n * B[k], S * n * (4 + B[k])) for k in B}
        ways["b: to_host + fvad_wav_write f32"] = (way_b(False), S * n * 4, None)
        ways["b: to_host + fvad_wav_write pcm16"] = (way_b(True), S * n * 4, None)
        walls, kernel = {k: [] for k in ways}, {k: [] for k in ways}
        print(f"{S} x {n / 48000 / 3600:.2f} h mono f32 lanes, {S * n * 4 / 1e9:.2f} GB on the device; files in {work}", flush=True)
        ctx.enable_timing(True)
        for rnd in range(a.repeats + 1):   # round 0: the warm-up, and the comparison of the f32 files
            made = {}
            for name, (fn, _, hbm) in ways.items():
                ctx.kernel_times()
                t0 = time.perf_counter()
                made[name] = fn()
                wall = time.perf_counter() - t0
                kt = ctx.kernel_times().get("egress", 0.0) * 1e-3
                if rnd:
                    walls[name].append(wall)
                    kernel[name].append(kt)
                    print(f"  round {rnd} ({name}) {wall:.3f} s", flush=True)
                if rnd or "f32" not in name:
                    shutil.rmtree(made[name])
            if rnd == 0:
                x, y = made["a: fvad_egress -> f32"], made["b: to_host + fvad_wav_write f32"]
                names = sorted(os.listdir(x))
                match, mismatch, errors = filecmp.cmpfiles(x, y, names, shallow=False)
                if match != names or names != sorted(os.listdir(y)):
                    raise SystemExit(f"the f32 files of fvad_egress differ from fvad_wav_write's: {mismatch} {errors}")
                shutil.rmtree(x)
                shutil.rmtree(y)
        ctx.enable_timing(False)
        for name, (_, pcie, hbm) in ways.items():
            line = f"  ({name:34s}) {fmt(walls[name])}   PCIe {pcie / 1e9:7.2f} GB"
            entry = {"wall_s": walls[name], "pcie_bytes": pcie}
            if hbm is not None:
                k = float(np.median(kernel[name]))
                line += f"   egress kernel {k * 1e3:8.2f} ms [{min(kernel[name]) * 1e3:.2f} - {max(kernel[name]) * 1e3:.2f}], {hbm / 1e9:.2f} GB of HBM traffic = " \
                        f"{hbm / k / 1e12:.2f} TB/s ({100 * hbm / k / COPY_RATE:.0f}% of the {COPY_RATE / 1e12:.2f} TB/s copy rate)"
                entry.update(kernel_s=kernel[name], hbm_bytes=hbm)
            print(line, flush=True)
            res["ways"][name] = entry
        for k, b in (("f32", "f32"), ("pcm16", "pcm16")):
            ratio = float(np.median(walls[f"b: to_host + fvad_wav_write {b}"]) / np.median(walls[f"a: fvad_egress -> {k}"]))
            res[f"b_over_a_{k}"] = ratio
            print(f"  (b) / (a), {k}: {ratio:.1f}x by the medians", flush=True)
    finally:
        ctx.device_free(d_lanes)
        ctx.close()
        shutil.rmtree(work, ignore_errors=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
