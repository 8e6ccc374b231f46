"""A/B of the shared-trigger form of the device VAD sweep (context option vad_trigger "shared") against the per-config machines, on
vad_sweep_time.py's device corpus (21 mono two-hour streams by default).  A grid is K trigger keys (vad_sweep_time.make_configs(K))
x an (open, gap, duration) product of N / K combinations, run under vad_chain "coop" with the ring and with the table averages,
segment room given from the start.  Protocol of DESIGN section 7.1: kernel times by device events; per shape one warm-up, then
--reps rounds that alternate "config" and "shared" in one process; median [min - max].  Printed per shape: the per-config
machines' kernel, the emitting machines, the finishing kernel on its own, their sum, the table kernels (both forms run them
first), the bytes of the bits, and whether the two forms gave the same segments, audits and lazy statistics.  --only-config runs the per-config side
alone (a build without the option: the parent's side of the A/B).  --overflow SHAPE adds one run of that shape with room for two
segments: the machines launch once, the finishing kernel again and again (trigger_launches).
python tools/vad_trigger_time.py [--streams 21] [--hours 2] [--shapes 4096x256,1024x64,256x256] [--reps 3] [--overflow 1024x64]"""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from conftest import load_package  # noqa: E402
from vad_sweep_time import device_corpus, make_configs  # noqa: E402

FINISH_FIELDS = ("min_consecutive_sec_to_open", "max_speech_gap_sec", "min_vad_duration_sec")


def finishing(n):
    """n (open, gap, duration) combinations: a product of up to 4 x 4 x 4 values, its first n"""
    prod = itertools.product([0.0, 0.05, 0.1, 0.2], [0.5, 1.0, 2.0, 3.0], [0.2, 0.5, 0.7, 1.0])
    out = [dict(zip(FINISH_FIELDS, v)) for v in prod]
    assert n <= len(out), n
    return out[:n]


def grid_configs(N, K, seed):
    """K keys x N / K finishing combinations, combination-major (a key's configs are K apart in the caller's order)"""
    keys = [{k: v for k, v in c.items() if k not in FINISH_FIELDS} for c in make_configs(K, seed)]
    return [dict(t, **f) for f in finishing(N // K) for t in keys]


def stat(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:8.1f} [{v[0]:8.1f} - {v[-1]:8.1f}]" if v else "       -"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--shapes", default="4096x256,1024x64,256x256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--avgs", default="ring,table")
    ap.add_argument("--only-config", action="store_true")
    ap.add_argument("--overflow", default=None)
    ap.add_argument("--seg-cap", type=int, default=2048, help="segment room per machine, given from the start")
    a = ap.parse_args()
    import torch
    pkg = load_package()
    fv = pkg.binding
    ctx = fv.Context(0)
    ctx.enable_timing(True)
    S = a.streams
    audio, rms, n_chunks = device_corpus(S, a.hours, a.seed)
    L = audio.shape[1]
    nf = L // 1024
    forms = ["config"] if a.only_config else ["config", "shared"]
    shapes = [tuple(int(x) for x in sh.split("x")) for sh in a.shapes.split(",")]
    jobs = [(N, K, None) for N, K in shapes]
    if a.overflow and not a.only_config:
        N, K = (int(x) for x in a.overflow.split("x"))
        jobs.append((N, K, 2))
    ctx.set_option("vad_chain", "coop")
    for N, K, room in jobs:
        cfgs = grid_configs(N, K, a.seed + K)
        sw = fv.VadSweep(S, cfgs)
        bins, _ = sw.bands()
        band = torch.empty((len(bins), S, nf), dtype=torch.float32, device=audio.device)
        ctx.band_sums_device(audio.data_ptr(), S, L, L, bins, band.data_ptr(), nf)
        torch.cuda.synchronize()
        n_keys = len(sw.trigger_keys()[1]) if hasattr(sw, "trigger_keys") else K
        ctx.set_option("vad_seg_cap", str(room if room else min(nf // 4 + 1, a.seg_cap)))
        for avgs in a.avgs.split(","):
            ctx.set_option("vad_avgs", avgs)
            ms = {f: {"vad_machines": [], "vad_finish": [], "tables": []} for f in forms}
            kept, info = {}, {}
            for rep in range(-1, 1 if room else a.reps):   # (-1: the warm-up, not kept)
                for f in forms:
                    if not a.only_config:
                        ctx.set_option("vad_trigger", f)
                    ctx.kernel_times()
                    l0 = sw.trigger_launches() if not a.only_config else (0, 0)
                    sw.run_device(ctx, band.data_ptr(), nf, [nf] * S, rms, [n_chunks] * S)
                    kt = ctx.kernel_times()
                    if avgs == "table":   # the two table kernels, which both forms run before their machines
                        kt["tables"] = kt.get("vad_minvol", 0.0) + kt.get("vad_avgs", 0.0)
                    if not a.only_config:
                        assert sw.trigger_form() == (2 if f == "shared" else 1), (f, sw.trigger_form())
                        l1 = sw.trigger_launches()
                        info[f] = (sw.trigger_bytes(), l1[0] - l0[0], l1[1] - l0[1])
                    if rep >= 0:
                        for k in ms[f]:
                            if k in kt:
                                ms[f][k].append(kt[k])
                    if rep == 0:
                        kept[f] = ([sw.segments(c) for c in range(0, N, max(N // 64, 1))],
                                   [sw.audit(s, c) for s in range(S) for c in range(N)],
                                   [sw.lazy_stats(s, c) for s in range(S) for c in range(N)])
            same = "-" if a.only_config else str(kept["shared"] == kept["config"])
            print(f"N={N} K={K} keys={n_keys} avgs={avgs} room={room or 'full'}  (ms, median [min - max])")
            print(f"  config: machines {stat(ms['config']['vad_machines'])}  tables {stat(ms['config']['tables'])}")
            if not a.only_config:
                m, fi = ms["shared"]["vad_machines"], ms["shared"]["vad_finish"]
                both = [x + y for x, y in zip(m, fi)]
                print(f"  shared: machines {stat(m)}  finish {stat(fi)}  sum {stat(both)}  tables {stat(ms['shared']['tables'])}")
                print(f"  bits {info['shared'][0] / 1e6:.1f} MB, launches of the last run: machines {info['shared'][1]}, finish {info['shared'][2]}; "
                      f"same results: {same}")
            sys.stdout.flush()
        ctx.set_option("vad_avgs", None)
        ctx.set_option("vad_seg_cap", None)
        if not a.only_config:
            ctx.set_option("vad_trigger", None)
        sw.close()
        del band
    ctx.close()


if __name__ == "__main__":
    main()
