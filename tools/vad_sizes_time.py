"""Cost of a VAD sweep over the FFT size: one launch of machines on several frame clocks (fvad_vad_batch_run_device_sized) against
one single-size launch per size run one after another (fvad_vad_batch_run_device), on vad_sweep_time.py's device corpus (S mono
streams x H hours) with that tool's N configs at each size of --sizes.  Device events around the machines' kernels
(kernel timing "vad_machines"); each shape warmed up once, the forms alternated, --reps repetitions, median [min - max].  The
sized launch's machines are checked bit for bit against the single-size ones (segments, audits, lazy statistics), with the
default size-major lane order and with the caller's order (context option vad_size_order).  Then simulator.run_grid wall time
for one grid with "fft_size": [sizes] against one run_grid per size (--grid-streams stereo PCM16 streams of --grid-minutes).
python tools/vad_sizes_time.py [--streams 21] [--hours 2] [--configs 64,256] [--sizes 512,1024,2048] [--reps 3]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from conftest import load_package  # noqa: E402
from vad_sweep_time import device_corpus, make_configs  # noqa: E402


def med(xs):
    return f"{np.median(xs):8.1f} [{min(xs):8.1f} - {max(xs):8.1f}]"


def results(sw, S, cs):
    return [(sw.segments(c), [sw.audit(s, c) for s in range(S)], [sw.lazy_stats(s, c) for s in range(S)]) for c in cs]


def machines(fv, ctx, S, cfgs, sizes, n_chunks, rms, d_den, L, torch, reps):
    """(sized ms list, per-size-sum ms list, caller-order ms list, bit-identical)"""
    chunk = 24000
    N = len(cfgs)
    dev = torch.device("cuda:0")
    # the sized batch and its band blocks: one band-sum pass per size
    sized = fv.VadSweepSized(S, cfgs * len(sizes), [F for F in sizes for _ in cfgs])
    blocks = sized.size_blocks()
    n_bands = sum(len(b) for _, _, b in blocks)
    stride = n_chunks * chunk // min(sizes)
    band = torch.zeros((n_bands, S, stride), dtype=torch.float32, device=dev)
    for F, j0, bins in blocks:
        ctx.band_sums_device(d_den, S, L, L, bins, band.data_ptr() + j0 * S * stride * 4, stride, fft_size=F)
    nf_sized = [[n_chunks * chunk // F] * S for F in sized.sizes]
    singles = []
    for g, F in enumerate(sizes):   # each size's create_sweep batch reads the sized batch's blocks of its size
        sw = fv.VadSweep(S, cfgs, fft_size=F)
        bins, _ = sw.bands()
        js = [blocks[g][1] + blocks[g][2].index(b) for b in bins]
        bb = torch.stack([band[j, :, :n_chunks * chunk // F] for j in js]).contiguous()
        singles.append((sw, bb, F))
    torch.cuda.synchronize()

    def run_sized():
        ctx.kernel_times()
        sized.run_device(ctx, band.data_ptr(), stride, nf_sized, rms, [n_chunks] * S)
        return ctx.kernel_times().get("vad_machines", float("nan"))

    def run_singles():
        t = 0.0
        for sw, bb, F in singles:
            ctx.kernel_times()
            nf = n_chunks * chunk // F
            sw.run_device(ctx, bb.data_ptr(), nf, [nf] * S, rms, [n_chunks] * S)
            t += ctx.kernel_times().get("vad_machines", float("nan"))
        return t

    run_sized()   # warm-up, once per shape
    run_singles()
    ts, tm, tc = [], [], []
    for _ in range(reps):
        ts.append(run_sized())
        tm.append(run_singles())
    same = results(sized, S, range(len(sizes) * N)) == [r for sw, _, _ in singles for r in results(sw, S, range(N))]
    ctx.set_option("vad_size_order", "caller")
    try:
        run_sized()
        for _ in range(reps):
            tc.append(run_sized())
        same = same and results(sized, S, range(len(sizes) * N)) == [r for sw, _, _ in singles for r in results(sw, S, range(N))]
    finally:
        ctx.set_option("vad_size_order", None)
    sized.close()
    for sw, _, _ in singles:
        sw.close()
    return ts, tm, tc, same


def grid_times(pkg, ctx, sizes, n_streams, minutes, reps):
    fv, sim = pkg.binding, pkg.simulator
    grid = {"axes": {"speech_threshold_factor": [3.0, 5.0, 7.0, 10.0], "speech_min_freq": [300.0, 500.0],
                     "long_term_speech_avg_sec": [60.0, 180.0, 300.0, 600.0]}}
    with tempfile.TemporaryDirectory() as tmp:
        insts = []
        for i in range(n_streams):
            pcm, labels = pkg.synth.make_stream(minutes * 60.0, seed=700 + i, n_channels=2)
            fv.wav_write(os.path.join(tmp, f"s{i}.wav"), pcm, pcm16=True)
            with open(os.path.join(tmp, f"s{i}.txt"), "w") as f:
                f.write(pkg.synth.labels_to_audacity(labels))
            insts.append({"name": f"s{i}", "audio_path": f"s{i}.wav", "ref_path": f"s{i}.txt"})
        plans = {}
        for F in sizes:
            plans[F] = os.path.join(tmp, f"plan{F}.json")
            with open(plans[F], "w") as f:
                json.dump({"instances": insts, "config": {"vad_config": {"fft_size": F}}}, f)
        kw = {"vad_on": "device", "out": None, "ctx": ctx}
        one, three = [], []
        res1 = res3 = None
        for r in range(reps + 1):   # (the first of each: warm-up)
            t0 = time.perf_counter()
            res1 = sim.run_grid(plans[1024], dict(grid, fft_size=list(sizes)), **kw)
            t1 = time.perf_counter()
            res3 = [sim.run_grid(plans[F], grid, **kw) for F in sizes]
            t2 = time.perf_counter()
            if r:
                one.append(t1 - t0)
                three.append(t2 - t1)
        same = np.array_equal(res1["stats"].view(np.uint32), np.concatenate([r["stats"] for r in res3]).view(np.uint32))
        return one, three, same, len(res1["configs"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--configs", default="64,256")
    ap.add_argument("--sizes", default="512,1024,2048")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--grid-streams", type=int, default=6)
    ap.add_argument("--grid-minutes", type=float, default=20.0)
    a = ap.parse_args()
    import torch
    pkg = load_package()
    fv = pkg.binding
    ctx = fv.Context(0)
    ctx.load_synth(7)
    sizes = [int(x) for x in a.sizes.split(",")]
    S = a.streams
    audio, rms, n_chunks = device_corpus(S, a.hours, a.seed)
    L = n_chunks * 24000
    print(f"{S} streams x {a.hours:g} h, mono, sizes {sizes}; machine kernels, ms, median [min - max] of {a.reps}", flush=True)
    ctx.enable_timing(True)
    for N in [int(x) for x in a.configs.split(",")]:
        cfgs = make_configs(N, a.seed + N)
        ts, tm, tc, same = machines(fv, ctx, S, cfgs, sizes, n_chunks, rms, audio.data_ptr(), L, torch, a.reps)
        print(f"N={N:4d} x {len(sizes)} sizes: one sized launch {med(ts)} (caller order {med(tc)}) | {len(sizes)} single-size "
              f"launches {med(tm)} | ratio {np.median(ts) / np.median(tm):5.2f} | bit-identical: {same}", flush=True)
    ctx.enable_timing(False)
    del audio
    torch.cuda.empty_cache()
    if a.grid_streams:
        one, three, same, n = grid_times(pkg, ctx, sizes, a.grid_streams, a.grid_minutes, a.reps)
        print(f"run_grid, {a.grid_streams} stereo PCM16 x {a.grid_minutes:g} min, {n} configs: one grid over {sizes} "
              f"{med([x * 1e3 for x in one])} ms | one run_grid per size {med([x * 1e3 for x in three])} ms | "
              f"stats bit-identical: {same}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
