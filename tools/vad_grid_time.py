"""Cost of scoring a VAD parameter sweep: S streams x H hours of synthetic denoised-like audio (vad_sweep_time.py's corpus: seeded
noise with speech-like bursts, generated on the device; the bursts are the reference labels), N configs (vad_sweep_time.py's).
Per N, after one untimed warm-up call:
  * how many times the call launches the machines (a machine closing more segments than the first launch has room for makes it
    launch them again) and the machine kernel's time per launch (device events inside fvad_vad_batch_run_device); where there
    are two, one more call with room for the largest count from the start (context option vad_seg_cap) times a single launch;
  * device scoring (the scoring kernel, kernels_eval.hip) against the host scorer fvad_vad_batch_score on T threads over the same
    segments, and for N <= --python-max against run_sweep's per-segment Python scoring (segments
    to Python tuples, seconds in a list comprehension, one fvad_stats_from_segments call per (stream, config));
  * the whole call: fvad_vad_batch_run_device with device scoring and keep_segments 0 against the call that brings the
    segments back plus the host scorer, alternating, --repeats times each (median [min .. max]);
  * bytes copied back by either call and the peak device memory of the lean one (free memory polled during the call);
  * device against host scores, bit for bit.
python tools/vad_grid_time.py [--streams 21] [--hours 2] [--configs 64,256,1024,4096] [--threads 16] [--python-max 256] [--repeats 3]"""
import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_package  # noqa: E402
from vad_sweep_time import make_configs  # noqa: E402

STAT = {"extrude_start": 5.0, "extrude_end": 10.0, "fill_gaps": 5.0}


class PeakMemory:
    """the lowest free device memory seen while the block runs, polled every 2 ms (hipMemGetInfo through torch)"""

    def __init__(self, torch):
        self.torch = torch

    def __enter__(self):
        self.base = self.low = self.torch.cuda.mem_get_info()[0]
        self.stop = False

        def poll():
            while not self.stop:
                self.low = min(self.low, self.torch.cuda.mem_get_info()[0])
                time.sleep(0.002)
        self.th = threading.Thread(target=poll)
        self.th.start()
        return self

    def __exit__(self, *exc):
        self.stop = True
        self.th.join()

    @property
    def peak_bytes(self):
        return self.base - self.low


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--configs", default="64,256,1024,4096")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--python-max", type=int, default=256)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    pkg = load_package()
    fv = pkg.binding
    ctx = fv.Context(0)
    chunk, F, FS = 24000, 1024, 48000
    n_chunks = int(a.hours * 3600 * FS) // chunk
    L = n_chunks * chunk
    nf = L // F
    S = a.streams
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    rng = np.random.default_rng(a.seed)
    audio = torch.empty((S, L), dtype=torch.float32, device=dev)
    refs = []
    for s in range(S):  # vad_sweep_time.py's streams; each burst is a label
        edges = np.cumsum(rng.uniform(0.5, 20.0, int(L / FS / 5) + 8)) * FS / F
        env = np.zeros(nf + 1, np.float32)
        labels = []
        for x in edges:
            i0 = int(x)
            if i0 >= nf:
                break
            i1 = min(nf, i0 + int(rng.uniform(0.5, 5.0) * FS / F))
            env[i0:i1] = 1.0
            labels.append((i0 * F / FS, i1 * F / FS))
        refs.append(labels)
        e = torch.from_numpy(env[:nf]).to(dev).repeat_interleave(F)
        audio[s] = torch.randn(L, generator=g, device=dev) * (0.01 + 0.2 * e)
        del e
    rms = torch.sqrt(torch.mean(audio.view(S, n_chunks, chunk) ** 2, dim=2)).cpu().numpy().astype(np.float32)
    torch.cuda.synchronize()
    d_den = audio.data_ptr()
    print(f"{S} streams x {a.hours:g} h ({nf} frames each), mono, fft 1024, {sum(len(r) for r in refs)} labels", flush=True)
    ctx.enable_timing(True)
    for N in [int(x) for x in a.configs.split(",")]:
        cfgs = make_configs(N, a.seed + N)
        scs = [{"ignore_shorter_than_sec": float(np.float32(c.get("min_vad_duration_sec", 0.7))), **STAT} for c in cfgs]
        M = S * N
        sw = fv.VadSweep(S, cfgs)
        bins, _ = sw.bands()
        band = torch.empty((len(bins), S, nf), dtype=torch.float32, device=dev)
        ctx.band_sums_device(d_den, S, L, L, bins, band.data_ptr(), nf)
        torch.cuda.synchronize()
        sw.set_references(refs, scs)

        def call(keep):
            """one fvad_vad_batch_run_device -> (wall s, machine kernel ms summed over its launches, scoring kernel ms)"""
            sw.keep_segments(keep)
            ctx.kernel_times()
            t0 = time.perf_counter()
            sw.run_device(ctx, band.data_ptr(), nf, [nf] * S, rms, [n_chunks] * S)
            wall = time.perf_counter() - t0
            kt = ctx.kernel_times()
            return wall, kt.get("vad_machines", float("nan")), kt.get("vad_score", float("nan"))

        # 1. untimed warm-up that keeps the segments: the per-machine counts, the device scores, the host and Python scorers
        call(True)
        dev_stats = np.stack([sw.config_stats(c) for c in range(N)])
        t0 = time.perf_counter()
        sw.score(a.threads)
        t_host = time.perf_counter() - t0
        same = np.array_equal(dev_stats.view(np.uint32), np.stack([sw.config_stats(c) for c in range(N)]).view(np.uint32))
        offs = (fv.sz * (S + 1))()
        n_segs, most = 0, 0
        for c in range(N):   # (the counts only: fvad_vad_batch_config_segments without a buffer fills the offsets)
            fv.lib().fvad_vad_batch_config_segments(sw.h, c, None, 0, offs)
            n_segs += offs[S]
            most = max(most, max(offs[s + 1] - offs[s] for s in range(S)))
        # the room of the first launch, as fvad_vad_batch_run_device sizes it; a machine that closes more segments makes the call
        # launch the machines a second time with room for the largest count
        cap0 = min(nf // 4 + 1, max(256, (512 << 20) // 24 // M))
        launches = 1 if most <= cap0 else 2
        cap = cap0 if launches == 1 else most
        bytes_lean = launches * M * 4 + M * (24 + 16 + 44)   # counts after each launch, audits, lazy statistics, scores
        bytes_keep = bytes_lean + cap * M * 24               # + every segment slot of the final launch
        t_py = None
        if N <= a.python_max:                                # the per-segment path run_sweep has
            t0 = time.perf_counter()
            py_stats = []
            for c in range(N):
                per = sw.segments(c)
                for s in range(S):
                    secs = [(float(np.float32(x[0]) / np.float32(FS)), float(np.float32(x[1]) / np.float32(FS))) for x in per[s]]
                    py_stats.append(fv.stats_from_segments(secs, refs[s], scs[c]))
            t_py = time.perf_counter() - t0
            py = np.stack([fv.single_stats_to_array(x) for x in py_stats]).reshape(N, S, -1)
            same = same and np.array_equal(py.view(np.uint32), dev_stats.view(np.uint32))
        # 2. timed: the lean call (device scoring, segments left on the device) and the call that brings the segments back
        #    followed by the host scorer, alternating, --repeats times each
        lean_t, keep_t, mach, score, ratio = [], [], [], [], []
        for _ in range(a.repeats):
            with PeakMemory(torch) as pm:
                w, km, ks = call(False)
            lean_t.append(w)
            mach.append(km / launches)
            score.append(ks)
            same = same and np.array_equal(np.stack([sw.config_stats(c) for c in range(N)]).view(np.uint32), dev_stats.view(np.uint32))
            w, km, _ = call(True)
            mach.append(km / launches)
            t0 = time.perf_counter()
            sw.score(a.threads)
            keep_t.append(w + time.perf_counter() - t0)
            ratio.append(keep_t[-1] / lean_t[-1])
        # 3. with room for the largest count from the start: one launch, the machine kernel's own time at this N
        single = ""
        if launches == 2:
            ctx.set_option("vad_seg_cap", str(most))
            try:
                w, km, _ = call(False)
            finally:
                ctx.set_option("vad_seg_cap", None)
            single = f" | room for {most} from the start: one launch, machine kernel {km:8.1f} ms, lean call {w * 1e3:8.1f} ms"

        def spread(xs, scale=1.0, fmt="8.1f"):
            xs = sorted(x * scale for x in xs)
            return f"{xs[len(xs) // 2]:{fmt}} [{xs[0]:{fmt}} .. {xs[-1]:{fmt}}]"
        py_txt = f"{t_py * 1e3:8.1f} ms" if t_py is not None else "       -   "
        print(f"N={N:5d}: {launches} launch(es) (most segments of a machine {most}, first room {cap0}) | machine kernel per launch "
              f"{spread(mach)} ms | scoring: device {spread(score, fmt='6.2f')} ms, host {a.threads} threads {t_host * 1e3:7.1f} ms, "
              f"per-segment Python {py_txt} | call: lean {spread(lean_t, 1e3)} ms vs segments back + host scoring "
              f"{spread(keep_t, 1e3)} ms, ratio {spread(ratio, fmt='5.2f')}"
              + (f" (+ Python scoring instead: {(sorted(keep_t)[len(keep_t) // 2] - t_host + t_py) / sorted(lean_t)[len(lean_t) // 2]:5.2f}x)"
                 if t_py is not None else "")
              + f" | D2H {bytes_lean / 2**20:7.1f} MB vs {bytes_keep / 2**20:8.1f} MB | peak device memory of the lean call "
              f"{pm.peak_bytes / 2**30:6.2f} GB | {n_segs} segments | bit-identical: {same}{single}", flush=True)
        sw.close()
        del band
        torch.cuda.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
