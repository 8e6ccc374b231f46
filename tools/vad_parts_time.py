"""Cost of running the GPU VAD machines in parts, and of run_grid in time slices.
  1. The machine kernel on vad_sweep_time.py's device-generated corpus (S streams x H hours, mono): one launch
     (fvad_vad_batch_run_device) against P parts (fvad_vad_batch_run_device_part) for each P of --parts and N of --configs.
     Device events around the kernel launches (summed over the parts), the forms alternated rep after rep, median [min - max];
     the call's wall time too; segments, audits and lazy statistics bit for bit against the one launch; the device bytes the
     batch holds between the parts.
  2. simulator.run_grid sliced (--slice-chunks) against unsliced on a plan of synthetic PCM16 WAV files written to --plan-dir
     (as many --plan-minutes streams as --plan-streams asks, fewer if the disk has less room): wall time per stage,
     device_bytes, the low-water mark of free device memory (torch.cuda.mem_get_info sampled every 20 ms: other processes on
     a shared card move it too), and the configs whose statistics differ between the two (default mode: the NN kernels the
     engine selects depend on the launch size).
python tools/vad_parts_time.py [--streams 21] [--hours 2] [--configs 256,1024] [--parts 4,16,64] [--reps 3]
                               [--plan-streams 8] [--plan-minutes 30] [--slice-chunks 1024] [--skip-grid]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_package  # noqa: E402
from vad_sweep_time import device_corpus, make_configs  # noqa: E402

CHUNK, F = 24000, 1024


def med(xs):
    return f"{np.median(xs):9.1f} [{min(xs):9.1f} - {max(xs):9.1f}]"


def results(sw, S, N):
    return ([sw.segments(c) for c in range(N)], [[sw.audit(s, c) for c in range(N)] for s in range(S)],
            [[sw.lazy_stats(s, c) for c in range(N)] for s in range(S)])


def machines(fv, ctx, a):
    import torch
    S = a.streams
    audio, rms, n_chunks = device_corpus(S, a.hours, a.seed)
    L = n_chunks * CHUNK
    nf = L // F
    print(f"[1] {S} streams x {a.hours:g} h ({nf} frames each), mono, fft 1024; kernel ms from device events, median [min - max] "
          f"of {a.reps} alternated reps", flush=True)
    ctx.enable_timing(True)
    for N in [int(x) for x in a.configs.split(",")]:
        cfgs = make_configs(N, a.seed + N)
        probe = fv.VadSweep(S, cfgs)
        bins, _ = probe.bands()
        probe.close()
        band = torch.empty((len(bins), S, nf), dtype=torch.float32, device=audio.device)
        torch.cuda.synchronize()
        ctx.band_sums_device(audio.data_ptr(), S, L, L, bins, band.data_ptr(), nf)
        ctx.kernel_times()
        forms = ["one launch"] + [f"{P} parts" for P in (int(x) for x in a.parts.split(","))]
        kern = {f: [] for f in forms}
        wall = {f: [] for f in forms}
        want, same, state = None, {}, {}
        for rep in range(a.reps):
            for f in forms:
                sw = fv.VadSweep(S, cfgs)
                t0 = time.perf_counter()
                if f == "one launch":
                    sw.run_device(ctx, band.data_ptr(), nf, [nf] * S, rms, [n_chunks] * S)
                else:
                    P = int(f.split()[0])
                    step = -(-n_chunks // (P * 16)) * 16   # chunks per part, a multiple of 16
                    for c0 in range(0, n_chunks, step):
                        c1 = min(c0 + step, n_chunks)
                        f0, f1 = c0 * CHUNK // F, c1 * CHUNK // F
                        sw.run_device_part(ctx, band.data_ptr() + f0 * 4, nf, [f1 - f0] * S, np.ascontiguousarray(rms[:, c0:c1]),
                                           [c1 - c0] * S, f0)
                wall[f].append((time.perf_counter() - t0) * 1e3)
                kern[f].append(ctx.kernel_times().get("vad_machines", float("nan")))
                if rep == a.reps - 1:
                    r = results(sw, S, N)
                    if f == "one launch":
                        want = r
                    else:
                        same[f] = r == want
                        state[f] = sw.device_bytes()
                sw.close()
        base = np.median(kern["one launch"])
        for f in forms:
            extra = "" if f == "one launch" else (f" | x{np.median(kern[f]) / base:5.3f} of one launch | bit-identical: {same[f]} | "
                                                  f"held between parts {state[f] / 2**20:8.1f} MiB "
                                                  f"({state[f] / (S * N):7.0f} B per machine)")
            print(f"N={N:5d} {f:>10}: kernel {med(kern[f])} ms, call {med(wall[f])} ms{extra}", flush=True)
        del band
    ctx.enable_timing(False)
    del audio


def write_corpus(fv, d, n_streams, minutes, seed):
    """stereo PCM16 streams with speech-like bursts and their labels; returns the plan path"""
    rng = np.random.default_rng(seed)
    insts = []
    n = int(minutes * 60 * 48000)
    for i in range(n_streams):
        t_on, labels, x = np.zeros(n // 1024 + 1, np.float32), [], rng.uniform(0, 3)
        while x < n / 48000:
            dur = rng.uniform(0.5, 5.0)
            labels.append((x, min(x + dur, n / 48000)))
            t_on[int(x * 48000 / 1024):int((x + dur) * 48000 / 1024)] = 1
            x += dur + rng.uniform(1.0, 15.0)
        env = np.repeat(t_on, 1024)[:n]
        pcm = np.empty((2, n), np.float32)
        for c in range(2):
            pcm[c] = rng.standard_normal(n).astype(np.float32) * (0.01 + (0.2 if c == 0 else 0.12) * env)
        fv.wav_write(os.path.join(d, f"s{i}.wav"), pcm, pcm16=True)
        with open(os.path.join(d, f"s{i}.txt"), "w") as f:
            f.writelines(f"{a:.4f}\t{b:.4f}\tspeech\n" for a, b in labels)
        insts.append({"name": f"s{i}", "audio_path": f"s{i}.wav", "ref_path": f"s{i}.txt"})
    with open(os.path.join(d, "plan.json"), "w") as f:
        json.dump({"instances": insts}, f)
    return os.path.join(d, "plan.json")


class FreeLow:
    """the lowest free device memory seen while it runs (sampled)"""

    def __enter__(self):
        import torch
        self.low, self.stop = torch.cuda.mem_get_info()[0], False

        def loop():
            while not self.stop:
                self.low = min(self.low, torch.cuda.mem_get_info()[0])
                time.sleep(0.02)
        self.th = threading.Thread(target=loop, daemon=True)
        self.th.start()
        return self

    def __exit__(self, *exc):
        self.stop = True
        self.th.join()


def grid(pkg, fv, ctx, a):
    import torch
    sim = pkg.simulator
    d = tempfile.mkdtemp(dir=a.plan_dir)
    try:
        per_stream = int(a.plan_minutes * 60 * 48000) * 2 * 2
        room = shutil.disk_usage(d).free // 2   # (half the free disk at most)
        n_streams = max(1, min(a.plan_streams, room // per_stream))
        plan = write_corpus(fv, d, n_streams, a.plan_minutes, a.seed)
        g = {"axes": {"speech_threshold_factor": [3.0, 5.0, 7.0, 10.0], "long_term_speech_avg_sec": [60.0, 180.0],
                      "min_vad_duration_sec": [0.5, 1.0], "initial_long_term_avg": [None, 0.2]}}
        print(f"[2] run_grid: {n_streams} stereo PCM16 streams x {a.plan_minutes:g} min ({n_streams * per_stream / 2**30:.2f} GiB of "
              f"WAV), 32 configs, machines and scoring on the device; free-memory low-water is sampled and includes other "
              f"processes on the card", flush=True)
        out = {}
        for name, sc in (("unsliced", None), (f"{a.slice_chunks}-chunk slices", a.slice_chunks)):
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            t0 = time.perf_counter()
            with FreeLow() as fl:
                r = sim.run_grid(plan, g, vad_on="device", score_on="device", ctx=ctx, out=None, slice_chunks=sc)
            w = time.perf_counter() - t0
            out[name] = r
            t = r["times"]
            db = "not computed (unsliced)" if r["device_bytes"] is None else f"{r['device_bytes'] / 2**30:.2f} GiB"
            print(f"{name:>20}: {w:7.2f} s wall (denoise {t['denoise']:.2f}, bands {t['bands']:.2f}, machines {t['machines']:.2f}, "
                  f"scoring {t['scoring']:.3f}), {r['slices']} slice(s), device_bytes {db}, free-memory low-water "
                  f"{fl.low / 2**30:.1f} GiB (at start {free0 / 2**30:.1f} GiB: {(free0 - fl.low) / 2**30:.2f} GiB used)", flush=True)
        s0, s1 = (out[k]["stats"] for k in out)
        differ = int(np.sum(np.any(s0.view(np.uint32) != s1.view(np.uint32), axis=(1, 2))))
        print(f"configs whose statistics differ (default mode, as uint32): {differ} of {s0.shape[0]}", flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--configs", default="256,1024")
    ap.add_argument("--parts", default="4,16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--plan-dir", default=tempfile.gettempdir())
    ap.add_argument("--plan-streams", type=int, default=8)
    ap.add_argument("--plan-minutes", type=float, default=30.0)
    ap.add_argument("--slice-chunks", type=int, default=1024)
    ap.add_argument("--skip-machines", action="store_true")
    ap.add_argument("--skip-grid", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (torch's HIP runtime first, then the library's context, as vad_sweep_time.py does)
    pkg = load_package()
    fv = pkg.binding
    ctx = fv.Context(0)
    ctx.load_synth(7)
    try:
        if not a.skip_machines:
            machines(fv, ctx, a)
        if not a.skip_grid:
            grid(pkg, fv, ctx, a)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
