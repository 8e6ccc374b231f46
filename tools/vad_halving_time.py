"""Cost of successive halving over VAD sweeps (fvad_vad_batch_retain_configs between device parts).
  1. The machine kernel on vad_sweep_time.py's device-generated corpus (S streams x H hours, mono) for each N of --configs: the
     plain parts (slices of --slice-chunks chunks) against the same parts with successive halving (eta --eta, --rungs rungs at
     simulator.halving_schedule's ends; each rung scores the prefix on the device against synthetic labels cut to it and keeps
     the best ceil(n / eta)).  Per stretch between rungs: machine kernel ms (device events); per retain: the gather's kernel ms,
     its rate counted as twice the new state's bytes (read + write) over that time, and device_bytes before and after.  The
     survivors' segment counts, audits, lazy statistics and full-corpus scores against a fresh batch of just the survivors run
     over the same parts, bit for bit.
  2. simulator.run_grid sliced with and without halving on a plan of synthetic PCM16 WAV files (vad_parts_time.write_corpus):
     wall time per stage, the rung lines, device_bytes.
python tools/vad_halving_time.py [--streams 21] [--hours 2] [--configs 4096,16384] [--eta 4] [--rungs 2] [--slice-chunks 1024]
                                 [--plan-streams 8] [--plan-minutes 30] [--grid-configs 1024] [--skip-grid]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_package  # noqa: E402
from vad_parts_time import write_corpus  # noqa: E402
from vad_sweep_time import device_corpus, make_configs  # noqa: E402

CHUNK, F = 24000, 1024


def labels_for(S, seconds, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(S):
        labs, x = [], rng.uniform(0, 5)
        while x < seconds:
            d = rng.uniform(0.5, 5.0)
            labs.append((x, min(x + d, seconds)))
            x += d + rng.uniform(1.0, 20.0)
        out.append(np.asarray(labs, np.float32).reshape(-1, 2))
    return out


def machines(fv, sim, ctx, a):
    import torch
    S = a.streams
    audio, rms, n_chunks = device_corpus(S, a.hours, a.seed)
    L = n_chunks * CHUNK
    nf = L // F
    N_sl = a.slice_chunks
    ends = sim.halving_schedule(n_chunks, N_sl, a.eta, a.rungs)
    labels = labels_for(S, n_chunks * CHUNK / 48000.0, a.seed)
    print(f"[1] {S} streams x {a.hours:g} h ({nf} frames each), mono, fft 1024, slices of {N_sl} chunks, eta {a.eta}, rungs at "
          f"chunks {ends} of {n_chunks}; kernel ms from device events", flush=True)
    ctx.enable_timing(True)
    sc = {"ignore_shorter_than_sec": 0.7, "extrude_start": 5.0, "extrude_end": 10.0, "fill_gaps": 5.0}
    for N in [int(x) for x in a.configs.split(",")]:
        cfgs = make_configs(N, a.seed + N)
        probe = fv.VadSweep(S, cfgs)
        bins, _ = probe.bands()
        probe.close()
        band = torch.empty((len(bins), S, nf), dtype=torch.float32, device=audio.device)
        torch.cuda.synchronize()
        ctx.band_sums_device(audio.data_ptr(), S, L, L, bins, band.data_ptr(), nf)
        ctx.kernel_times()

        def run(sw, halving):
            """sw over the slices; with halving, the rungs.  -> (kernel ms per stretch, [(retain ms, bytes before, after)],
            survivors)"""
            cur_bins = list(bins)
            block = {b: j for j, b in enumerate(bins)}
            alive = list(range(sw.n_configs))
            stretch, retains, kern = [], [], 0.0
            sw.set_references(labels, [sc] * len(alive))
            sw.keep_segments(False)
            d_part = torch.empty((len(bins), S, N_sl * CHUNK // F), dtype=torch.float32, device=audio.device)
            for c0 in range(0, n_chunks, N_sl):
                c1 = min(c0 + N_sl, n_chunks)
                f0, f1 = c0 * CHUNK // F, c1 * CHUNK // F
                idx = torch.tensor([block[b] for b in cur_bins], device=audio.device)
                part = d_part[:len(cur_bins), :, :f1 - f0]
                part.copy_(band.index_select(0, idx)[:, :, f0:f1])
                torch.cuda.synchronize()
                sw.run_device_part(ctx, d_part.data_ptr(), d_part.shape[2], [f1 - f0] * S, np.ascontiguousarray(rms[:, c0:c1]),
                                   [c1 - c0] * S, f0)
                kern += ctx.kernel_times().get("vad_machines", 0.0)
                if halving and c1 in ends:
                    t = c1 * CHUNK / 48000.0
                    sw.set_references([sim._clip_labels(x, t) for x in labels], [sc] * len(alive))
                    sw.score_device(ctx)
                    rows = [dict(config=c, F=sim._agg_row(fv.stats_aggregate_array(np.ascontiguousarray(sw.config_stats(c))))["F"])
                            for c in range(len(alive))]
                    keep = sorted(r["config"] for r in sim._ranked(rows)[:-(-len(alive) // a.eta)])
                    ctx.kernel_times()
                    before = sw.device_bytes()
                    sw.retain(ctx, keep)
                    rt = ctx.kernel_times().get("vad_retain", float("nan"))
                    retains.append((rt, before, sw.device_bytes(), len(alive), len(keep)))
                    alive = [alive[c] for c in keep]
                    cur_bins = sw.bands()[0]
                    sw.set_references(labels, [sc] * len(alive))
                    stretch.append(kern)
                    kern = 0.0
            stretch.append(kern)
            sw.score_device(ctx)
            return stretch, retains, alive

        plain = fv.VadSweep(S, cfgs)
        t0 = time.perf_counter()
        p_str, _, _ = run(plain, False)
        p_wall = time.perf_counter() - t0
        plain.close()
        hv = fv.VadSweep(S, cfgs)
        t0 = time.perf_counter()
        h_str, rets, alive = run(hv, True)
        h_wall = time.perf_counter() - t0
        got = ([hv.config_stats(c).copy() for c in range(len(alive))], [[hv.audit(s, c) for c in range(len(alive))] for s in range(S)],
               [[hv.lazy_stats(s, c) for c in range(len(alive))] for s in range(S)])
        hv.close()
        fresh = fv.VadSweep(S, [cfgs[i] for i in alive])
        fb, _ = fresh.bands()
        band_sub = band.index_select(0, torch.tensor([bins.index(b) for b in fb], device=audio.device)).contiguous()
        band_full, band = band, band_sub
        bins_full, bins = bins, fb
        run(fresh, False)
        band, bins = band_full, bins_full
        want = ([fresh.config_stats(c).copy() for c in range(len(alive))], [[fresh.audit(s, c) for c in range(len(alive))] for s in range(S)],
                [[fresh.lazy_stats(s, c) for c in range(len(alive))] for s in range(S)])
        fresh.close()
        same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got[0], want[0])) and got[1:] == want[1:]
        print(f"N={N:5d} plain parts: machine kernel {sum(p_str):9.1f} ms, wall {p_wall:6.2f} s", flush=True)
        print(f"N={N:5d} halving    : machine kernel {sum(h_str):9.1f} ms ({sum(h_str) / sum(p_str):5.3f} of plain; per stretch "
              f"{', '.join(f'{x:.1f}' for x in h_str)} ms), wall {h_wall:6.2f} s; {len(alive)} survivors bit-identical to a fresh "
              f"batch of them: {same}", flush=True)
        for k, (rt, b0, b1, n_in, n_keep) in enumerate(rets):
            print(f"        retain {k + 1}: {n_in} -> {n_keep} configs, kernel {rt:7.3f} ms, {2 * b1 / (rt * 1e-3) / 1e9:7.1f} GB/s "
                  f"(2 x new state), device_bytes {b0 / 2**20:9.1f} -> {b1 / 2**20:9.1f} MiB", flush=True)
        del band_sub, band_full
    ctx.enable_timing(False)
    del audio


def grid(fv, sim, ctx, a):
    d = a.plan_dir or tempfile.mkdtemp(prefix="halving_plan_")
    try:
        plan = write_corpus(fv, d, a.plan_streams, a.plan_minutes, a.seed)
        side = int(round(a.grid_configs ** (1 / 3)))
        g = {"base": {},
             "axes": {"speech_threshold_factor": np.linspace(1.5, 12.0, side).round(3).tolist(),
                      "long_term_speech_avg_sec": np.linspace(10.0, 300.0, side).round(1).tolist(),
                      "min_vad_duration_sec": np.linspace(0.1, 1.5, a.grid_configs // (side * side)).round(3).tolist()}}
        print(f"[2] run_grid on {a.plan_streams} x {a.plan_minutes:g} min stereo PCM16, "
              f"{side * side * (a.grid_configs // (side * side))} configs, slices of {a.slice_chunks} chunks", flush=True)
        for kw in ({}, {"halving_eta": a.eta, "halving_rungs": a.rungs}):
            t0 = time.perf_counter()
            r = sim.run_grid(plan, g, top=3, vad_on="device", score_on="device", ctx=ctx, slice_chunks=a.slice_chunks, **kw)
            print(f"    {'halving' if kw else 'plain'}: {time.perf_counter() - t0:.2f} s, device_bytes {r['device_bytes'] / 2**20:.1f} MiB",
                  flush=True)
    finally:
        if not a.plan_dir:
            shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--configs", default="4096,16384")
    ap.add_argument("--eta", type=int, default=4)
    ap.add_argument("--rungs", type=int, default=2)
    ap.add_argument("--slice-chunks", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--plan-dir", default=None)
    ap.add_argument("--plan-streams", type=int, default=8)
    ap.add_argument("--plan-minutes", type=float, default=30.0)
    ap.add_argument("--grid-configs", type=int, default=1024)
    ap.add_argument("--skip-grid", action="store_true")
    ap.add_argument("--skip-machines", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (torch's HIP runtime first, then the library's context, as vad_sweep_time.py does)
    pkg = load_package()
    fv, sim = pkg.binding, pkg.simulator
    ctx = fv.Context(0)
    ctx.load_synth(7)
    try:
        if not a.skip_machines:
            machines(fv, sim, ctx, a)
        if not a.skip_grid:
            grid(fv, sim, ctx, a)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
