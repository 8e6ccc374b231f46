"""Cost of a VAD parameter sweep on config 4's corpus shape: S streams x H hours of synthetic denoised-like audio (seeded noise
with speech-like bursts, generated on the device), N configs that vary threshold, windows and speech band.  Per N:
  * K4: one multi-band pass (fvad_engine_band_sums_device with the sweep's distinct bands) against one single-band pass per
    distinct band (and against one per config: each distinct band's pass counted for every config that uses it);
  * the GPU VAD stage: device events around the machines' kernel inside fvad_vad_batch_run_device with both lane mappings
    (context option vad_lane_map: a stream's configs per wavefront, the default, or a config's streams), and the call's host
    part (frame ratios, uploads, read-back) separately;
  * fvad_vad_batch_run with T host threads over the same band sums;
  * device against host, bit for bit (segments and audits of every machine).
--vad-chain lane | coop sets the context option of that name for the device runs (how the machines run their exact long-term
chains).  --vad-chain both is the A/B mode for the two forms: per N one warm-up launch, then --reps rounds that alternate
lane and coop in one process, the machines' kernel time by device events, median [min - max] per form; the K4 comparison and the
config lane map are left out, the segment room is given from the start (vad_seg_cap) so that every N is one launch, and both
forms are checked against the host bit for bit.  --vad-chain lane-ab is the same protocol for the lane form alone (for a build
without the option: the parent's side of an A/B).
--vad-avgs both is the same A/B protocol for the averages (context option vad_avgs) under vad_chain coop: ring and table
alternated; besides the machines' kernel it prints the two table kernels' times on their own, table plus machines, the key
counts and the tables' bytes.  --grid-axes runs it on an axes grid (4 short windows x 8 bands x factors: 32 short keys whatever
N) instead of make_configs, whose random windows share few keys.
python tools/vad_sweep_time.py [--streams 21] [--hours 2] [--configs 1,8,64,256] [--threads 16] [--vad-chain both --reps 3] [--vad-avgs both [--grid-axes]]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

BANDS = [(500.0, 2000.0), (300.0, 3400.0), (1000.0, 4000.0), (200.0, 1200.0), (400.0, 2500.0), (600.0, 1800.0), (250.0, 4000.0),
         (800.0, 3000.0)]


def make_configs(n, seed):
    rng = np.random.default_rng(seed)
    out = [{}]
    while len(out) < n:
        lo, hi = BANDS[rng.integers(len(BANDS))]
        out.append({"speech_min_freq": lo, "speech_max_freq": hi, "speech_threshold_factor": float(rng.uniform(3.0, 15.0)),
                    "long_term_speech_avg_sec": float(rng.choice([60.0, 120.0, 180.0, 300.0])),
                    "short_term_speech_avg_sec": float(rng.uniform(0.1, 0.5)),
                    "channel_vol_ratio_avg_sec": float(rng.uniform(0.3, 1.0)),
                    "max_speech_gap_sec": float(rng.uniform(1.0, 3.0)), "min_vad_duration_sec": float(rng.uniform(0.5, 1.0))})
    return out[:n]


def axes_configs(n):
    """n configs as an axes grid: 4 short windows x 8 bands x (n / 32) factors -- 32 short keys and one ratio key whatever n"""
    out = []
    for st in (0.1, 0.2, 0.3, 0.5):
        for lo, hi in BANDS:
            for i in range(max(n // 32, 1)):
                out.append({"speech_min_freq": lo, "speech_max_freq": hi, "short_term_speech_avg_sec": st,
                            "speech_threshold_factor": 3.0 + 12.0 * i / max(n // 32, 1)})
    return out[:n]


def device_corpus(S, hours, seed, chunk=24000, F=1024):
    """S streams x hours of synthetic denoised-like mono audio on the device (a noise floor with bursts of 0.5 .. 5 s every
    1 .. 20 s, at frame resolution): (audio [S][n_chunks * chunk] f32 torch tensor on cuda:0, chunk RMS [S][n_chunks] numpy
    f32, n_chunks)"""
    import torch
    n_chunks = int(hours * 3600 * 48000) // chunk
    L = n_chunks * chunk
    nf = L // F
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.default_rng(seed)
    audio = torch.empty((S, L), dtype=torch.float32, device=dev)
    for s in range(S):
        edges = np.cumsum(rng.uniform(0.5, 20.0, int(L / 48000 / 5) + 8)) * 48000 / F
        env = np.zeros(nf + 1, np.float32)
        for x in edges:
            i0 = int(x)
            if i0 >= nf:
                break
            env[i0:min(nf, i0 + int(rng.uniform(0.5, 5.0) * 48000 / F))] = 1.0
        e = torch.from_numpy(env[:nf]).to(dev).repeat_interleave(F)
        audio[s] = torch.randn(L, generator=g, device=dev) * (0.01 + 0.2 * e)
        del e
    rms = torch.sqrt(torch.mean(audio.view(S, n_chunks, chunk) ** 2, dim=2)).cpu().numpy().astype(np.float32)
    torch.cuda.synchronize()
    return audio, rms, n_chunks


def ab_forms(a, fv, ctx, torch, audio, rms, n_chunks, S, L, nf):
    """--vad-chain both / lane-ab: the machines' kernel per form, alternated in one process (module docstring).  --vad-avgs
    both: under vad_chain coop, the ring form against the table form (context option vad_avgs) -- the machines' kernel, the two
    table kernels each on their own, and the tables' bytes"""
    avgs = a.vad_avgs == "both"
    forms = ["ring", "table"] if avgs else ["lane", "coop"] if a.vad_chain == "both" else ["lane"]
    grid = a.grid_axes
    dev = audio.device
    for N in [int(x) for x in a.configs.split(",")]:
        cfgs = axes_configs(N) if grid else make_configs(N, a.seed + N)
        sw = fv.VadSweep(S, cfgs)
        bins, _ = sw.bands()
        band = torch.empty((len(bins), S, nf), dtype=torch.float32, device=dev)
        ctx.band_sums_device(audio.data_ptr(), S, L, L, bins, band.data_ptr(), nf)
        torch.cuda.synchronize()
        ctx.set_option("vad_seg_cap", str(min(nf // 4 + 1, a.seg_cap)))   # room from the start: one launch whatever N
        ms = {f: [] for f in forms}
        tab = {"vad_minvol": [], "vad_avgs": []}
        tab_bytes = 0
        kept = {}
        try:
            if avgs:
                ctx.set_option("vad_chain", "coop")
            for rep in range(-1, a.reps):   # (-1: the warm-up, not kept)
                for f in forms:
                    if avgs:
                        ctx.set_option("vad_avgs", f)
                    elif a.vad_chain == "both":
                        ctx.set_option("vad_chain", f)
                    ctx.kernel_times()
                    sw.run_device(ctx, band.data_ptr(), nf, [nf] * S, rms, [n_chunks] * S)
                    kt = ctx.kernel_times()
                    t = kt.get("vad_machines", float("nan"))
                    if avgs:
                        assert sw.avgs_form() == (2 if f == "table" else 1), (f, sw.avgs_form())
                    if rep >= 0:
                        ms[f].append(t)
                        if f == "table":
                            for k in tab:
                                tab[k].append(kt.get(k, float("nan")))
                            tab_bytes = sw.avgs_bytes()
                    if rep == 0 and not a.no_host:
                        kept[f] = ([sw.segments(c) for c in range(N)], [sw.audit(s, c) for s in range(S) for c in range(N)],
                                   [sw.lazy_stats(s, c) for s in range(S) for c in range(N)])
        finally:
            ctx.set_option("vad_seg_cap", None)
            if a.vad_chain == "both" or avgs:
                ctx.set_option("vad_chain", None)
            if avgs:
                ctx.set_option("vad_avgs", None)
        host_txt = "host not run"
        if not a.no_host:
            hb = band.cpu().numpy()
            hs = fv.VadSweep(S, cfgs)
            t0 = time.perf_counter()
            hs.run(hb, rms, n_threads=a.threads)
            host = time.perf_counter() - t0
            want = ([hs.segments(c) for c in range(N)], [hs.audit(s, c) for s in range(S) for c in range(N)],
                    [hs.lazy_stats(s, c) for s in range(S) for c in range(N)])
            same = all(kept[f] == want for f in forms)
            chains = sum(x[0] for x in want[2])
            host_txt = (f"host {a.threads} threads {host * 1e3:9.1f} ms | {chains} exact chains ({chains * 64.0 / (S * N):.0f} per full "
                        f"wavefront) | bit-identical to the host: {same}")
            hs.close()
            del hb
        txt = " | ".join(f"{f} {np.median(ms[f]):8.2f} ms [{min(ms[f]):8.2f} - {max(ms[f]):8.2f}]" for f in forms)
        if avgs:
            st_keys, cr_keys, _, _ = sw.avg_keys()
            both = [m + x + y for m, x, y in zip(ms["table"], tab["vad_minvol"], tab["vad_avgs"])]
            txt += (f" | table kernels: min_volume {np.median(tab['vad_minvol']):7.2f} ms, averages {np.median(tab['vad_avgs']):8.2f} ms"
                    f" | table + machines {np.median(both):8.2f} ms [{min(both):8.2f} - {max(both):8.2f}] | {len(st_keys)} short keys, "
                    f"{len(cr_keys)} ratio keys, tables {tab_bytes / 2**30:.2f} GiB")
        print(f"N={N:4d} ({(S * N + 63) // 64} wavefronts): GPU VAD kernel {txt} | {host_txt}", flush=True)
        sw.close()
        del band


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--configs", default="1,8,64,256")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--vad-chain", default=None, choices=("lane", "coop", "both", "lane-ab"))
    ap.add_argument("--vad-avgs", default=None, choices=("both",),
                    help="alternate vad_avgs ring and table under vad_chain coop: the machines' kernel, the two table kernels, the tables' bytes")
    ap.add_argument("--grid-axes", action="store_true", help="with --vad-avgs both: an axes grid (shared keys) instead of make_configs")
    ap.add_argument("--reps", type=int, default=3, help="with --vad-chain both / lane-ab: timed rounds per form")
    ap.add_argument("--seg-cap", type=int, default=2048, help="with --vad-chain both / lane-ab: segment room per machine")
    ap.add_argument("--no-host", action="store_true", help="with --vad-chain both / lane-ab: skip the host run (and the bit check)")
    a = ap.parse_args()
    import torch
    pkg = load_package()
    fv = pkg.binding
    ctx = fv.Context(0)
    chunk, F = 24000, 1024
    S = a.streams
    audio, rms, n_chunks = device_corpus(S, a.hours, a.seed)
    L = n_chunks * chunk
    nf = L // F
    dev = audio.device
    d_den = audio.data_ptr()
    print(f"{S} streams x {a.hours:g} h ({nf} frames each), mono, fft 1024", flush=True)
    ctx.enable_timing(True)
    if a.vad_chain in ("both", "lane-ab") or a.vad_avgs == "both":
        ab_forms(a, fv, ctx, torch, audio, rms, n_chunks, S, L, nf)
        ctx.close()
        return
    if a.vad_chain:
        ctx.set_option("vad_chain", a.vad_chain)
    for N in [int(x) for x in a.configs.split(",")]:
        cfgs = make_configs(N, a.seed + N)
        sw = fv.VadSweep(S, cfgs)
        bins, band_of = sw.bands()
        band = torch.empty((len(bins), S, nf), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ctx.kernel_times()
        ctx.band_sums_device(d_den, S, L, L, bins, band.data_ptr(), nf)
        k4_multi = ctx.kernel_times().get("k4_bands", float("nan"))
        one = torch.empty((S, nf), dtype=torch.float32, device=dev)
        single = []
        for b in bins:
            ctx.band_sums_device(d_den, S, L, L, [b], one.data_ptr(), nf)
            single.append(ctx.kernel_times().get("k4_bands", float("nan")))
        k4_distinct = sum(single)
        k4_singles = sum(single[j] for j in band_of)
        torch.cuda.synchronize()
        lane_ms = {}
        for lane_map in ("config", "stream"):   # the device run kept below is the last one
            ctx.set_option("vad_lane_map", lane_map)
            t0 = time.perf_counter()
            sw.run_device(ctx, band.data_ptr(), nf, [nf] * S, rms, [n_chunks] * S)
            wall = time.perf_counter() - t0
            kt = ctx.kernel_times()
            lane_ms[lane_map] = kt.get("vad_machines", float("nan"))
            if lane_map == "config":
                segs_cfg = [sw.segments(c) for c in range(N)]
        ctx.set_option("vad_lane_map", None)
        vad_ms = lane_ms["stream"]
        hb = band.cpu().numpy()
        hs = fv.VadSweep(S, cfgs)
        t0 = time.perf_counter()
        hs.run(hb, rms, n_threads=a.threads)
        host = time.perf_counter() - t0
        same = all(sw.segments(c) == hs.segments(c) == segs_cfg[c] for c in range(N)) and \
            all(sw.audit(s, c) == hs.audit(s, c) for s in range(S) for c in range(N))
        n_segs = sum(len(x) for c in range(N) for x in sw.segments(c))
        ex_d = sum(sw.lazy_stats(s, c)[0] for s in range(S) for c in range(N))
        ex_h = sum(hs.lazy_stats(s, c)[0] for s in range(S) for c in range(N))
        print(f"N={N:4d} ({len(bins)} bands): K4 multi-band {k4_multi:8.2f} ms vs {len(bins)} single-band passes {k4_distinct:8.2f} ms "
              f"({N} per config: {k4_singles:9.2f} ms) | GPU VAD kernel {vad_ms:8.2f} ms (lanes by config: {lane_ms['config']:8.2f} ms) "
              f"+ host part {wall * 1e3 - vad_ms:7.2f} ms | host {a.threads} threads {host * 1e3:9.1f} ms | "
              f"speed-up {host * 1e3 / vad_ms:6.1f}x (kernel), {host / wall:6.1f}x (call) | {n_segs} segments, exact evals "
              f"{ex_d} dev / {ex_h} host | bit-identical: {same}", flush=True)
        sw.close()
        hs.close()
        del band, one
    ctx.close()


if __name__ == "__main__":
    main()
