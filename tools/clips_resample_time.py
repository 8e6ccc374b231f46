"""What clips at rates that are no whole fraction of 48 kHz cost (fvad_clips_export_resampled with fvad_resample_design's default
taps), in one process, on tools/clips_fir_time.py's corpus and schedule: one warm-up that is not kept, then --rounds
rounds, median [min - max].

Kernel: clip_gather_resampled at 44100 (f32 and PCM16 clips) and at 22050, beside the full-rate gather and the FIR gather at
16000 on the same clips (device time by events), and beside the kernel's computed minima from the shapes: the fma count at the
vector f32 rate, the LDS bytes the filter loop reads (window, and taps where the table is in LDS), the HBM bytes.

Wall: fvad_clips_export_resampled at 44100 against the route a user had before -- a full-rate fvad_clips_export and the same taps
applied phase by phase in numpy on the host.  The host route is timed on the first --host-clips clips and scaled by the samples;
its result is held against the device's.  The bytes each route moves over PCIe are printed.

run_clips end to end (tools/clips_sliced_time.py's corpus, --harness-hours of it): f32 clips, both kinds at 48000 (the arguments
run_clips always had) against both kinds resampled, the original at 44100 and the denoised at 22050.
There is no pass / fail number.

python tools/clips_resample_time.py [--streams 21] [--hours 2] [--rounds 3] [--host-clips 40] [--harness-hours 2] [--no-harness] [--dir DIR]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_package  # noqa: E402
from clips_time import clip_schedule  # noqa: E402
from clips_sliced_time import write_corpus  # noqa: E402
from clips_rate_time import mmm  # noqa: E402

PEAK_FMA, LDS_BPC, CUS, CLOCK, HBM = 157.3e12 / 2, 128, 256, 2.4e9, 8.0e12   # fma/s; ds_read_b32 bytes per clock and CU; CUs; Hz; B/s
TABLE_LDS = 6144                                                              # kClipResampleTableLds


def host_polyphase(x, taps, up, down):
    """y[o] = sum_j taps[r + j up] x[q - j], K + o down = q up + r, phase by phase (o mod up) in float64: per phase one matrix
    product of the phase's taps with the windows of its outputs"""
    h = taps.astype(np.float64)
    K, n = (len(h) - 1) // 2, len(x)
    n_out = -(-n * up // down)
    J = -(-len(h) // up)
    xp = np.concatenate([np.zeros(J), x.astype(np.float64), np.zeros(J + 1)])   # sample i at xp[J + i]
    win = sliding_window_view(xp, J)                                           # win[s] = xp[s : s + J] = x[s - J .. s - 1]
    y = np.zeros(n_out)
    for om in range(min(up, n_out)):
        q0, r = divmod(K + om * down, up)
        hp = np.zeros(J)
        hp[:len(h[r::up])] = h[r::up]
        k = np.arange(-(-(n_out - om) // up))
        q = q0 + down * k                                                      # x[q - J + 1 .. q] = win[q + 1]: the phase's taps reversed against it
        ok = q + 1 < len(win)
        y[om + up * k[ok]] = win[q[ok] + 1] @ hp[::-1]
        for kk in k[~ok]:                                                      # (outputs whose window runs past the padding: none for K <= J up)
            y[om + up * kk] = sum(hp[j] * (x[q[kk] - j] if 0 <= q[kk] - j < n else 0.0) for j in range(J))
    return y


def minima_ms(n_out, n_taps, up, n_src, src_bytes, out_bytes):
    J = -(-n_taps // up)
    fma = n_out * J
    lds = fma * (src_bytes if src_bytes == 4 else 4) + (fma * 4 if J * up <= TABLE_LDS else 0) + n_src * src_bytes + n_out * 8
    hbm = n_src * src_bytes + n_out * out_bytes
    return fma / PEAK_FMA * 1e3, lds / (LDS_BPC * CUS * CLOCK) * 1e3, hbm / HBM * 1e3


def export_part(pkg, a):
    import torch
    fv = pkg.binding
    ctx = fv.Context(0)
    S = a.streams
    L = int(a.hours * 3600 * 48000) // 24000 * 24000
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    audio = torch.empty((S, L), dtype=torch.float32, device=dev)
    for l in range(S):
        audio[l] = torch.randn(L, generator=g, device=dev) * 0.05
    torch.cuda.synchronize()
    clips = clip_schedule(S, 1, L, a.seed)
    lens = clips[:, 3] - clips[:, 2]
    n = int(lens.sum())
    ratios = {rate: fv.resample_ratio(48000, rate) for rate in (44100, 22050)}
    designs = {rate: fv.resample_design(*ratios[rate]) for rate in ratios}
    n_at = {rate: int(fv.clips_plan_resampled(lens, *ratios[rate])[0].sum()) for rate in ratios}
    skips = fv.clips_phase_skips(clips[:, 2], 3, 0)
    fir = fv.clips_fir_design(3)
    print(f"{S} mono streams x {a.hours:g} h on the device; {len(clips)} clips: {n} samples at 48 kHz, {n_at[44100]} at 44.1 kHz, {n_at[22050]} at 22.05 kHz; "
          f"{len(designs[44100])} and {len(designs[22050])} taps", flush=True)

    def export(way, pcm16):
        kw = dict(out_pcm16=pcm16)
        if way == "fir":
            kw.update(step=3, skips=skips, taps=fir)
        elif way != "full":
            kw.update(up=ratios[way][0], down=ratios[way][1], taps=designs[way])
        return ctx.clips_export(audio.data_ptr(), False, S, L, L, clips, **kw)

    name = {"full": "clip_gather", "fir": "clip_gather_fir", 44100: "clip_gather_resampled", 22050: "clip_gather_resampled"}
    ways = [("full", False), ("fir", False), (44100, False), (44100, True), (22050, False)]
    wall, kern = {w: [] for w in ways}, {w: [] for w in ways}
    ctx.enable_timing(True)
    for rnd in range(-1, a.rounds):   # (-1: the warm-up, not kept)
        for w in ways:
            ctx.kernel_times()
            t0 = time.perf_counter()
            export(*w)
            t = time.perf_counter() - t0
            kt = ctx.kernel_times()
            if rnd >= 0:
                wall[w].append(t)
                kern[w].append(kt[name[w[0]]])
    ctx.enable_timing(False)
    for w in ways:
        way, pcm16 = w
        line = f"{str(way):>6s} {'PCM16' if pcm16 else 'f32  '} clips: {name[way]} {mmm(kern[w])} ms | export wall {mmm(wall[w])} s"
        if way in ratios:
            e = minima_ms(n_at[way], len(designs[way]), ratios[way][0], n, 4, 2 if pcm16 else 4)
            out_b = n_at[way] * (2 if pcm16 else 4)
            line += (f" | computed minima: {e[0]:.2f} ms of fma at the vector peak, {e[1]:.2f} ms of LDS reads, {e[2]:.2f} ms of HBM traffic -> "
                     f"{np.median(kern[w]) / max(e):.1f}x of the largest | {out_b / 1e6:.0f} MB over PCIe")
        elif way == "full":
            line += f" | {n * 4 / 1e6:.0f} MB over PCIe"
        print(line, flush=True)

    # ---- the wall time against the host route (f32 clips at 44100), the host route on the first clips and scaled
    up, down = ratios[44100]
    taps = designs[44100]
    got = export(44100, False)
    t0 = time.perf_counter()
    full = export("full", False)
    t_exp = time.perf_counter() - t0
    few = range(min(a.host_clips, len(clips)))
    t0 = time.perf_counter()
    ys = [host_polyphase(full["out"][int(full["offsets"][i]):int(full["offsets"][i]) + int(lens[i])], taps, up, down) for i in few]
    t_few = time.perf_counter() - t0
    n_few = int(sum(int(lens[i]) for i in few))
    worst = max(float(np.max(np.abs(got["out"][int(got["offsets"][i]):int(got["offsets"][i]) + int(got["out_lens"][i])] - y))) for i, y in zip(few, ys))
    t_host = t_exp + t_few * n / n_few
    print(f"f32 clips at 44100, wall: fvad_clips_export_resampled {mmm(wall[(44100, False)])} s ({n_at[44100] * 4 / 1e6:.0f} MB over PCIe) | fvad_clips_export "
          f"{t_exp:.2f} s ({n * 4 / 1e6:.0f} MB over PCIe) + the same taps phase by phase in numpy on the host {t_few * n / n_few:.0f} s (SCALED from {t_few:.1f} s on the "
          f"first {len(few)} clips, {n_few} of {n} samples) = {t_host / np.median(wall[(44100, False)]):.0f}x | largest difference between the two on those clips {worst:.2e}", flush=True)
    ctx.close()
    del audio
    torch.cuda.empty_cache()


def harness_part(pkg, a):
    fv, sim = pkg.binding, pkg.simulator
    root = a.dir or tempfile.mkdtemp(prefix="clips_resample_")
    os.makedirs(root, exist_ok=True)
    t0 = time.perf_counter()
    plan, L = write_corpus(pkg, root, a.streams, a.harness_hours)
    print(f"{a.streams} mono streams x {L / 48000 / 3600:.2f} h as PCM16 WAV in {root} ({time.perf_counter() - t0:.0f} s to write)", flush=True)
    ctx = fv.Context(0)
    ctx.load_synth(7)
    ways = {"48000 / 48000 (the arguments run_clips always had)": {},
            "44100 / 22050 resampled": dict(original_filter="resample", original_rate=44100, denoised_filter="resample", denoised_rate=22050)}
    wall = {w: [] for w in ways}
    out = os.path.join(root, "out")
    with ctx.options(reproducible="1"):
        for rnd in range(-1, a.rounds):   # (-1: the warm-up, not kept)
            for w, kw in ways.items():
                shutil.rmtree(out, ignore_errors=True)
                t0 = time.perf_counter()
                sim.run_clips(plan, out, ctx=ctx, ingest=a.ingest, **kw)
                t = time.perf_counter() - t0
                if rnd >= 0:
                    wall[w].append(t)
    base = np.median(wall[next(iter(ways))])
    for w in ways:
        print(f"run_clips f32 clips, original / denoised at {w}: wall {mmm(wall[w])} s ({np.median(wall[w]) / base:.2f}x)", flush=True)
    ctx.close()
    shutil.rmtree(root if a.dir is None else out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--harness-hours", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-clips", type=int, default=40)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--ingest", default="device", choices=("host", "device"))
    ap.add_argument("--no-harness", action="store_true")
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    pkg = load_package()
    export_part(pkg, a)
    if not a.no_harness:
        harness_part(pkg, a)


if __name__ == "__main__":
    main()
