"""What anti-aliased 16 kHz clips cost (fvad_clips_export_fir with step 3 and the default 97 taps), in one process, on
tools/clips_rate_time.py's corpus and schedule.  Three comparisons, the ways of each alternated: one warm-up that is not kept,
then --rounds rounds, median [min - max].

Kernel: clip_gather_fir against clip_gather_strided on the same clips (device time by events), as f32 and as PCM16 clips, beside
the time the mapping predicts from the shapes: the fma count at the vector f32 rate, the LDS bytes the filter loop and the image
pass move, the HBM bytes.

Wall: fvad_clips_export_fir against the route a user had before -- a full-rate fvad_clips_export and the same filter in numpy on
the host.  The host filter is the cheaper of a polyphase form (three np.convolve of a third of the length each) and
np.convolve(...)[::3], chosen on the first clips and named in the output; its result is held against the device's.

run_clips end to end (tools/clips_sliced_time.py's corpus: S mono streams as PCM16 WAV files): PCM16 clips, the original kind at
16000 with original_filter "fir" against "none" (the denoised kind at 16000 in both), unsliced and in slices of --slice-chunks.
There is no pass / fail number.

python tools/clips_fir_time.py [--streams 21] [--hours 2] [--rounds 3] [--slice-chunks 1024] [--ingest device] [--no-harness] [--dir DIR]"""
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
from clips_time import clip_schedule  # noqa: E402
from clips_sliced_time import write_corpus  # noqa: E402
from clips_rate_time import mmm  # noqa: E402

STEP = 3
PEAK_FMA, LDS_BPC, CUS, CLOCK, HBM = 157.3e12 / 2, 128, 256, 2.4e9, 8.0e12   # fma/s; ds_read_b32 bytes per clock and CU; CUs; Hz; B/s


def host_direct(x, taps, skip):
    h = taps.astype(np.float64)
    H = (len(h) - 1) // 2
    return np.convolve(x.astype(np.float64), h[::-1])[H + skip:H + len(x):STEP]


def host_polyphase(x, taps, skip):
    """the same centres from three convolutions of a third of the length: y[q] = sum_j sum_m h[j + 3 m] xp[skip + j + 3 (q + m)]"""
    h = taps.astype(np.float64)
    H = (len(h) - 1) // 2
    n_out = -(-(len(x) - skip) // STEP)
    xp = np.concatenate([np.zeros(H), x.astype(np.float64), np.zeros(H + 2 * STEP)])
    y = np.zeros(n_out)
    for j in range(STEP):
        hj = h[j::STEP]
        xj = xp[skip + j::STEP][:n_out + len(hj) - 1]
        y += np.convolve(xj, hj[::-1], mode="valid")[:n_out]
    return y


def expected_ms(n_out, n_taps, n_src, out_bytes):
    """the kernel's time from the shapes: 4 outputs per lane read n_taps + 3 step samples for 4 n_taps fma; the image pass reads
    and writes every staged sample once more"""
    fma = n_out * n_taps
    lds = n_out / 4 * (n_taps + 3 * STEP) * 4 + (n_out * STEP) * (4 + 4 + 4)   # the loop; staging store, image load and store
    hbm = n_src * 4 + n_out * out_bytes
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
    n = int((clips[:, 3] - clips[:, 2]).sum())
    skips = fv.clips_phase_skips(clips[:, 2], STEP, 0)
    n3 = int(fv.clips_plan_strided(clips[:, 3] - clips[:, 2], skips, STEP)[0].sum())
    taps = fv.clips_fir_design(STEP)
    print(f"{S} mono streams x {a.hours:g} h on the device; {len(clips)} clips: {n} samples at 48 kHz, {n3} at 16 kHz; {len(taps)} taps", flush=True)

    def export(way, pcm16):
        return ctx.clips_export(audio.data_ptr(), False, S, L, L, clips, out_pcm16=pcm16, step=1 if way == "full" else STEP,
                                skips=None if way == "full" else skips, taps=taps if way == "fir" else None)

    # ---- the kernels
    ways = [(way, pcm16) for pcm16 in (False, True) for way in ("strided", "fir")]
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
                kern[w].append(kt["clip_gather_fir" if w[0] == "fir" else "clip_gather_strided"])
    for pcm16 in (False, True):
        e = expected_ms(n3, len(taps), n, 2 if pcm16 else 4)
        s, f = np.median(kern[("strided", pcm16)]), np.median(kern[("fir", pcm16)])
        print(f"{'PCM16' if pcm16 else 'f32  '} clips: clip_gather_strided {mmm(kern[('strided', pcm16)])} ms | clip_gather_fir {mmm(kern[('fir', pcm16)])} ms = {f / s:.1f}x | "
              f"from the shapes: {e[0]:.2f} ms of fma at the vector peak, {e[1]:.2f} ms of LDS traffic, {e[2]:.2f} ms of HBM traffic -> {f / max(e):.1f}x of the largest | "
              f"wall {mmm(wall[('strided', pcm16)])} s strided, {mmm(wall[('fir', pcm16)])} s filtered", flush=True)
    ctx.enable_timing(False)

    # ---- the wall time against the host route (f32 clips)
    few = range(min(40, len(clips)))
    full = export("full", False)
    cost = {}
    for name, fn in (("polyphase", host_polyphase), ("np.convolve(...)[::3]", host_direct)):
        t0 = time.perf_counter()
        for i in few:
            o = int(full["offsets"][i])
            fn(full["out"][o:o + int(clips[i, 3] - clips[i, 2])], taps, int(skips[i]))
        cost[name] = time.perf_counter() - t0
    host_name = min(cost, key=cost.get)
    host_fn = host_polyphase if host_name == "polyphase" else host_direct
    print("the host filter on the first clips: " + ", ".join(f"{k} {v:.2f} s" for k, v in cost.items()) + f" -> {host_name}", flush=True)
    routes = {"device": [], "host": [], "host: export": []}
    worst = 0.0
    for rnd in range(-1, a.rounds):
        t0 = time.perf_counter()
        got = export("fir", False)
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        full = export("full", False)
        t_exp = time.perf_counter() - t0
        ys = []
        for i in range(len(clips)):
            o = int(full["offsets"][i])
            ys.append(host_fn(full["out"][o:o + int(clips[i, 3] - clips[i, 2])], taps, int(skips[i])).astype(np.float32))
        t_host = time.perf_counter() - t0
        if rnd >= 0:
            routes["device"].append(t_dev)
            routes["host"].append(t_host)
            routes["host: export"].append(t_exp)
        else:
            for y, o, m in zip(ys, got["offsets"], got["out_lens"]):
                worst = max(worst, float(np.max(np.abs(got["out"][int(o):int(o) + int(m)] - y))))
    print(f"f32 clips, wall: fvad_clips_export_fir {mmm(routes['device'])} s | fvad_clips_export + {host_name} on the host {mmm(routes['host'])} s "
          f"(of which the export {mmm(routes['host: export'])} s) = {np.median(routes['host']) / np.median(routes['device']):.1f}x | "
          f"largest difference between the two {worst:.2e}", flush=True)
    ctx.close()
    del audio
    torch.cuda.empty_cache()


def harness_part(pkg, a):
    fv, sim = pkg.binding, pkg.simulator
    root = a.dir or tempfile.mkdtemp(prefix="clips_fir_")
    os.makedirs(root, exist_ok=True)
    t0 = time.perf_counter()
    plan, L = write_corpus(pkg, root, a.streams, a.hours)
    print(f"{a.streams} mono streams x {L / 48000 / 3600:.2f} h as PCM16 WAV in {root} ({time.perf_counter() - t0:.0f} s to write)", flush=True)
    ctx = fv.Context(0)
    ctx.load_synth(7)
    ways = [(sl, filt) for sl in (None, a.slice_chunks) for filt in ("none", "fir")]
    wall = {w: [] for w in ways}
    out = os.path.join(root, "out")
    with ctx.options(reproducible="1"):
        for rnd in range(-1, a.rounds):   # (-1: the warm-up, not kept)
            for w in ways:
                sl, filt = w
                shutil.rmtree(out, ignore_errors=True)
                t0 = time.perf_counter()
                sim.run_clips(plan, out, pcm16=True, ctx=ctx, ingest=a.ingest, slice_chunks=sl, denoised_rate=16000, original_rate=16000, original_filter=filt)
                t = time.perf_counter() - t0
                if rnd >= 0:
                    wall[w].append(t)
    for sl, filt in ways:
        base = np.median(wall[(sl, "none")])
        print(f"run_clips PCM16 16000 Hz {'unsliced' if sl is None else f'slices of {sl}':16s} original_filter {filt:4s}: wall {mmm(wall[(sl, filt)])} s "
              f"({np.median(wall[(sl, filt)]) / base:.2f}x of none)", flush=True)
    ctx.close()
    shutil.rmtree(root if a.dir is None else out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--slice-chunks", type=int, default=1024)
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
