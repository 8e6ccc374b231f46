"""Getting a denoised corpus off the device as WAV files at 44.1 kHz ("Recordings at other rates"):
fvad_egress_resample into mapped files against the only way there was before it, on synthetic lanes standing in for denoised audio.
  --streams mono f32 lanes of --hours hours on the device (config 4's corpus shape, 21 x 2 h; fewer if host memory or the free
  space of --dir does not allow, said so).  After one warm-up, --repeats rounds; printed per way: the median [min - max] wall time
  and the PCIe bytes it moves --
    (a) run_denoise(rate=44100)'s export step, as pcm16 and as f32: every file created at its final size with its header and
        mapped (simulator._DenoisedFile), one fvad_egress_resample over all of them with fvad_resample_design's default taps
        (147/160, 5121 taps), the maps dropped;
    (b) the way before: the f32 lanes copied back (Context.to_host), the same taps applied phase by phase in numpy (float32
        products, as tools/clips_resample_time.py's host route) and fvad_wav_write as f32.  It is MEASURED ON --host-minutes
        MINUTES OF ONE STREAM AND SCALED by the samples to the corpus, as the resampling ingest's host baseline was; its result is
        held against the device's f32 file over those minutes (to 1e-5: the sums are ordered differently) and a larger difference
        ends the tool;
  and for (a) the `egress_resample` kernel's device-event time summed over the call's batches, beside its computed minima from
  the shapes: the fma count at the vector f32 rate, the LDS bytes the filter loop reads (window and taps, 4 bytes each per
  term) and writes, the HBM bytes (lane bytes read + file bytes written) at the 6.29 TB/s copy rate DESIGN uses.
There is no pass / fail number.  Files are removed after every way.  Neither way waits for the disk.
timeout 900 python tools/egress_resample_time.py [--streams 21] [--hours 2] [--repeats 3] [--host-minutes 10] [--dir DIR] [--json PATH]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_package  # noqa: E402
from egress_time import fmt, mem_available  # noqa: E402

PEAK_FMA, LDS_BPC, CUS, CLOCK, COPY_RATE = 157.3e12 / 2, 128, 256, 2.4e9, 6.29e12   # fma/s; LDS bytes per clock and CU; CUs; Hz; B/s
RATE = 44100


def host_polyphase(x, taps, up, down):
    """the definition over a whole stream x (float32), phase by phase: float32 products summed by numpy -> float32 [out_frames]"""
    n, K = x.size, (taps.size - 1) // 2
    out_frames = -(-n * up // down)
    J = -(-taps.size // up)
    xp = np.concatenate([np.zeros(J + 1, np.float32), x, np.zeros(J + 1 + K // up + 1, np.float32)])
    P = K + np.arange(out_frames, dtype=np.int64) * down
    q, r = P // up, P % up
    y = np.zeros(out_frames, np.float32)
    for ph in range(up):
        sel = np.flatnonzero(r == ph)
        if sel.size == 0:
            continue
        h = taps[ph::up]                                        # taps[r + j up], j = 0 ..
        idx = q[sel, None] - np.arange(h.size)[None, :] + (J + 1)   # frames q - j, in the padded array
        y[sel] = (xp[idx] * h[None, :]).sum(axis=1, dtype=np.float32)
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-minutes", type=float, default=10.0)
    ap.add_argument("--dir", default=None, help="where the files go (default: a fresh temporary directory)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = load_package()
    fv, sim = pkg.binding, pkg.simulator
    n = int(a.hours * 3600 * 48000) // 24000 * 24000   # whole chunks, as the denoised lanes are
    rs = sim._denoised_resample(RATE)
    up, down, taps = rs["up"], rs["down"], rs["taps"]
    n_out = fv.resample_out_frames(n, up, down)
    work = tempfile.mkdtemp(prefix="egress_resample_time_", dir=a.dir)
    S = a.streams
    avail, free = mem_available(), shutil.disk_usage(work).free
    limits = [S] + ([int(0.45 * avail // (n_out * 4 + 1))] if avail is not None else []) + [int(0.8 * free // (n_out * 4 + 1))]
    if min(limits) < S:
        S = max(1, min(limits))
        print(f"host memory {0 if avail is None else avail / 1e9:.0f} GB available, {free / 1e9:.0f} GB free in {work}: timing {S} of {a.streams} streams", flush=True)
    ctx = fv.Context(0)
    d_lanes = ctx.device_alloc(S * n * 4)
    insts = [{"name": f"s{i:02d}"} for i in range(S)]
    res = {"streams_asked": a.streams, "streams": S, "hours": a.hours, "n_frames": n, "out_frames": n_out, "rate": RATE, "taps": int(taps.size),
           "repeats": a.repeats, "ways": {}}
    try:
        one = np.tile((np.random.default_rng(5).standard_normal(48000) * 0.2).astype(np.float32), -(-n // 48000))[:n]
        for i in range(S):   # (every lane its own device pages; the values repeat, the kernel does not care)
            ctx.to_device(d_lanes + i * n * 4, np.roll(one, 997 * i))
        lanes = dict(d_lanes=d_lanes, n_lanes=S, lane_stride=n, n_samples=n)

        def way_a(fmt_name):
            out = os.path.join(work, "a-" + fmt_name)
            os.makedirs(out, exist_ok=True)
            files = [sim._DenoisedFile(out, inst, fmt_name, 1, n, rs) for inst in insts]
            try:
                ctx.egress_resample([f.sink_resampled(n_out, i, 0, 0, n) for i, f in enumerate(files)], up, down, taps, out=[f.map for f in files], **lanes)
            finally:
                for f in files:
                    f.close()
            return out

        B = {"pcm16": 2, "f32": 4}
        print(f"{S} x {n / 48000 / 3600:.2f} h mono f32 lanes, {S * n * 4 / 1e9:.2f} GB on the device, written at {RATE} Hz ({up}/{down}, {taps.size} taps); files in {work}",
              flush=True)
        # ---- (b) on the first minutes of stream 0, and its result against the device's
        m = min(n, int(a.host_minutes * 60 * 48000) // 24000 * 24000)
        m_out = fv.resample_out_frames(m, up, down)
        t0 = time.perf_counter()
        host = ctx.to_host(np.empty(m, np.float32), d_lanes)
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        y = host_polyphase(host, taps, up, down)
        t_filter = time.perf_counter() - t0
        t0 = time.perf_counter()
        fv.wav_write(os.path.join(work, "b.wav"), y[None, :], sample_rate=RATE)
        t_write = time.perf_counter() - t0
        os.remove(os.path.join(work, "b.wav"))
        d_o = ctx.device_alloc(m_out * 4)
        try:
            ctx.egress_resample([(0, m_out, 1, fv.INGEST_F32, 0, 0, 0, m, m, 0)], up, down, taps, out=d_o, out_bytes=m_out * 4, **lanes)
            dev = ctx.to_host(np.empty(m_out, np.float32), d_o)
        finally:
            ctx.device_free(d_o)
        diff = float(np.abs(dev - y).max())
        if not diff <= 1e-5:
            raise SystemExit(f"the host route's samples differ from the device's by {diff}")
        scale = S * n / m
        b = {"minutes": m / 48000 / 60, "copy_s": t_copy, "filter_s": t_filter, "write_s": t_write, "scale": scale,
             "scaled_s": (t_copy + t_filter + t_write) * scale, "max_diff": diff, "pcie_bytes": S * n * 4}
        res["ways"]["b: to_host + numpy polyphase + fvad_wav_write f32"] = b
        print(f"  (b: to_host + numpy polyphase + fvad_wav_write f32) on {b['minutes']:.1f} min of one stream: copy {t_copy:.3f} s, filter {t_filter:.3f} s, "
              f"write {t_write:.3f} s; scaled by {scale:.0f} to the corpus: {b['scaled_s']:.0f} s   PCIe {S * n * 4 / 1e9:.2f} GB   (max difference to the device {diff:.2e})",
              flush=True)
        # ---- (a)
        walls, kernel = {k: [] for k in B}, {k: [] for k in B}
        ctx.enable_timing(True)
        for rnd in range(a.repeats + 1):   # round 0: the warm-up
            for k in B:
                ctx.kernel_times()
                t0 = time.perf_counter()
                out = way_a(k)
                wall = time.perf_counter() - t0
                kt = ctx.kernel_times().get("egress_resample", 0.0) * 1e-3
                shutil.rmtree(out)
                if rnd:
                    walls[k].append(wall)
                    kernel[k].append(kt)
                    print(f"  round {rnd} (a: fvad_egress_resample -> {k}) {wall:.3f} s, kernel {kt * 1e3:.1f} ms", flush=True)
        ctx.enable_timing(False)
        outs = S * n_out
        terms = outs * (-(-taps.size // up))          # at most ceil(n_taps / up) terms an output (35 at 147/160)
        for k, bytes_per in B.items():
            t_fma = terms / PEAK_FMA
            t_lds = (terms * 8 + outs * bytes_per) / (LDS_BPC * CUS * CLOCK)
            hbm = S * n * 4 + outs * bytes_per
            t_hbm = hbm / COPY_RATE
            kk = float(np.median(kernel[k]))
            name = f"a: fvad_egress_resample -> {k}"
            print(f"  ({name:34s}) {fmt(walls[k])}   PCIe {outs * bytes_per / 1e9:7.2f} GB   egress_resample kernel {kk * 1e3:8.2f} ms "
                  f"[{min(kernel[k]) * 1e3:.2f} - {max(kernel[k]) * 1e3:.2f}]; computed minima: fma {t_fma * 1e3:.2f} ms, LDS {t_lds * 1e3:.2f} ms, "
                  f"HBM {t_hbm * 1e3:.2f} ms ({hbm / 1e9:.2f} GB)", flush=True)
            res["ways"][name] = {"wall_s": walls[k], "kernel_s": kernel[k], "pcie_bytes": outs * bytes_per, "hbm_bytes": hbm,
                                 "min_fma_s": t_fma, "min_lds_s": t_lds, "min_hbm_s": t_hbm}
            res[f"b_over_a_{k}"] = b["scaled_s"] / float(np.median(walls[k]))
            print(f"  (b, scaled) / (a), {k}: {res[f'b_over_a_{k}']:.0f}x by the medians", flush=True)
    finally:
        ctx.device_free(d_lanes)
        ctx.close()
        shutil.rmtree(work, ignore_errors=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
