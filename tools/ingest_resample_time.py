"""Getting a corpus at another rate onto the device ("Corpora at other rates"): --streams synthetic mono PCM16
streams of --hours hours at 44100 Hz (config 4's corpus shape, 21 x 2 h; fewer if host memory does not allow, said so), as
interleaved raw buffers in host memory standing in for page-cached files.  After one warm-up the ways alternate --repeats
times; printed per way: the median [min - max] wall time until the 48 kHz f32 lanes are on the device, the PCIe bytes, and the
kernel's own device-event time summed over the call's batches --
    (r) fvad_ingest_resample: the 44.1 kHz bytes, 160/147, the default design (5121 taps, 33 a phase);
    (a) the same durations at 48000 Hz through fvad_ingest: what resampling adds to today's way in;
    (b) the only way in today: the same taps applied on the host in numpy (float32, phase by phase over strided views) to
        --host-minutes of ONE stream, scaled to the corpus, plus the upload of one stream's f32 lane, scaled likewise.
Beside (r)'s kernel time: its minima at peak rates -- the fmas at the 157.3 TFLOP/s vector rate, the LDS reads (one per tap) at
32 lanes per clock and CU, 256 CUs, 2.4 GHz, and the HBM bytes (raw read + lanes written) at the 6.29 TB/s copy rate.  The first
outputs of stream 0 are held against the host's result (float32 sums in another order: 1e-5 of full scale); a larger
difference ends the tool.
python tools/ingest_resample_time.py [--streams 21] [--hours 2] [--repeats 3] [--host-minutes 10] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_package  # noqa: E402
from ingest_time import fmt, make_raw, mem_available  # noqa: E402

FMA_RATE = 157.3e12 / 2          # fma/s: the vector f32 peak
LDS_READ_RATE = 256 * 32 * 2.4e9  # lane reads/s: ds_read_u16 / _b32 serve 32 lanes per clock and CU
COPY_RATE = 6.29e12              # bytes/s: the device copy rate DESIGN §3 measures against


def host_resample(x_i16, taps, up, down, n_out):
    """the definition of fvad.h in numpy float32: the decode, then per o mod up one strided multiply-add per tap of the phase"""
    K = (taps.size - 1) // 2
    J = -(-taps.size // up)
    pad = J + 1
    xp = np.zeros(x_i16.size + 2 * pad + down + 2, np.float32)
    np.multiply(x_i16, np.float32(1.0 / 32768.0), out=xp[pad:pad + x_i16.size], casting="unsafe")
    y = np.zeros(n_out, np.float32)
    for om in range(min(up, n_out)):
        q0, r = divmod(K + om * down, up)
        M = len(range(om, n_out, up))
        acc = np.zeros(M, np.float32)
        for j in range((taps.size - 1 - r) // up + 1 if r < taps.size else 0):
            start = q0 - j + pad
            if start < 0:
                continue
            seg = xp[start:start + down * (M - 1) + 1:down]
            acc[:seg.size] += taps[r + j * up] * seg
        y[om::up] = acc
    return y


def timed(ctx, fn, name, repeats):
    walls, kernels = [], []
    for rnd in range(repeats + 1):   # round 0: the warm-up
        ctx.kernel_times()
        t0 = time.perf_counter()
        fn()
        wall = time.perf_counter() - t0
        kt = ctx.kernel_times().get(name, 0.0) * 1e-3
        if rnd:
            walls.append(wall)
            kernels.append(kt)
    return walls, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-minutes", type=float, default=10.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    fv = load_package().binding
    rate = 44100
    up, down = fv.resample_ratio(rate)
    taps = fv.resample_design(up, down)
    per_phase = -(-taps.size // up)
    n_in = int(a.hours * 3600 * rate)
    n_out = fv.resample_out_frames(n_in, up, down)
    stride = (n_out + 3) // 4 * 4
    per_stream = n_out * 2 + (64 << 20)   # host memory: the larger of the two raw sets, one at a time
    avail = mem_available()
    S = a.streams
    if avail is not None and S * per_stream > 0.6 * avail:
        S = max(1, int(0.6 * avail // per_stream))
        print(f"host memory: {avail / 1e9:.0f} GB available, {a.streams} streams need {a.streams * per_stream / 1e9:.0f} GB: timing {S} streams", flush=True)
    ctx = fv.Context(0)
    res = {"streams": S, "hours": a.hours, "rate": rate, "up": up, "down": down, "n_taps": int(taps.size), "taps_per_phase": per_phase}
    d_lanes = ctx.device_alloc(S * stride * 4)
    try:
        ctx.enable_timing(True)
        lanes = dict(d_lanes=d_lanes, n_lanes=S, lane_stride=stride, n_samples=stride)
        # ---- (r) 44.1 kHz bytes through fvad_ingest_resample
        one = make_raw(n_in, 1, 2, seed=S)
        raws = [one] + [one.copy() for _ in range(S - 1)]   # (copies: every stream its own pages, as files have)
        rows = [(0, n_in, 1, fv.INGEST_PCM16, i, 0, stride, 0, n_in, 0, n_out) for i in range(S)]
        w_r, k_r = timed(ctx, lambda: ctx.ingest_resample(rows, up, down, taps, raw=raws, **lanes), "ingest_resample", a.repeats)
        raw_r = sum(r.size for r in raws)
        head = ctx.to_host(np.empty(1 << 16, np.float32), d_lanes)
        # ---- (b) the host way on part of one stream, and one lane's upload
        n_host_in = min(n_in, int(a.host_minutes * 60 * rate))
        n_host_out = fv.resample_out_frames(n_host_in, up, down)
        t0 = time.perf_counter()
        y = host_resample(one[:2 * n_host_in].view("<i2"), taps, up, down, n_host_out)
        t_host = (time.perf_counter() - t0) * (n_in / n_host_in) * S
        n_cmp = min(head.size, n_host_out - 64)
        diff = float(np.max(np.abs(head[:n_cmp].astype(np.float64) - y[:n_cmp])))
        if not diff < 1e-5:
            raise SystemExit(f"the lanes of fvad_ingest_resample differ from the host's by {diff:g}")
        lane = np.zeros(stride, np.float32)
        ups = []
        for _ in range(a.repeats + 1):
            t0 = time.perf_counter()
            ctx.to_device(d_lanes, lane)
            ups.append(time.perf_counter() - t0)
        t_up = float(np.median(ups[1:])) * S
        del raws, one, y, lane
        # ---- (a) the same durations at 48 kHz through fvad_ingest
        n48 = int(a.hours * 3600 * 48000)
        one = make_raw(n48, 1, 2, seed=S + 1)
        raws = [one] + [one.copy() for _ in range(S - 1)]
        rows48 = [(0, n48, 1, fv.INGEST_PCM16, i, 0, stride) for i in range(S)]
        w_a, k_a = timed(ctx, lambda: ctx.ingest(rows48, raw=raws, **lanes), "ingest", a.repeats)
        raw_a = sum(r.size for r in raws)
        del raws, one
    finally:
        ctx.enable_timing(False)
        ctx.device_free(d_lanes)
        ctx.close()
    outputs = S * n_out
    hbm = raw_r + S * stride * 4
    mins = {"fma_s": outputs * per_phase / FMA_RATE, "lds_s": outputs * per_phase / LDS_READ_RATE, "hbm_s": hbm / COPY_RATE}
    k = float(np.median(k_r))
    print(f"{S} x {a.hours:.2f} h mono PCM16 at {rate} Hz -> 48000 Hz, {up}/{down}, {taps.size} taps ({per_phase} a phase), {outputs / 1e9:.2f} G outputs")
    print(f"  (r: fvad_ingest_resample      ) {fmt(w_r)}   PCIe {raw_r / 1e9:7.2f} GB   ingest_resample kernel {k * 1e3:8.2f} ms [{min(k_r) * 1e3:.2f} - {max(k_r) * 1e3:.2f}]")
    print(f"  (a: 48 kHz through fvad_ingest) {fmt(w_a)}   PCIe {raw_a / 1e9:7.2f} GB   ingest kernel          {np.median(k_a) * 1e3:8.2f} ms [{min(k_a) * 1e3:.2f} - {max(k_a) * 1e3:.2f}]")
    print(f"  (b: numpy on the host + upload) {t_host + t_up:8.3f} s = {t_host:.3f} s of numpy ({a.host_minutes:g} min of one stream, scaled) + {t_up:.3f} s of f32 upload "
          f"(one lane, scaled)   PCIe {S * stride * 4 / 1e9:7.2f} GB")
    print(f"  the kernel's minima: {mins['fma_s'] * 1e3:.2f} ms of fma at {FMA_RATE / 1e12:.1f} T fma/s, {mins['lds_s'] * 1e3:.2f} ms of LDS reads at "
          f"{LDS_READ_RATE / 1e12:.1f} T lane reads/s, {mins['hbm_s'] * 1e3:.2f} ms of HBM for {hbm / 1e9:.2f} GB at {COPY_RATE / 1e12:.2f} TB/s; "
          f"measured {k * 1e3:.2f} ms = {k / max(mins.values()):.1f} x the largest; largest difference from the host's float32 result {diff:.2e}")
    res.update(resample={"wall_s": w_r, "kernel_s": k_r, "pcie_bytes": raw_r}, native={"wall_s": w_a, "kernel_s": k_a, "pcie_bytes": raw_a},
               host={"numpy_s_scaled": t_host, "upload_s_scaled": t_up, "host_minutes": a.host_minutes}, minima=mins, hbm_bytes=hbm, max_diff=diff)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
