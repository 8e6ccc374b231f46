"""Getting a corpus onto the device: today's host path against fvad_ingest, on interleaved raw buffers in host
memory standing in for page-cached files.
  Sets: --streams mono PCM16 streams of --hours hours (config 4's corpus shape, 21 x 2 h; fewer if host memory does not allow,
  said so), then 4 stereo PCM16 and 4 stereo PCM24 streams of the same length.  Per set, after one warm-up of each way, the
  ways alternate --repeats times; printed per way: the median [min - max] wall time and the PCIe bytes it moves --
    (a) today's path (simulator._denoise_resident / _slice_denoise_and_bands): a fresh zeroed f32 host image per round, which
        numpy fills one channel at a time (PCM16 times 1 / 32768; a contiguous read for mono, the strided read of a mapped
        file for stereo), and Context.to_device uploads; all three are in its time; no 24-bit form;
    (b) fvad_ingest into f32 lanes;
    (c) fvad_ingest into PCM16 lanes (PCM16 sources only);
  and for (b) and (c) the `ingest` kernel's device-event time summed over the call's batches and its HBM bytes (raw bytes
  read + lane bytes written) per second, beside the 6.29 TB/s copy rate DESIGN uses.  The lanes of (a) and (b) must be the
  same bits (compared once per set over three 64 K-sample windows of every lane: start, middle, end); a difference ends the tool.
python tools/ingest_time.py [--streams 21] [--hours 2] [--repeats 3] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

COPY_RATE = 6.29e12   # bytes/s: the device copy rate DESIGN §3 measures against


def mem_available():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return None


def make_raw(n_frames, n_channels, sample_bytes, seed):
    """interleaved little-endian samples: one second of seeded noise (moderate amplitude), tiled"""
    rng = np.random.default_rng(seed)
    block = 48000 * n_channels
    if sample_bytes == 2:
        one = rng.integers(-12000, 12000, block).astype("<i2").view(np.uint8)
    else:
        one = rng.integers(-(1 << 21), 1 << 21, block).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].reshape(-1)
    reps = -(-n_frames * n_channels * sample_bytes // one.size)
    return np.tile(one, reps)[:n_frames * n_channels * sample_bytes].copy()


def fmt(ts):
    return f"{np.median(ts):8.3f} s [{min(ts):.3f} - {max(ts):.3f}]"


def run_set(fv, ctx, label, raws, n_frames, n_channels, fmt_id, repeats, out):
    S = len(raws)
    n_lanes = S * n_channels
    stride = (n_frames + 3) // 4 * 4
    raw_bytes = sum(r.size for r in raws)
    rows = [(0, n_frames, n_channels, fmt_id, i * n_channels, 0, stride) for i in range(S)]
    d_f32 = ctx.device_alloc(n_lanes * stride * 4)
    d_i16 = ctx.device_alloc(n_lanes * stride * 2) if fmt_id == fv.INGEST_PCM16 else None
    W = min(1 << 16, stride)
    windows = sorted({0, (stride - W) // 2, stride - W})   # the samples the comparison reads: three windows per lane

    def checksum(d, dtype):
        acc = []
        one = np.empty(W, dtype)
        for l in range(n_lanes):
            for w in windows:
                acc.append(ctx.to_host(one, d + (l * stride + w) * one.itemsize).tobytes())
        return b"".join(acc)

    def way_a():
        host = np.zeros((n_lanes, stride), np.float32)
        l = 0
        for r in raws:
            a = r.view("<i2").reshape(n_frames, n_channels)
            for c in range(n_channels):
                np.multiply(a[:, c], np.float32(1.0 / 32768.0), out=host[l, :n_frames], casting="unsafe")
                l += 1
        ctx.to_device(d_f32, host)

    def way_b():
        ctx.ingest(rows, d_lanes=d_f32, n_lanes=n_lanes, lane_stride=stride, n_samples=stride, raw=raws)

    def way_c():
        ctx.ingest(rows, out_pcm16=True, d_lanes=d_i16, n_lanes=n_lanes, lane_stride=stride, n_samples=stride, raw=raws)

    ways = {}
    if fmt_id == fv.INGEST_PCM16:
        ways["a: numpy fill + f32 upload"] = (way_a, n_lanes * stride * 4, None)
    ways["b: fvad_ingest -> f32 lanes"] = (way_b, raw_bytes, raw_bytes + n_lanes * stride * 4)
    if fmt_id == fv.INGEST_PCM16:
        ways["c: fvad_ingest -> PCM16 lanes"] = (way_c, raw_bytes, raw_bytes + n_lanes * stride * 2)
    walls = {k: [] for k in ways}
    kernel = {k: [] for k in ways}
    sums = {}
    print(f"{label}: {S} x {n_frames / 48000 / 3600:.2f} h, {n_channels} channel(s), {raw_bytes / 1e9:.2f} GB raw, {n_lanes} lanes", flush=True)
    try:
        ctx.enable_timing(True)
        for rnd in range(repeats + 1):   # round 0: the warm-up
            for name, (fn, _, hbm) in ways.items():
                ctx.kernel_times()
                t0 = time.perf_counter()
                fn()
                wall = time.perf_counter() - t0
                kt = ctx.kernel_times().get("ingest", 0.0) * 1e-3
                if rnd == 0 and name[0] in "ab":
                    sums[name[0]] = checksum(d_f32, np.float32)
                if rnd:
                    walls[name].append(wall)
                    kernel[name].append(kt)
        if "a" in sums and sums["a"] != sums["b"]:
            raise SystemExit(f"{label}: the lanes of fvad_ingest differ from the host path's")
    finally:
        ctx.enable_timing(False)
        ctx.device_free(d_f32)
        if d_i16:
            ctx.device_free(d_i16)
    res = {"label": label, "streams": S, "n_frames": n_frames, "n_channels": n_channels, "raw_bytes": raw_bytes, "ways": {}}
    for name, (_, pcie, hbm) in ways.items():
        line = f"  ({name:30s}) {fmt(walls[name])}   PCIe {pcie / 1e9:7.2f} GB"
        entry = {"wall_s": walls[name], "pcie_bytes": pcie}
        if hbm is not None:
            k = float(np.median(kernel[name]))
            line += f"   ingest kernel {k * 1e3:8.2f} ms [{min(kernel[name]) * 1e3:.2f} - {max(kernel[name]) * 1e3:.2f}], {hbm / 1e9:.2f} GB of HBM traffic = " \
                    f"{hbm / k / 1e12:.2f} TB/s ({100 * hbm / k / COPY_RATE:.0f}% of the {COPY_RATE / 1e12:.2f} TB/s copy rate)"
            entry.update(kernel_s=kernel[name], hbm_bytes=hbm)
        print(line, flush=True)
        res["ways"][name] = entry
    out.append(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    fv = load_package().binding
    n_frames = int(a.hours * 3600 * 48000)
    # host memory of the mono set: the raw bytes, way (a)'s f32 image, and the copy the checksum holds
    per_stream = n_frames * (2 + 4) + (64 << 20)
    avail = mem_available()
    streams = a.streams
    if avail is not None and streams * per_stream > 0.7 * avail:
        streams = max(1, int(0.7 * avail // per_stream))
        print(f"host memory: {avail / 1e9:.0f} GB available, {a.streams} streams need {a.streams * per_stream / 1e9:.0f} GB: timing {streams} streams", flush=True)
    ctx = fv.Context(0)
    out = []
    try:
        sets = (("mono PCM16", streams, 1, 2, fv.INGEST_PCM16), ("stereo PCM16", 4, 2, 2, fv.INGEST_PCM16), ("stereo PCM24", 4, 2, 3, fv.INGEST_PCM24))
        for label, S, C_, B, fmt_id in sets:
            one = make_raw(n_frames, C_, B, seed=S)
            raws = [one] + [one.copy() for _ in range(S - 1)]   # (copies: every stream its own pages, as files have)
            run_set(fv, ctx, label, raws, n_frames, C_, fmt_id, a.repeats, out)
            del raws, one
    finally:
        ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"streams_asked": a.streams, "hours": a.hours, "repeats": a.repeats, "sets": out}, f, indent=1)


if __name__ == "__main__":
    main()
