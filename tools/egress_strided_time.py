"""Getting a denoised corpus off the device as WAV files made from the network's own 16 kHz samples ("Recordings
from the network's samples"): run_denoise(source="network")'s export step against the lanes' ways, in one process, on synthetic
lanes standing in for denoised audio.
  --streams mono f32 lanes of --hours hours on the device (config 4's corpus shape, 21 x 2 h; fewer if host memory or the free
  space of --dir does not allow, said so).  After one warm-up, --repeats rounds; printed per way, as pcm16 and as f32: the median
  [min - max] wall time of the export step (every file created at its final size with its header and mapped, one call over all
  of them, the maps dropped), the PCIe bytes it moves, and the kernel's device-event time summed over the call's batches beside
  its computed minima from the shapes -- the fma count at the vector f32 rate, the LDS bytes the filter loop reads (window and
  taps, 4 bytes each per term) and writes (the staged window, the image), the HBM bytes (lane bytes read: at step 3 every
  128-byte line of the lanes is touched, so all of them; + file bytes written) at the 6.29 TB/s copy rate DESIGN uses:
    network 16000 / 48000 / 44100: fvad_egress_resample_strided over lane[3 j + 2] with _network_resample's taps (1/1 with the
        tap 1.0; 3/1, 101 taps; 441/160, 14701 taps: the table in global memory);
    lanes 16000 / 44100: fvad_egress_resample over the lanes with the default designs (1/3, 97 taps; 147/160, 5121 taps);
    lanes 48000: fvad_egress.
There is no pass / fail number.  The one expectation it prints a verdict for: at 16000 the strided kernel does 1 term per output
where the lanes' kernel does 97 and reads the same bytes, so it should not be the slower one.  Files are removed after every way.
No way waits for the disk.
timeout 900 python tools/egress_strided_time.py [--streams 21] [--hours 2] [--repeats 3] [--dir DIR] [--json PATH]"""
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
B = {"pcm16": 2, "f32": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=21)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a fresh temporary directory)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = load_package()
    fv, sim = pkg.binding, pkg.simulator
    n = int(a.hours * 3600 * 48000) // 24000 * 24000   # whole chunks, as the denoised lanes are
    work = tempfile.mkdtemp(prefix="egress_strided_time_", dir=a.dir)
    S = a.streams
    avail, free = mem_available(), shutil.disk_usage(work).free   # the largest way holds every 48 kHz f32 file
    limits = [S] + ([int(0.45 * avail // (n * 4 + 1))] if avail is not None else []) + [int(0.8 * free // (n * 4 + 1))]
    if min(limits) < S:
        S = max(1, min(limits))
        print(f"host memory {0 if avail is None else avail / 1e9:.0f} GB available, {free / 1e9:.0f} GB free in {work}: timing {S} of {a.streams} streams", flush=True)
    # (source, rate, the filter, the kernel's name in kernel_times)
    ways = [("network", r, sim._network_resample(r), "egress_strided") for r in (16000, 48000, 44100)]
    ways += [("lanes", r, sim._denoised_resample(r), "egress_resample") for r in (16000, 44100)] + [("lanes", 48000, None, "egress")]
    ctx = fv.Context(0)
    d_lanes = ctx.device_alloc(S * n * 4)
    insts = [{"name": f"s{i:02d}"} for i in range(S)]
    res = {"streams_asked": a.streams, "streams": S, "hours": a.hours, "n_frames": n, "repeats": a.repeats, "ways": {}}
    try:
        one = np.tile((np.random.default_rng(5).standard_normal(48000) * 0.2).astype(np.float32), -(-n // 48000))[:n]
        for i in range(S):   # (every lane its own device pages; the values repeat, the kernels do not care)
            ctx.to_device(d_lanes + i * n * 4, np.roll(one, 997 * i))
        lanes = dict(d_lanes=d_lanes, n_lanes=S, lane_stride=n, n_samples=n)

        def export(source, rate, rs, fmt_name):
            out = os.path.join(work, f"{source}-{rate}-{fmt_name}")
            os.makedirs(out, exist_ok=True)
            files = [sim._DenoisedFile(out, inst, fmt_name, 1, n, rs) for inst in insts]
            try:
                maps = [f.map for f in files]
                if rs is None:
                    ctx.egress([f.sink(0, n, i, 0) for i, f in enumerate(files)], out=maps, **lanes)
                else:
                    rows = [f.sink_resampled(f.manifest["frames"], i, rs.get("phase", 0), 0, f.stream_frames) for i, f in enumerate(files)]
                    sim._egress_resampled(ctx, rs, rows, maps, lanes)
            finally:
                for f in files:
                    f.close()
            return out

        print(f"{S} x {n / 48000 / 3600:.2f} h mono f32 lanes, {S * n * 4 / 1e9:.2f} GB on the device; files in {work}", flush=True)
        keys = [(w, k) for w in range(len(ways)) for k in B]   # (a way's index: its filter is a dict)
        walls, kernel = {key: [] for key in keys}, {key: [] for key in keys}
        ctx.enable_timing(True)
        for rnd in range(a.repeats + 1):   # round 0: the warm-up
            for w, k in keys:
                source, rate, rs, kname = ways[w]
                ctx.kernel_times()
                t0 = time.perf_counter()
                out = export(source, rate, rs, k)
                wall = time.perf_counter() - t0
                kt = ctx.kernel_times().get(kname, 0.0) * 1e-3
                shutil.rmtree(out)
                if rnd:
                    walls[(w, k)].append(wall)
                    kernel[(w, k)].append(kt)
                    print(f"  round {rnd} ({source} {rate} -> {k}) {wall:.3f} s, {kname} kernel {kt * 1e3:.1f} ms", flush=True)
        ctx.enable_timing(False)
        med = {}
        for w, k in keys:
            source, rate, rs, kname = ways[w]
            bytes_per = B[k]
            if rs is None:
                outs, terms, staged = S * n, 0, 0
            else:
                stream = n // rs.get("step", 1)
                outs = S * fv.resample_out_frames(stream, rs["up"], rs["down"])
                terms = outs * (-(-rs["taps"].size // rs["up"]))          # at most ceil(n_taps / up) terms an output
                staged = S * stream * 4                                    # the window written to LDS once (the reach's overlap aside)
            t_fma = terms / PEAK_FMA
            t_lds = (terms * 8 + staged + outs * bytes_per) / (LDS_BPC * CUS * CLOCK)
            hbm = S * n * 4 + outs * bytes_per
            t_hbm = hbm / COPY_RATE
            kk = float(np.median(kernel[(w, k)]))
            med[(source, rate, k)] = kk
            name = f"{source} {rate} -> {k}"
            print(f"  ({name:24s}) {fmt(walls[(w, k)])}   PCIe {outs * bytes_per / 1e9:7.2f} GB   {kname} kernel {kk * 1e3:8.2f} ms "
                  f"[{min(kernel[(w, k)]) * 1e3:.2f} - {max(kernel[(w, k)]) * 1e3:.2f}]; computed minima: fma {t_fma * 1e3:.2f} ms, LDS {t_lds * 1e3:.2f} ms, "
                  f"HBM {t_hbm * 1e3:.2f} ms ({hbm / 1e9:.2f} GB); terms an output {0 if rs is None else -(-rs['taps'].size // rs['up'])}", flush=True)
            res["ways"][name] = {"wall_s": walls[(w, k)], "kernel_s": kernel[(w, k)], "kernel": kname, "pcie_bytes": outs * bytes_per, "hbm_bytes": hbm,
                                 "min_fma_s": t_fma, "min_lds_s": t_lds, "min_hbm_s": t_hbm}
        for k in B:
            s_, p_ = med[("network", 16000, k)], med[("lanes", 16000, k)]
            res[f"strided_over_parent_16000_{k}"] = s_ / p_
            print(f"  at 16000, {k}: egress_strided {s_ * 1e3:.2f} ms against egress_resample {p_ * 1e3:.2f} ms: "
                  f"{'not slower, as expected' if s_ <= p_ else 'SLOWER -- collect the counters in a run of their own'}", flush=True)
    finally:
        ctx.device_free(d_lanes)
        ctx.close()
        shutil.rmtree(work, ignore_errors=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
