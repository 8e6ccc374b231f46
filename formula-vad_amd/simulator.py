"""Batch-evaluation harness reproducing the observable behaviour of the reference's `simulator`
executable (src/simulator.zig, src/simulator/SimulationInstance.zig, src/simulator/report_generator.zig)
on top of the C ABI -- SURVEY.md section 8 f1/f3.  Plumbing only (JSON, paths, text); audio decode,
the pipeline, the Evaluator and the statistics all live behind include/fvad.h.

    python -m ... simulator.py -i plan.json           (or: run_plan(path))
    python -m ... simulator.py -i plan.json --export-clips DIR [--clips-pcm16]   (or: run_clips(path, DIR): the plan's speech
                                                      clips, original and denoised, cut and picked on the GPU;
                                                      --clips-denoised-rate 16000 / --clips-original-rate 16000: at NSNet2's rate;
                                                      --clips-original-filter fir: anti-aliased, also at 24000 and 8000;
                                                      --clips-features logmel | fbank: the denoised clips' log-mel or Kaldi
                                                      filter-bank features as .npy)
    python -m ... simulator.py -i plan.json --export-denoised DIR [--denoised-format pcm16|pcm24|f32] [--denoised-rate R|source] [--denoised-source lanes|network]   (or: run_denoise(path,
                                                      DIR): the denoised recordings as WAV files, converted and interleaved
                                                      on the GPU; --denoised-kinds denoised,original,residual,mix
                                                      --denoised-mix W: the time-aligned original, what was removed and a
                                                      wet/dry mix beside them)
    python -m ... simulator.py -i plan.json --sweep   (or: run_sweep(path): every config of the plan, one table row each)
    python -m ... simulator.py -i plan.json --sweep-grid grid.json [--top K] [--devices 0,1]   (or: run_grid(path, grid): a
                                                      parameter grid, every machine scored on the GPU, the top K configs by
                                                      F-score; with --devices the instances dealt round-robin to the GPUs)

Plan schema = the reference's (simulator.zig:41-76, tmp/plan.example.json), unknown fields ignored
(simulator.zig:152-154); audio/ref paths are relative to the plan file (simulator.zig:146,
SimulationInstance.zig:101-104).  Differences, by design:
  * audio files are WAV (PCM16 / float32), not OGG: there is no libsndfile here;
  * instances are not run one-thread-each (simulator.zig:221-232): all channels of all instances on a GPU
    form ONE batch, then the per-instance VAD state machines run on the host; with --devices the
    instances are dealt round-robin to one context + one host thread per GPU;
  * `preload_audio` only changes how samples are pushed in the reference, not the result.
"""
import argparse
import collections
import functools
import itertools
import json
import math
import os
import sys
import threading
import time
from decimal import ROUND_HALF_UP, Decimal

import numpy as np

if __package__:
    from . import binding as fv
else:   # run as a file (python formula-vad_amd/simulator.py): the directory's name is not an identifier, load it as the package
    import importlib.util
    _dir = os.path.dirname(os.path.abspath(__file__))
    _spec = importlib.util.spec_from_file_location("formula_vad_amd", os.path.join(_dir, "__init__.py"),
                                                   submodule_search_locations=[_dir])
    _pkg = importlib.util.module_from_spec(_spec)
    sys.modules["formula_vad_amd"] = _pkg
    _spec.loader.exec_module(_pkg)
    fv = _pkg.binding

VAD_FIELDS = ("speech_min_freq", "speech_max_freq", "long_term_speech_avg_sec", "initial_long_term_avg",
              "short_term_speech_avg_sec", "speech_threshold_factor", "channel_vol_ratio_avg_sec",
              "channel_vol_ratio_threshold", "min_consecutive_sec_to_open", "max_speech_gap_sec",
              "min_vad_duration_sec")


def vad_overrides(cfg_json):
    """VADMachine.Config fields of the plan (VADMachine.zig:30-51) -> binding overrides"""
    out = {}
    for k, v in (cfg_json or {}).items():
        if k == "initial_long_term_avg":
            if v is None:
                out["has_initial_long_term_avg"] = 0
            else:
                out["has_initial_long_term_avg"] = 1
                out["initial_long_term_avg"] = float(v)
        elif k in VAD_FIELDS:
            out[k] = float(v)
    return out


def load_plan(path):
    """-> dict(instances=[{name, audio_path, ref_path}], config={...}, base_path)"""
    with open(path) as f:
        plan = json.load(f)
    base = os.path.dirname(path) or "."
    cfg = plan.get("config", {}) or {}
    vad_cfg = cfg.get("vad_config", {}) or {}
    return {
        "base_path": base,
        "instances": [{"name": i["name"],
                       "audio_path": os.path.normpath(os.path.join(base, i["audio_path"])),
                       "ref_path": os.path.normpath(os.path.join(base, i["ref_path"]))}
                      for i in plan["instances"]],
        "fft_size": int(vad_cfg.get("fft_size", 1024)),
        "vad_machine_config": vad_overrides(vad_cfg.get("vad_machine_config")),
        "alt_vad_machine_configs": [vad_overrides(a) for a in (vad_cfg.get("alt_vad_machine_configs") or [])],
        "denoiser_model_path": vad_cfg.get("denoiser_model_path"),
        "output_dir": cfg.get("output_dir"),
        "preload_audio": bool(cfg.get("preload_audio", False)),
        "audio_read_frame_count": int(cfg.get("audio_read_frame_count", 48000)),
    }


# ------------------------------------------------------------------ Zig-style number formatting
def zig_fixed(x, precision):
    """std.fmt `{d:.N}`: shortest round-trip decimal of the value (as f64), rounded half-up"""
    x = float(x)
    if x != x:
        return "nan"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    q = Decimal(1).scaleb(-precision)
    return str(Decimal(repr(x)).quantize(q, rounding=ROUND_HALF_UP))


def _f(x, width, precision):
    return zig_fixed(x, precision).rjust(width)


DEFINITIONS = (  # report_generator.zig:10-19
    "P   (Positives):                            Total duration of real speech segments (from reference labels)\n"
    "TP  (True positives):                       Duration of correctly detected speech segments\n"
    "FP  (False positives):                      Duration of incorrectly detected speech segments\n"
    "FN  (False negatives):                      Duration of missed speech segments\n"
    "TPR (True positive rate, sensitivity):      Probability that VAD detects a real speech segment. = TP / P \n"
    "PPV (Precision, Positive predictive value): Probability that detected speech segment is true.   = TP / (TP + FP) \n"
    "FNR (False negative rate, miss rate):       Probability that VAD misses a speech segment.       = FN / P \n"
    "FDR (False discovery rate):                 Probability that detected speech segment is false.  = FP / (TP + FP) ")


def report_text(names, stats, agg):
    """report_generator.bufPrintSimulationReport (report_generator.zig:29-116)"""
    out = ["\n\n=> Definitions\n\n" + DEFINITIONS, "\n\n=> Performance Report\n\n"]
    hdr = ("Name", "P", "TP", "FP", "FN", "TPR", "PPV", "FNR (!)", "FDR (!)")
    widths = (30, 4, 4, 4, 4, 6, 6, 8, 8)
    out.append("| " + " | ".join(h.rjust(w) for h, w in zip(hdr, widths)) + " |\n")
    out.append("| " + " | ".join("-" * w for w in widths) + " |\n")
    for name, s in zip(names, stats):
        out.append("| {} | {} | {} | {} | {} | {}% | {}% | {}% | {}% |\n".format(
            name.rjust(30), _f(s.total_positives_sec, 4, 0), _f(s.true_positives_sec, 4, 0),
            _f(s.false_positives_sec, 4, 0), _f(s.false_negatives_sec, 4, 0),
            _f(np.float32(s.true_positive_rate) * np.float32(100), 5, 1),
            _f(np.float32(s.precision) * np.float32(100), 5, 1),
            _f(np.float32(s.false_negative_rate) * np.float32(100), 7, 1),
            _f(np.float32(s.false_discovery_rate) * np.float32(100), 7, 1)))
    out.append("\n=> Aggregate stats \n\n")
    out.append("Total speech duration  (P): {} sec\n".format(_f(agg.total_positives_sec, 7, 1)))
    out.append("True positives        (TP): {} sec\n".format(_f(agg.true_positives_sec, 7, 1)))
    out.append("False positives       (FP): {} sec\n".format(_f(agg.false_positives_sec, 7, 1)))
    out.append("False negatives       (FN): {} sec".format(_f(agg.false_negatives_sec, 7, 1)))
    out.append("    Min.    Avg.    Max. \n")
    for label, a in (("True positive rate   (TPR)", agg.true_positive_rate), ("Precision            (PPV)", agg.precision),
                     ("False negative rate  (FNR)", agg.false_negative_rate), ("False discovery rate (FDR)", agg.false_discovery_rate)):
        p = lambda v: _f(np.float32(v) * np.float32(100), 5, 1)  # noqa: E731
        out.append("{}:   {}%  |  {}% /{}% /{}% \n".format(label, p(a.overall), p(a.min), p(a.avg), p(a.max)))
    out.append("F-Score (β = {})       :   {}% \n".format(_f(agg.f_score_beta, 5, 2), _f(np.float32(agg.f_score) * np.float32(100), 5, 1)))
    out.append("Fowlkes-Mallows index     :   {}% \n".format(_f(np.float32(agg.fm_index) * np.float32(100), 5, 1)))
    return "".join(out)


def audacity_txt(vad_secs, debug_infos, ref_secs, cfg):
    """formats.serializeEvaluatorToAudacityTxt (formats.zig:38-56): VAD segments (sorted by start) with
    their comment, then the reference segments nothing overlapped, labelled "missed".
    (The overlap test of every VAD segment against every reference is one float32 matrix expression: as a Python double loop
    it was 0.44 s per two-hour instance -- 9 s for config 4's plan, ten times its GPU time.)"""
    order = sorted(range(len(vad_secs)), key=lambda i: vad_secs[i][0])
    refs = sorted(ref_secs, key=lambda r: r[0])
    vs = np.array([vad_secs[i] for i in order], np.float32).reshape(-1, 2)
    rs = np.array(refs, np.float32).reshape(-1, 2)
    # overlap = f32(min(ends)) - f32(max(starts)) > 0, as SpeechSegment.overlap computes it (SpeechSegment.zig:22-57)
    ov = (np.minimum(vs[:, 1, None], rs[None, :, 1]) - np.maximum(vs[:, 0, None], rs[None, :, 0])) > 0
    v_matched = ov.any(axis=1) if rs.shape[0] else np.zeros(vs.shape[0], bool)
    r_matched = ov.any(axis=0) if vs.shape[0] else np.zeros(rs.shape[0], bool)
    lines = []
    for j, i in enumerate(order):
        v = vad_secs[i]
        comment = debug_infos[i] if v_matched[j] else "UNMATCHED " + debug_infos[i]
        lines.append("{}\t{}\t{}\n".format(zig_fixed(v[0], 4), zig_fixed(v[1], 4), comment))
    for k, r in enumerate(refs):
        if not r_matched[k]:
            lines.append("{}\t{}\t{}\n".format(zig_fixed(r[0], 4), zig_fixed(r[1], 4), "missed"))
    return "".join(lines)


def _make_ctx(plan, device, synth_seed):
    ctx = fv.Context(device)
    if plan["denoiser_model_path"]:
        ctx.load_onnx(os.path.join(plan["base_path"], plan["denoiser_model_path"]))
    elif os.path.exists("data/nsnet2-20ms-baseline.onnx"):   # NSNet2.zig:56 default
        ctx.load_onnx("data/nsnet2-20ms-baseline.onnx")
    else:
        if synth_seed is None:
            ctx.close()
            raise FileNotFoundError("no denoiser_model_path in the plan and no data/nsnet2-20ms-baseline.onnx "
                                    "(pass synth_seed to run on random-init weights)")
        ctx.load_synth(synth_seed)
    return ctx


def _run_instances(ctx, plan, audio):
    """The path for a set of instances on one context: ONE GPU batch over all their channels, then the
    per-instance VAD state machines on the host.  Returns [(segments, audit)] in the order given."""
    if not audio:
        return []
    lanes = [pcm[c] for pcm in audio for c in range(pcm.shape[0])]
    vm = plan["vad_machine_config"]
    bin_w = np.float32(48000) / np.float32(plan["fft_size"])  # band edges: FFT.freqToBin (FFT.zig:156-167)
    min_bin = int(np.round(np.float32(vm.get("speech_min_freq", 500.0)) / bin_w))
    max_bin = int(np.round(np.float32(vm.get("speech_max_freq", 2000.0)) / bin_w))
    res = ctx.engine_run(lanes, min_bin=min_bin, max_bin=max_bin, fft_size=plan["fft_size"])
    first = np.cumsum([0] + [pcm.shape[0] for pcm in audio])

    def host_stage(i):
        r = res[first[i]:first[i] + audio[i].shape[0]]
        return _vad_host_stage(plan, np.stack([x["band_sum"] for x in r]), np.stack([x["chunk_rms"] for x in r]))

    return _map_instances(host_stage, len(audio))


def _vad_host_stage(plan, band, rms):
    """The host stage of one instance: the library's batched form (frame metadata + VAD state machine) over the engine's band
    sums [channel][frame] and chunk RMS [channel][chunk] -> (segments, audit)"""
    band, rms = np.ascontiguousarray(band), np.ascontiguousarray(rms)
    vb = fv.VadBatch(1, n_channels=band.shape[0], fft_size=plan["fft_size"], overrides=plan["vad_machine_config"])
    try:
        segs = vb.run(band, rms)[0] if band.shape[1] else []
        return segs, vb.audit(0)
    finally:
        vb.close()


def _map_instances(host_stage, n):
    """host_stage(i) for every instance, side by side on host threads, like the reference's thread per file
    (simulator.zig:221-232): a two-hour stream's state machine is 36 ms on one core, 21 of them one after the other were
    as long as the GPU's part of the plan (instances differ in length and channel count: one call each)"""
    from concurrent.futures import ThreadPoolExecutor
    n_workers = max(1, min(n, os.cpu_count() or 1, 16))
    if n_workers == 1:
        return [host_stage(i) for i in range(n)]
    with ThreadPoolExecutor(max_workers=n_workers) as pool:
        return list(pool.map(host_stage, range(n)))


# (the reference refuses such a file; here the GPU resamples it while it is ingested)
OTHER_RATE_HINT = "a file that is not at 48 kHz is resampled on the GPU only: run with --ingest device (ingest='device')"


def _read_instance(inst):
    try:    # PCM16 files stay 16-bit all the way to the GPU (half the PCIe / HBM bytes; converted by the kernel
        pcm, sr = fv.wav_read_i16(inst["audio_path"])   # that reads them, bit-identical to converting first)
    except fv.FvadError:
        pcm, sr = fv.wav_read(inst["audio_path"])
    if sr != 48000:
        raise fv.FvadError(-9, f"{inst['name']}: sample rate {sr}", OTHER_RATE_HINT)   # VADPipeline.zig:55-58
    with open(inst["ref_path"], "rb") as f:
        return pcm, fv.parse_audacity(f.read())


def _read_labels(inst):
    with open(inst["ref_path"], "rb") as f:
        return fv.parse_audacity(f.read())


def _map_audio(inst):
    """an instance's audio mapped, not read (fv.wav_map): [n_frames][n_channels] int16 or float32"""
    pcm, sr = fv.wav_map(inst["audio_path"])
    if sr != 48000:
        raise fv.FvadError(-9, f"{inst['name']}: sample rate {sr}", OTHER_RATE_HINT)   # VADPipeline.zig:55-58
    return pcm


INGESTS = ("host", "device")


@functools.lru_cache(maxsize=None)
def _resample_design(rate):
    """(up, down, taps) of a file rate: fvad_resample_ratio to 48 kHz and fvad_resample_design's default taps, made once per rate"""
    up, down = fv.resample_ratio(rate, 48000)
    return up, down, fv.resample_design(up, down)


class _RawAudio:
    """An instance's audio for ingest="device": the bytes of its file's data chunk, mapped and interleaved as the file holds
    them (fv.wav_map_raw), which fvad_ingest de-interleaves and decodes on the GPU.  n_channels and n_frames are what the
    harness needs of a loaded instance (_dims); it is no array.
    A file at another rate (`rate` != 48000) is resampled while it is ingested (fvad_ingest_resample, _resample_design's ratio
    and taps): n_frames is then its 48 kHz output count and `source` takes 48 kHz coordinates, so that everything downstream
    sees an ordinary 48 kHz instance; file_frames is what the file holds."""

    def __init__(self, raw, info):
        self.raw, self.format = raw, info["format"]
        self.n_channels, self.n_frames = info["n_channels"], info["n_frames"]
        self.frame_bytes = self.n_channels * (info["bits"] // 8)
        self.rate = info.get("sample_rate", 48000)
        if self.rate != 48000:
            self.up, self.down, self.taps = _resample_design(self.rate)
            self.file_frames = info["n_frames"]
            self.n_frames = fv.resample_out_frames(self.file_frames, self.up, self.down)

    def source(self, frame_from, frame_to, first_lane, dst_offset, fill_to):
        """the fvad_ingest source row of frames [frame_from, frame_to); frame_to <= frame_from (a slice behind the file's end):
        a row without frames at byte 0, which only fills.  At another rate: the fvad_ingest_resample row of the 48 kHz outputs
        [frame_from, frame_to), whose given frames are exactly the window of that range (fvad_resample_window)"""
        n = max(frame_to - frame_from, 0)
        if self.rate == 48000:
            return (frame_from * self.frame_bytes if n else 0, n, self.n_channels, self.format, first_lane, dst_offset, fill_to)
        lo, hi = fv.resample_window(self.up, self.down, self.taps.size, self.file_frames, frame_from, n) if n else (0, 0)
        return (lo * self.frame_bytes, hi - lo, self.n_channels, self.format, first_lane, dst_offset, fill_to,
                lo, self.file_frames, frame_from if n else 0, n)


def _ingest_rows(ctx, members, rows, **lanes):
    """The sources `rows` of the instances `members` (_RawAudio each) into the lanes: one fvad_ingest call for the 48 kHz members
    and one fvad_ingest_resample call per other rate present (one ratio and one set of taps per call)."""
    by_rate = {}
    for a, row in zip(members, rows):
        by_rate.setdefault(a.rate, []).append((a, row))
    for rate, pairs in by_rate.items():
        raws, rs = [a.raw for a, _ in pairs], [r for _, r in pairs]
        if rate == 48000:
            ctx.ingest(rs, raw=raws, **lanes)
        else:
            a = pairs[0][0]
            ctx.ingest_resample(rs, a.up, a.down, a.taps, raw=raws, **lanes)


def _dims(a, mapped=False):
    """(n_channels, n_frames) of a loaded instance: a _RawAudio's own, or the shape of the array the host path loads --
    [n_channels][n_frames] where it reads the files, [n_frames][n_channels] where it maps them (mapped: the sliced grid)"""
    if isinstance(a, _RawAudio):
        return a.n_channels, a.n_frames
    return (a.shape[1], a.shape[0]) if mapped else (a.shape[0], a.shape[1])


def _raw_audio(inst):
    raw, info = fv.wav_map_raw(inst["audio_path"])
    if info["sample_rate"] != 48000:
        try:   # any rate with a ratio to 48 kHz that fvad_resample_ratio takes (up <= 640) is resampled by the ingest
            fv.resample_ratio(info["sample_rate"], 48000)
        except fv.FvadError:
            raise fv.FvadError(-9, f"{inst['name']}: sample rate {info['sample_rate']}", "no ratio to 48000 with up <= 640") from None
    if info["n_channels"] > 64:
        raise fv.FvadError(fv.FVAD_ERR_INVALID_ARGUMENT, inst["name"], f"{info['n_channels']} channels: fvad_ingest takes 64")
    return _RawAudio(raw, info)


def _check_ingest(ingest):
    if ingest not in INGESTS:
        raise ValueError(f"ingest: {ingest!r} (one of {', '.join(INGESTS)})")


def _load_instances(plan, ingest, mapped=False):
    """[(audio, labels)] per instance.  ingest "host": the files read (_read_instance), or mapped for the sliced grid
    (_map_audio); a file those refuse that fvad_wav_probe takes -- 24-bit PCM -- is refused with a pointer to the other way.
    ingest "device": every file mapped as bytes (_RawAudio), nothing read."""
    if ingest == "device":
        return [(_raw_audio(i), _read_labels(i)) for i in plan["instances"]]
    loaded = []
    for i in plan["instances"]:
        try:
            loaded.append((_map_audio(i), _read_labels(i)) if mapped else _read_instance(i))
        except fv.FvadError as e:
            try:
                pcm24 = fv.wav_probe(i["audio_path"])["format"] == fv.INGEST_PCM24
            except fv.FvadError:
                pcm24 = False
            if not pcm24:
                raise
            raise fv.FvadError(e.status, f"{i['name']}: {i['audio_path']}",
                               "24-bit PCM is decoded on the GPU only: run with --ingest device (ingest='device')") from e
    return loaded


def _is_raw(audio):
    return bool(audio) and isinstance(audio[0], _RawAudio)


def instance_shares(n_instances, n_devices):
    """How run_plan and run_grid deal a plan's instances to n_devices contexts: instance i to share i % n_devices, each share
    in plan order -> [[instance]] per share (a share may be empty)"""
    return [[i for i in range(n_instances) if i % n_devices == d] for d in range(n_devices)]


def _evaluate(plan, per_inst, refs):
    """Evaluator + statistics + the report of a plan's per-instance (segments, audit), and the files of output_dir
    (simulator.zig:127-132,157-168) -> (report text, per-instance results)"""
    vm = plan["vad_machine_config"]
    # --- Evaluator + statistics (simulator.zig:127-132)
    stat_cfg = {"ignore_shorter_than_sec": float(np.float32(vm.get("min_vad_duration_sec", 0.7))),
                "extrude_start": 5.0, "extrude_end": 10.0, "fill_gaps": 5.0}
    names, stats, results = [], [], []
    for inst, (segs, audit), ref in zip(plan["instances"], per_inst, refs):
        secs = [(float(np.float32(s[0]) / np.float32(48000)), float(np.float32(s[1]) / np.float32(48000))) for s in segs]
        infos = ["vr:{} vad:{}s".format(zig_fixed(s[2], 2), zig_fixed(s[3], 1)) for s in segs]  # SimulationInstance.zig:240-244
        st = fv.stats_from_segments(secs, ref, stat_cfg)
        names.append(inst["name"])
        stats.append(st)
        results.append({"name": inst["name"], "segments": segs, "segments_sec": secs, "debug_info": infos,
                        "stats": st, "audacity": audacity_txt(secs, infos, ref, stat_cfg), "audit": audit})
    agg = fv.stats_aggregate(stats)
    text = report_text(names, stats, agg)
    if plan["output_dir"]:
        out_dir = os.path.join(plan["base_path"], plan["output_dir"], str(int(time.time())))  # simulator.zig:157-168
        os.makedirs(out_dir, exist_ok=True)
        for r in results:
            with open(os.path.join(out_dir, f"{r['name']}-audacity.txt"), "w") as f:
                f.write(r["audacity"])
        with open(os.path.join(out_dir, "report.txt"), "w") as f:
            f.write(text)
    return text, results


def run_plan(plan_path, ctx=None, synth_seed=None, out=sys.stdout, devices=None):
    """Runs a whole plan; returns (report_text, per_instance_results).

    devices: list of HIP device indices -- one context and one host thread per entry, instance i on
    devices[i % len(devices)] (the reference's unit of parallelism is the instance: one thread per file,
    simulator.zig:221-232; here one thread per GPU with that GPU's instances as one batch).  The report is built
    from the per-instance statistics in PLAN order whatever the split (report_generator.zig:48-68,
    statistics.zig:116-172), so it is identical for every device list."""
    import threading
    plan = load_plan(plan_path)
    own_ctx = ctx is None
    if own_ctx:
        ctxs = [_make_ctx(plan, d, synth_seed) for d in (devices or [0])]
    else:
        ctxs = [ctx]
    read_instance = _read_instance

    # the files side by side (the reference opens them on a thread each, SimulationInstance.zig:144-152): reading and
    # de-interleaving a two-hour file is most of a plan's wall time once the GPU does the rest
    from concurrent.futures import ThreadPoolExecutor
    n_readers = max(1, min(len(plan["instances"]), os.cpu_count() or 1, 8))
    if n_readers == 1:
        loaded = [read_instance(i) for i in plan["instances"]]
    else:
        with ThreadPoolExecutor(max_workers=n_readers) as pool:
            loaded = list(pool.map(read_instance, plan["instances"]))
    audio = [a for a, _ in loaded]
    refs = [r for _, r in loaded]
    t0 = time.perf_counter()
    n_ctx = len(ctxs)
    parts = instance_shares(len(audio), n_ctx)
    done = [None] * n_ctx
    errs = []

    def work(d):
        try:
            done[d] = _run_instances(ctxs[d], plan, [audio[i] for i in parts[d]])
        except Exception as e:  # re-raised below, in the caller's thread
            errs.append(e)

    if n_ctx == 1:
        work(0)
    else:
        th = [threading.Thread(target=work, args=(d,)) for d in range(n_ctx)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    if errs:
        raise errs[0]
    per_inst = [None] * len(audio)
    for d in range(n_ctx):
        for i, r in zip(parts[d], done[d]):
            per_inst[i] = r
    elapsed = time.perf_counter() - t0
    text, results = _evaluate(plan, per_inst, refs)
    if out is not None:
        out.write(text)
        audio_s = sum(p.shape[1] for p in audio) / 48000.0
        out.write(f"\n[{audio_s:.0f} s of audio in {elapsed:.2f} s = {audio_s / elapsed:.0f}x realtime]\n")
    if own_ctx:
        for c in ctxs:
            c.close()
    return text, results


CLIP_RATES = {48000: 1, 16000: 3}                  # a clip kind's rate -> the export's step
CLIP_PHASE = {"denoised": 2, "original": 0}        # the lane indices (mod 3) kept at 16 kHz: the interpolator's native samples
                                                   # (resample.zig:32-79); what downsampleAudio feeds NSNet2 (resample.zig:9-29)


CLIP_FIR_RATES = {24000: 2, 16000: 3, 8000: 6}     # a filtered kind's rate -> the export's step (48000 would leave the filter nothing to do)
CLIP_FILTERS = ("none", "fir", "resample")


def _clip_resample(kind, rate):
    """the filter of a kind exported through the resampling gather at `rate`: up/down = rate/48000 in lowest terms and
    fvad_resample_design's default taps, its parameters spelt out for the manifest; ValueError for a rate that has none"""
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or rate <= 0 or rate == 48000 or rate >= 1 << 32:
        raise ValueError(f"run_clips: {kind}_rate {rate!r} with {kind}_filter 'resample' is no rate other than 48000")
    try:
        up, down = fv.resample_ratio(48000, int(rate))
        taps = fv.resample_design(up, down)
    except fv.FvadError:
        raise ValueError(f"run_clips: {kind}_rate {rate!r} with {kind}_filter 'resample': no ratio to 48000 with up <= {fv.RESAMPLE_UP_MAX} "
                         f"whose default design fits {fv.RESAMPLE_TAPS_MAX} taps") from None
    if fv.clips_resample_check(up, down, taps) != 0:
        raise ValueError(f"run_clips: {kind}_rate {rate!r} with {kind}_filter 'resample': the filter's window fits no tile of the gather")
    m = max(up, down)
    return {"up": up, "down": down, "half": 16, "cutoff": 0.45 / m, "beta": 6.0, "taps": taps}


def _clip_rates(original_rate, denoised_rate, original_filter="none", denoised_filter="none"):
    """-> ({kind: rate}, {kind: None, or the filter of a filtered kind}); raises ValueError for what run_clips does not offer"""
    rates, firs = {"original": original_rate, "denoised": denoised_rate}, {}
    for kind, filt in (("original", original_filter), ("denoised", denoised_filter)):
        rate = rates[kind]
        if filt not in CLIP_FILTERS:
            raise ValueError(f"run_clips: {kind}_filter {filt!r} is none of 'none', 'fir' and 'resample'")
        if filt == "none":
            if rate not in CLIP_RATES:
                raise ValueError(f"run_clips: {kind}_rate {rate!r} is neither 48000 nor 16000")
            firs[kind] = None
            continue
        if filt == "resample":
            firs[kind] = _clip_resample(kind, rate)
            continue
        if rate not in CLIP_FIR_RATES:
            raise ValueError(f"run_clips: {kind}_rate {rate!r} with {kind}_filter 'fir' is none of 24000, 16000 and 8000")
        step = CLIP_FIR_RATES[rate]
        # the default design of fvad_clips_fir_design for the step, its parameters spelt out for the manifest
        firs[kind] = {"step": step, "half": 16 * step, "cutoff": 0.45 / step, "beta": 6.0, "taps": fv.clips_fir_design(step)}
    return rates, firs


def _clip_skips(kind, rate, sample_from, fir=None):
    """(step, skips or None, taps or None) of one export of `kind` clips starting at the absolute lane indices sample_from.  At
    step 3 a filtered kind keeps the lane indices an unfiltered run keeps (first_sample agrees); at steps 2 and 6 phase 0.  A
    resampled kind has neither step nor skips: its phase starts at the clip (_clip_export_args adds up and down)"""
    if fir is not None and "up" in fir:
        return 1, None, fir["taps"]
    if fir is None:
        step = CLIP_RATES[rate]
        return (1, None, None) if step == 1 else (step, fv.clips_phase_skips(sample_from, step, CLIP_PHASE[kind]), None)
    step = fir["step"]
    return step, fv.clips_phase_skips(sample_from, step, CLIP_PHASE[kind] if step == 3 else 0), fir["taps"]


def _clip_export_args(kind, rate, sample_from, fir):
    """-> (the keyword arguments of one clips_export / clips_export_split of `kind`, skips or None, whether the result has out_lens)"""
    step, skips, taps = _clip_skips(kind, rate, sample_from, fir)
    kw = dict(step=step, skips=skips, taps=taps)
    if fir is not None and "up" in fir:
        kw.update(up=fir["up"], down=fir["down"])
    return kw, skips, step != 1 or "up" in kw


def _write_clip(path, samples, pcm16, rate):
    (fv.wav_write_i16 if pcm16 else fv.wav_write)(path, samples, rate)


def _clip_entry(path, best_channel, best_rms, runner_up_rms, rate, first_sample, length, fir=None):
    """a kind's manifest entry; a kind at 48 kHz has the keys it always had, an unfiltered kind at 16 kHz too"""
    e = {"file": os.path.basename(path), "best_channel": int(best_channel), "best_rms": float(best_rms), "runner_up_rms": float(runner_up_rms)}
    if rate != 48000:
        e.update(sample_rate=rate, first_sample=int(first_sample), length=int(length))
    if fir is not None and "up" in fir:
        e["filter"] = {"design": "kaiser_sinc_polyphase", "up": fir["up"], "down": fir["down"], "half": fir["half"], "cutoff": fir["cutoff"],
                       "beta": fir["beta"], "taps": int(len(fir["taps"]))}
    elif fir is not None:
        e["filter"] = {"design": "kaiser_sinc", "half": fir["half"], "cutoff": fir["cutoff"], "beta": fir["beta"], "taps": int(len(fir["taps"]))}
    return e


CLIP_FEATURES = (None, "logmel", "fbank")
CLIP_FEATURES_NORM = {None: None, "whisper": (8.0, 4.0, 0.25)}   # (range, offset, scale), the maximum taken per clip
CLIP_FEATURES_NORM_OF = {"logmel": (None, "whisper"), "fbank": (None, "cmn")}   # the norms each kind of features takes
# Whisper's front end on NSNet2's own 16 kHz samples: step 3 at the denoised kind's phase, 400-point periodic Hann, hop 160,
# 80 Slaney bands over 0 .. 8 kHz, log10(max(., 1e-10))
LOGMEL = dict(step=3, n_fft=400, hop=160, n_mels=80, sample_rate=16000, fmin=0.0, fmax=8000.0, floor=1e-10)
# Kaldi's fbank (compute-fbank-feats, torchaudio.compliance.kaldi.fbank) on the same samples: frames of 400 from t * 160 on
# (snip_edges), DC removed, pre-emphasis 0.97, Povey window, 512-point transform, 80 HTK-mel triangles over 20 Hz .. Nyquist,
# ln(max(., FLT_EPSILON)); samples scaled by 32768, Kaldi's convention
FBANK = dict(step=3, win_length=400, n_fft=512, hop=160, n_mels=80, sample_rate=16000, low_freq=20.0, high_freq=0.0, preemph=0.97,
             remove_dc=1, scale=32768.0, floor=fv.FLT_EPSILON)


def _check_features(features, features_norm, slice_chunks, features_sliced=False):
    """ValueError for what run_clips does not offer with features, before any work"""
    if features not in CLIP_FEATURES:
        raise ValueError(f"features = {features!r}: one of {CLIP_FEATURES}")
    if features_norm not in CLIP_FEATURES_NORM and features_norm != "cmn":
        raise ValueError(f"features_norm = {features_norm!r}: one of {tuple(CLIP_FEATURES_NORM) + ('cmn',)}")
    if features is None and features_norm is not None:
        raise ValueError("features_norm needs features")
    if features is not None and features_norm not in CLIP_FEATURES_NORM_OF[features]:
        raise ValueError(f"features_norm = {features_norm!r} with features = {features!r}: one of {CLIP_FEATURES_NORM_OF[features]}")
    if features_sliced and (features is None or slice_chunks is None):
        raise ValueError("features_sliced (--clips-features-sliced) needs both features and slice_chunks")
    # the gate: sliced features are opt-in, so that a run written for the refusal still gets it
    if features is not None and slice_chunks is not None and not features_sliced:
        raise ValueError("features with slice_chunks: the split-source form of the feature export (fvad_clips_export_split_mel / "
                         "_split_fbank) is opt-in: pass features_sliced=True (--clips-features-sliced)")


def logmel_window():
    """the periodic Hann window of LOGMEL's n_fft, float32"""
    n = LOGMEL["n_fft"]
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(np.float32)


def fbank_window():
    """Kaldi's Povey window of FBANK's win_length, evaluated in double and rounded once"""
    n = FBANK["win_length"]
    return ((0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1))) ** 0.85).astype(np.float32)


# what _features_share and _features_split take per kind of features: the parameters, the stream lengths L that have a frame (the
# skip rule), the export's call with the kind's window and designer (src: the contiguous call's source, or with split the split
# call's (a, b, src_pcm16)), and the manifest entry
_FEATURES = {
    "logmel": dict(
        p=LOGMEL, keeps=lambda p, L: L >= p["n_fft"] // 2 + 1 and L >= p["hop"],
        export=lambda ctx, p, src, rows, skips, norm, split=False: (ctx.clips_export_split_mel if split else ctx.clips_export_mel)(
            *src, rows, logmel_window(), fv.mel_design(p["sample_rate"], p["n_fft"], p["n_mels"], p["fmin"], p["fmax"]), step=p["step"], skips=skips, hop=p["hop"], floor=p["floor"], norm=CLIP_FEATURES_NORM[norm]),
        entry=lambda p, file, T, first, res, j, norm: {
            "file": file, "frames": T, "n_mels": p["n_mels"], "n_fft": p["n_fft"], "hop": p["hop"],
            "sample_rate": p["sample_rate"], "first_sample": first, "best_channel": int(res["best_channel"][j]),
            "max": float(res["feat_max"][j]), "floor": p["floor"], "norm": norm,
            "mel": {"design": "slaney", "fmin": p["fmin"], "fmax": p["fmax"]}}),
    "fbank": dict(
        p=FBANK, keeps=lambda p, L: L >= p["win_length"],
        export=lambda ctx, p, src, rows, skips, norm, split=False: (ctx.clips_export_split_fbank if split else ctx.clips_export_fbank)(
            *src, rows, fbank_window(), fv.mel_design_kaldi(p["sample_rate"], p["n_fft"], p["n_mels"], p["low_freq"], p["high_freq"]), n_fft=p["n_fft"], step=p["step"], skips=skips, hop=p["hop"], scale=p["scale"], preemph=p["preemph"],
            remove_dc=p["remove_dc"], floor=p["floor"], cmn=norm == "cmn"),
        entry=lambda p, file, T, first, res, j, norm: dict({
            "file": file, "kind": "fbank", "frames": T, "n_mels": p["n_mels"], "win_length": p["win_length"],
            "n_fft": p["n_fft"], "hop": p["hop"], "sample_rate": p["sample_rate"], "first_sample": first,
            "best_channel": int(res["best_channel"][j]), "window": "povey", "preemph": p["preemph"], "remove_dc": bool(p["remove_dc"]),
            "scale": p["scale"], "snip_edges": True, "log": "ln", "floor": p["floor"], "norm": norm,
            "mel": {"design": "kaldi", "low_freq": p["low_freq"], "high_freq": p["high_freq"]}},
            **({"means": [float(v) for v in res["means"][j]]} if norm == "cmn" else {}))),
}


def _features_share(ctx, r, insts, per_inst, lane0, n_channels, avail, out_dir, manifests, features_norm, features="logmel"):
    """the features of run_clips: one fvad_clips_export_mel (or fvad_clips_export_fbank) over the denoised lanes' clips,
    NAME-####-denoised.logmel.npy (.fbank.npy) per clip and its manifest entry under "features".  A clip too short for one
    reflected frame (for one frame of 400) has no entry and is counted in features_skipped"""
    fam = _FEATURES[features]
    p = fam["p"]
    rows, owner = [], []
    for i, (segs, _) in enumerate(per_inst):
        clips, _ = fv.clips_from_segments(segs, lane0[i], n_channels[i], avail[i])
        manifests[i]["features_skipped"] = 0
        k = 0
        for c in clips:
            while (segs[k][0], segs[k][1]) != (c[2], c[3]):
                k += 1
            skip = int(fv.clips_phase_skips(c[2:3], p["step"], CLIP_PHASE["denoised"])[0])
            if fam["keeps"](p, -(-(int(c[3] - c[2]) - skip) // p["step"])):
                rows.append(c)
                owner.append((i, k))
            else:
                manifests[i]["features_skipped"] += 1
            k += 1
    if not rows:
        return
    rows = np.array(rows, np.uint64)
    skips = fv.clips_phase_skips(rows[:, 2], p["step"], CLIP_PHASE["denoised"])
    res = fam["export"](ctx, p, (r.d_den, False, r.n_lanes, r.n_den, r.n_den), rows, skips, features_norm)
    for j, (i, k) in enumerate(owner):
        o, T = int(res["offsets"][j]), int(res["n_frames"][j])
        path = os.path.join(out_dir, "{}-{:04d}-denoised.{}.npy".format(insts[i]["name"], k, features))
        np.save(path, res["out"][o:o + T * p["n_mels"]].reshape(T, p["n_mels"]))
        manifests[i]["clips"][k]["features"] = fam["entry"](p, os.path.basename(path), T, int(rows[j, 2]) + int(skips[j]), res, j, features_norm)


def _features_split(ctx, a, b, rows, owner, insts, out_dir, feats, skipped, features, features_norm):
    """the features of a sliced run_clips: one fvad_clips_export_split_mel (or _split_fbank) over the denoised kind's due clips of
    a slice -- the split rows of its clip export over the held tail `a` and the slice's lanes `b`, owner[q] = (instance, segment,
    absolute sample_from) --, the files and entries of _features_share: the skips from the absolute sample_from, first_sample
    absolute.  feats[i][segment] gets the entry; a clip too short for a frame is counted in skipped[i]"""
    fam = _FEATURES[features]
    p = fam["p"]
    skips = fv.clips_phase_skips([a0 for _, _, a0 in owner], p["step"], CLIP_PHASE["denoised"])
    keep = []
    for q, (r, (i, _, _)) in enumerate(zip(rows, owner)):
        if fam["keeps"](p, -(-(int(r[3] + r[6]) - int(skips[q])) // p["step"])):
            keep.append(q)
        else:
            skipped[i] += 1
    if not keep:
        return
    res = fam["export"](ctx, p, (a, b, False), [rows[q] for q in keep], skips[keep], features_norm, split=True)
    for u, q in enumerate(keep):
        i, j, a0 = owner[q]
        o, T = int(res["offsets"][u]), int(res["n_frames"][u])
        path = os.path.join(out_dir, "{}-{:04d}-denoised.{}.npy".format(insts[i]["name"], j, features))
        np.save(path, res["out"][o:o + T * p["n_mels"]].reshape(T, p["n_mels"]))
        feats[i][j] = fam["entry"](p, os.path.basename(path), T, a0 + int(skips[q]), res, u, features_norm)


def _clips_share(ctx, plan, insts, audio, out_dir, pcm16, rates, firs, features=None, features_norm=None):
    """run_clips for the instances of one context -> [(segments, audit, manifest)] in the order given"""
    if not audio:
        return []
    held = []

    def dalloc(nbytes):
        held.append(ctx.device_alloc(max(int(nbytes), 4)))
        return held[-1]

    try:
        F, chunk = plan["fft_size"], 24000
        r = _denoise_resident(ctx, audio, F, plan["vad_machine_config"], dalloc)
        band = np.zeros((r.n_lanes, max(r.nf_all, 1)), np.float32)
        if r.nf_all:
            ctx.to_host(band, r.d_band0)
        lane0, l = {}, 0
        for i in r.order:
            lane0[i] = l
            l += _dims(audio[i])[0]

        def host_stage(i):
            C_, nck = _dims(audio[i])[0], r.n_chunks[i]
            return _vad_host_stage(plan, band[lane0[i]:lane0[i] + C_, :nck * chunk // F], r.rms[lane0[i]:lane0[i] + C_, :nck])

        per_inst = _map_instances(host_stage, len(audio))
        # one export per kind over every instance's clips: the reference's two recorders, each picking from its own audio
        kinds = (("original", r.d_pcm, r.stride, r.n_samples, [_dims(a)[1] for a in audio]),
                 ("denoised", r.d_den, r.n_den, r.n_den, [n * chunk for n in r.n_chunks]))
        manifests = [{"name": inst["name"], "sample_rate": 48000, "pcm16": bool(pcm16), "clips": [
            {"segment": k, "start": int(s[0]), "length": int(s[1] - s[0])} for k, s in enumerate(segs)]} for inst, (segs, _) in zip(insts, per_inst)]
        for kind, d_src, stride, n_samples, avail in kinds:
            rows, owner = [], []
            for i, (segs, _) in enumerate(per_inst):
                clips, skipped = fv.clips_from_segments(segs, lane0[i], _dims(audio[i])[0], avail[i])
                manifests[i][f"{kind}_skipped"] = skipped
                rows.append(clips)
                k = 0
                for c in clips:   # the clips are the kept segments, in order
                    while (segs[k][0], segs[k][1]) != (c[2], c[3]):
                        k += 1
                    owner.append((i, k))
                    k += 1
            rows = np.concatenate(rows) if rows else np.zeros((0, fv.CLIP_FIELDS), np.uint64)
            if not rows.shape[0]:
                continue
            kw, skips, has_lens = _clip_export_args(kind, rates[kind], rows[:, 2], firs[kind])
            res = ctx.clips_export(d_src, False, r.n_lanes, stride, n_samples, rows, out_pcm16=pcm16, **kw)
            lens = res["out_lens"] if has_lens else rows[:, 3] - rows[:, 2]
            for j, (i, k) in enumerate(owner):
                o, n = int(res["offsets"][j]), int(lens[j])
                path = os.path.join(out_dir, "{}-{:04d}-{}.wav".format(insts[i]["name"], k, kind))
                _write_clip(path, res["out"][o:o + n], pcm16, rates[kind])
                manifests[i]["clips"][k][kind] = _clip_entry(path, res["best_channel"][j], res["best_rms"][j], res["runner_up_rms"][j], rates[kind],
                                                             int(rows[j, 2]) + (0 if skips is None else int(skips[j])), n, firs[kind])
        if features is not None:
            _features_share(ctx, r, insts, per_inst, lane0, [_dims(a)[0] for a in audio], [n * chunk for n in r.n_chunks], out_dir, manifests,
                            features_norm, features)
        return [(segs, audit, m) for (segs, audit), m in zip(per_inst, manifests)]
    finally:
        for d in held:
            ctx.device_free(d)


def run_clips(plan_path, out_dir, pcm16=False, ctx=None, synth_seed=None, devices=None, ingest="host", slice_chunks=None, info=None,
              denoised_rate=48000, original_rate=48000, original_filter="none", denoised_filter="none", features=None, features_norm=None,
              features_sliced=False):
    """The plan's speech clips -- what main.zig writes out for the recogniser downstream: one original and one denoised
    single-channel clip per completed segment, the quietest channel over the clip (Recorder.zig:113-164), cut and picked on the
    GPU so that only the clips cross PCIe.  Per share of instances (dealt to `devices` like run_plan): the instances denoised
    device-resident (_denoise_resident), the plan's vad_machine_config per instance (run_plan's host stage),
    fvad_clips_from_segments, one export of the original and one of the denoised clips, then
    NAME-####-original.wav / NAME-####-denoised.wav (float32, or PCM16 with pcm16) and NAME-clips.json per instance in out_dir:
    per segment its start and length in samples and, of each kind, the file, the best channel and both RMS values; a kind whose
    audio ends before the segment does has no entry there and is counted in KIND_skipped (the denoised audio ends with the last
    whole chunk).  Returns run_plan's (report text, results), each result with its manifest under "clips".
    Segments and report are run_plan's whenever both passes select the same NSNet2 kernels (fvad_ctx_last_nn_path): the resident
    pass pads every lane to the longest instance, so a plan of unequal lengths may be cut into other launches (the context option
    "reproducible" makes the two agree bit for bit for every plan).
    ingest "device": the files' bytes go to the GPU as they are and are decoded there (run_grid); the same clips and manifests.
    With it a file at another rate (44.1 kHz, 16 kHz ...) is resampled to 48 kHz while it is ingested (fvad_ingest_resample,
    the default design): segments, manifests and reports stay in 48 kHz terms, and the clips of such an instance -- the
    "original" kind too -- are clips of the RESAMPLED audio, not of the file's own samples.
    slice_chunks N: the same files, manifests, report and return value from time slices of N chunks (_clips_sliced_share), the
    device memory bounded by a slice and the held tails instead of the corpus; None is the resident path above.
    info (a dict): filled with "held_peak_bytes", the most device memory the held tails took on one context, and "slices".
    denoised_rate / original_rate (48000 or 16000; anything else raises before any work): at 16000 a kind's clips are every third
    sample of what 48000 gives -- fvad_clips_export*_strided, so that only they cross PCIe -- picked as at 48000, over every
    sample.  The denoised kind keeps the lane indices = 2 (mod 3): K3's interpolator writes [lerp, lerp, sample] per 16 kHz
    sample, so these are NSNet2's own output and nothing is lost.  The original kind keeps the indices = 0 (mod 3), the
    reference's downsampleAudio: what NSNet2 was fed, WITHOUT an anti-alias filter -- it aliases exactly as the network's input
    does.  The files then say 16000 and the kind's manifest entries gain "sample_rate", "first_sample" (the absolute 48 kHz index
    of the first kept sample) and "length"; at 48000 files and manifests are byte for byte what they were.
    original_filter / denoised_filter ("none" or "fir"): with "fir" that kind's clips are low-pass filtered while they are
    decimated -- fvad_clips_export*_fir with fvad_clips_fir_design's default taps for the step (Kaiser-windowed sinc, 32 step + 1
    taps, cutoff 0.45 / step) -- and its rate may be 24000, 16000 or 8000 (steps 2, 3, 6); 48000 raises, like every other
    combination run_clips does not offer, before any work.  Each clip is filtered as a finite signal (zeros outside it), so a
    file is what filtering and decimating the 48000 file with the same taps gives, and a sliced run holds no more audio than
    before.  The pick and both RMS values are still taken over every unfiltered sample.  At 16000 the kept lane indices, hence
    "first_sample" and "length", are those of the unfiltered run; at 24000 and 8000 they are the indices = 0 (mod step).  A
    filtered kind's manifest entries gain "filter": {"design": "kaiser_sinc", "half", "cutoff", "beta", "taps"}.
    With "resample" that kind's clips leave at any other rate R: fvad_clips_export*_resampled at up/down = R/48000 in lowest terms
    with fvad_resample_design's default taps (K = 16 max(up, down), cutoff 0.45 / max(up, down), beta 6).  R is any rate but 48000
    whose ratio has up <= 640 and whose default design fits 20481 taps -- 44100, 32000, 22050 and 11025; 24000, 16000 and 8000
    too --, anything else raises before any work.  Output o of a clip sits o / R seconds after the clip's first sample: the phase
    starts at the clip, so "first_sample" is the segment's own start and "length" is ceil(len * up / down).  The manifest entries
    gain "filter": {"design": "kaiser_sinc_polyphase", "up", "down", "half", "cutoff", "beta", "taps"}.
    features "logmel": after the usual exports, one fvad_clips_export_mel over the denoised lanes' clips -- whatever rate and
    filter the denoised WAV files have -- with LOGMEL's parameters: the network's own 16 kHz samples (step 3, phase 2), 400-point
    periodic Hann, hop 160, fvad_mel_design(16000, 400, 80, 0, 8000), floor 1e-10.  Per clip NAME-####-denoised.logmel.npy
    (np.save, float32 [frames, 80]; frames = floor(L / 160) of the clip's L 16 kHz samples) and in its manifest entry "features":
    {file, frames, n_mels, n_fft, hop, sample_rate, first_sample, best_channel, max, floor, norm, mel: {design, fmin, fmax}}; a
    clip too short for one frame (under 201 samples at 16 kHz) has none and is counted in features_skipped.  features_norm
    "whisper": (max(x, max - 8) + 4) / 4 with the maximum taken per clip ("max" stays the un-normalised one).  An unknown
    features or features_norm, features_norm without features, and features with slice_chunks but without features_sliced (the
    split-source form of the feature export is opt-in) raise before any work.  With features None every file and manifest is
    what it was.
    features_sliced True (with features and slice_chunks; without either it raises before any work): the sliced run writes the
    features too -- per slice one fvad_clips_export_split_mel / _split_fbank over the due denoised clips' rows, the same .npy
    files, "features" entries and features_skipped as the unsliced run, byte for byte.
    features "fbank": Kaldi's filter-bank features in its place -- one fvad_clips_export_fbank with FBANK's parameters: the same
    samples (step 3, phase 2) times 32768, frames of 400 every 160 from the clip's first sample on (snip_edges), DC removed,
    pre-emphasis 0.97, the Povey window, a 512-point transform, fvad_mel_design_kaldi(16000, 512, 80, 20, 0), ln(max(.,
    FLT_EPSILON)).  Per clip NAME-####-denoised.fbank.npy (float32 [frames, 80], frames = 1 + (L - 400) // 160) and "features":
    every parameter above; a clip under 400 samples at 16 kHz has none and is counted in features_skipped.  features_norm "cmn":
    the clip's mean per band is subtracted (torchaudio's subtract_mean) and stated under "means".  "whisper" with "fbank" and
    "cmn" with "logmel" raise before any work."""
    _check_ingest(ingest)
    _check_features(features, features_norm, slice_chunks, features_sliced)
    rates, firs = _clip_rates(original_rate, denoised_rate, original_filter, denoised_filter)
    plan = load_plan(plan_path)
    if slice_chunks is not None:
        check_slice_chunks(slice_chunks, plan["fft_size"])
    own_ctx = ctx is None
    ctxs = [_make_ctx(plan, d, synth_seed) for d in (devices or [0])] if own_ctx else [ctx]
    try:
        os.makedirs(out_dir, exist_ok=True)
        loaded = _load_instances(plan, ingest, mapped=slice_chunks is not None)
        audio, refs = [a for a, _ in loaded], [r for _, r in loaded]
        parts = instance_shares(len(audio), len(ctxs))
        done, errs = [None] * len(ctxs), []
        notes = [{} for _ in ctxs]

        def work(d):
            try:
                insts_d, audio_d = [plan["instances"][i] for i in parts[d]], [audio[i] for i in parts[d]]
                if slice_chunks is None:
                    done[d] = _clips_share(ctxs[d], plan, insts_d, audio_d, out_dir, pcm16, rates, firs, features, features_norm)
                else:
                    done[d] = _clips_sliced_share(ctxs[d], plan, insts_d, audio_d, out_dir, pcm16, slice_chunks, notes[d], rates, firs, features, features_norm)
            except Exception as e:  # re-raised below, in the caller's thread
                errs.append(e)

        th = [threading.Thread(target=work, args=(d,)) for d in range(len(ctxs))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if errs:
            raise errs[0]
        per_inst = [None] * len(audio)
        for d, part in enumerate(parts):
            for i, x in zip(part, done[d]):
                per_inst[i] = x
        text, results = _evaluate(plan, [(segs, audit) for segs, audit, _ in per_inst], refs)
        for res, (_, _, manifest) in zip(results, per_inst):
            res["clips"] = manifest
            with open(os.path.join(out_dir, f"{manifest['name']}-clips.json"), "w") as f:
                json.dump(manifest, f, indent=1)
        if info is not None and slice_chunks is not None:
            info["held_peak_bytes"] = max([n.get("held_peak_bytes", 0) for n in notes] + [0])
            info["slices"] = sum(n.get("slices", 0) for n in notes)
        return text, results
    finally:
        if own_ctx:
            for c in ctxs:
                c.close()


class _HeldTails:
    """The audio of earlier slices that a sliced run_clips still needs, of one kind (original or denoised) for one channel-count
    group: every lane's samples [base, end) as f32 in a device buffer of L lanes `stride` apart, and a second buffer that the
    next carry writes (fvad_clips_export_split_device over this buffer and the slice, equal formats: the bits).  One base for
    the whole group -- the smallest any of its streams needs -- keeps the buffer a plain lane layout."""

    def __init__(self, ctx, n_lanes):
        self.ctx, self.L = ctx, n_lanes
        self.bufs = [[None, 0], [None, 0]]   # [device address, bytes]
        self.cur = 0
        self.base = self.end = 0
        self.stride = 0

    def a(self):
        """the held buffer as fvad_clips_export_split's A"""
        if self.end == self.base:
            return (None, 0, 0, 0)
        return (self.bufs[self.cur][0], self.L, self.stride, self.end - self.base)

    def bytes(self):
        return sum(b[1] for b in self.bufs)

    def carry(self, b, b_abs0, b_from, b_to, hold):
        """keep [hold, b_to) of every lane: [hold, b_from) from the held buffer, the rest from the slice's lanes b (A/B tuple;
        its sample 0 is absolute sample b_abs0, [b_from, b_to) of it valid).  hold None: nothing is needed any more."""
        if hold is None or hold >= b_to:
            self.base = self.end = b_to
            return
        hold = max(hold, self.base)
        n = b_to - hold
        n_a = max(min(b_from, self.end) - hold, 0)
        assert self.end == b_from or n_a == 0
        stride = (n + 3) // 4 * 4
        other = self.bufs[1 - self.cur]
        if other[1] < self.L * stride * 4:           # the plan's total says so: grow
            if other[0] is not None:
                self.ctx.device_free(other[0])
                other[0], other[1] = None, 0
            other[0], other[1] = self.ctx.device_alloc(self.L * stride * 4), self.L * stride * 4
        rows = [(1, l if n_a else 0, hold - self.base if n_a else 0, n_a, l, hold + n_a - b_abs0, n - n_a) for l in range(self.L)]
        res = self.ctx.clips_export_split(self.a(), b, False, rows, out_pcm16=False, d_out=other[0], out_capacity=self.L * stride)
        assert [int(o) for o in res["offsets"]] == [l * stride for l in range(self.L)]   # the lanes' new bases
        self.cur, self.base, self.end, self.stride = 1 - self.cur, hold, b_to, stride

    def close(self):
        for b in self.bufs:
            if b[0] is not None:
                self.ctx.device_free(b[0])
                b[0], b[1] = None, 0


def _clips_sliced_share(ctx, plan, insts, audio, out_dir, pcm16, slice_chunks, note, rates, firs, features=None, features_norm=None):
    """run_clips(slice_chunks=N) for the instances of one context -> [(segments, audit, manifest)] in the order given.
    Channel-count group after group, each in time slices [s0, s1) of N chunks read, denoised and band-summed as a sliced grid's
    (_slice_denoise_and_bands; audio mapped or raw), one single-config host batch per instance run on part by part (_HostParts).
    After each part, per kind (the reference's two recorders): the clips due -- the segments reported so far whose end the
    kind's audio has reached -- are exported in ONE fvad_clips_export_split over the held tail (A) and the slice's lanes (B:
    [s0, s1) of them is valid, the halo is not), the others stay pending or, once their stream has ended, are counted skipped;
    then the tail every pending or still possible clip needs (fvad_vad_batch_hold_from, the pending clips' starts) is carried
    into the other held buffer (_HeldTails).  The slices run one chunk past a group's last whole chunk where a file ends inside a
    chunk, so that the original audio's last samples are reached.  note: "held_peak_bytes", "slices".
    rates: a kind at 16000 exports with step 3, the skips from the clips' absolute sample_from (a clip's seam has no part in
    them); firs: a filtered kind exports with its step and taps, the filter running through the seam; the carry of the held
    tails stays a step-1 export.
    features: where a slice's due denoised clips are exported, their features are too -- one split feature call over the same
    rows (_features_split) --, so a clip gets its features when, and only if, its denoised clip is written."""
    if not audio:
        return []
    chunk, H, N, F = 24000, SLICE_HALO_CHUNKS, slice_chunks, plan["fft_size"]
    dims = [_dims(a, mapped=True) for a in audio]
    n_frames, n_chunks = [d[1] for d in dims], [d[1] // chunk for d in dims]
    groups = {}
    for i, d in enumerate(dims):
        groups.setdefault(d[0], []).append(i)
    job = _SweepJob([plan["vad_machine_config"]], [None], [F], False, F, N, "host", "host", 1, False)
    opts = _engine_opts(job.configs[0], F)
    n_max, fr_slice = N + H, N * chunk // F
    lanes_max = max(len(m) * nch for nch, m in groups.items())
    own = {"pcm": lanes_max * n_max * chunk * 4, "den": lanes_max * n_max * chunk * 4, "band0": lanes_max * (n_max * chunk // F + 1) * 4,
           "rms": lanes_max * n_max * 4, "bands": lanes_max * fr_slice * 4}
    d, host = {}, None
    times = collections.defaultdict(float)
    segs_of, audits = [[] for _ in audio], [None] * len(audio)
    entries = [{} for _ in audio]                   # [instance]{(segment, kind): manifest entry}
    skipped = [{"original": 0, "denoised": 0} for _ in audio]
    feats, feats_skipped = [{} for _ in audio], [0] * len(audio)   # [instance]{segment: the "features" entry}
    note.update(held_peak_bytes=0, slices=0)
    try:
        for k, nb in own.items():
            d[k] = ctx.device_alloc(max(nb, 16))
        if not _is_raw(audio):
            host = ctx.host_alloc(lanes_max * n_max * chunk)
        buf = _SliceBufs(d, host, opts, fr_slice)
        for nch, members in groups.items():
            L = len(members) * nch
            m = _HostParts(ctx, job, nch, [None] * len(members))
            tails = {"original": _HeldTails(ctx, L), "denoised": _HeldTails(ctx, L)}
            pending = {kind: [[] for _ in members] for kind in tails}     # [member][(segment, from, to)]
            seen = [0] * len(members)
            try:
                K = max(-(-n_frames[i] // chunk) for i in members)
                for s0 in range(0, K, N):
                    s1 = min(s0 + N, K)
                    start = max(s0 - H, 0)
                    n = s1 - start
                    note["slices"] += 1
                    rms = _slice_denoise_and_bands(ctx, audio, members, nch, s0, s1, buf, m.blocks, times)
                    nc = [max(0, min(n_chunks[i], s1) - s0) for i in members]
                    nf = [[max(0, min(n_chunks[i] * chunk // F, s1 * chunk // F) - s0 * chunk // F) for i in members]]
                    if max(nf[0]) > 0 or s0 == 0:
                        m.part(d["bands"], fr_slice, nf, rms, nc, s0 * chunk)
                    holds = []
                    for k, i in enumerate(members):
                        segs = m.hosts[k].segments(0)[0]
                        for kind in tails:
                            pending[kind][k] += [(j, int(sg[0]), int(sg[1])) for j, sg in enumerate(segs[seen[k]:], seen[k])]
                        seen[k], segs_of[i] = len(segs), segs
                        holds.append(None if s1 >= n_chunks[i] else m.hosts[k].hold_from(0)[0])   # (an ended machine reports nothing more)
                    for kind, d_b in (("original", d["pcm"]), ("denoised", d["den"])):
                        t = tails[kind]
                        b = (d_b, L, n * chunk, n * chunk)
                        rows, owner, need = [], [], []
                        for k, i in enumerate(members):
                            reach = min(n_frames[i], s1 * chunk) if kind == "original" else min(n_chunks[i], s1) * chunk
                            ended = s1 * chunk >= n_frames[i] if kind == "original" else s1 >= n_chunks[i]
                            still = []
                            for j, a0, a1 in pending[kind][k]:
                                if a1 > reach:
                                    if ended:   # Recorder.finalize never runs for a recording whose end the stream does not reach
                                        skipped[i][kind] += 1
                                    else:
                                        still.append((j, a0, a1))
                                    continue
                                cut = min(max(a0, s0 * chunk), a1)                      # the seam: [a0, cut) is held, [cut, a1) in the slice
                                n_a, n_b = cut - a0, a1 - cut
                                assert n_a == 0 or t.base <= a0 < t.end == s0 * chunk, "a due clip starts in front of the held tail"
                                rows.append((nch, k * nch if n_a else 0, a0 - t.base if n_a else 0, n_a,
                                             k * nch if n_b else 0, cut - start * chunk if n_b else 0, n_b))
                                owner.append((i, j, a0))
                            pending[kind][k] = still
                            need += [a0 for _, a0, _ in still] + ([] if holds[k] is None else [holds[k]])
                        if rows:
                            kw, skips, has_lens = _clip_export_args(kind, rates[kind], [a0 for _, _, a0 in owner], firs[kind])
                            res = ctx.clips_export_split(t.a(), b, False, rows, out_pcm16=pcm16, **kw)
                            lens = res["out_lens"] if has_lens else [r[3] + r[6] for r in rows]
                            for q, ((i, j, a0), o) in enumerate(zip(owner, res["offsets"])):
                                o, n_clip = int(o), int(lens[q])
                                path = os.path.join(out_dir, "{}-{:04d}-{}.wav".format(insts[i]["name"], j, kind))
                                _write_clip(path, res["out"][o:o + n_clip], pcm16, rates[kind])
                                entries[i][(j, kind)] = _clip_entry(path, res["best_channel"][q], res["best_rms"][q], res["runner_up_rms"][q],
                                                                    rates[kind], a0 + (0 if skips is None else int(skips[q])), n_clip, firs[kind])
                            if features is not None and kind == "denoised":
                                _features_split(ctx, t.a(), b, rows, owner, insts, out_dir, feats, feats_skipped, features, features_norm)
                        t.carry(b, start * chunk, s0 * chunk, s1 * chunk, min(need) if need else None)
                    note["held_peak_bytes"] = max(note["held_peak_bytes"], sum(t.bytes() for t in tails.values()))
                for k, i in enumerate(members):
                    audits[i] = m.hosts[k].audit(0, 0)
            finally:
                for t in tails.values():
                    t.close()
                m.close()
    finally:
        for a in d.values():
            ctx.device_free(a)
        if host is not None:
            ctx.host_free(host)
    out = []
    for i, inst in enumerate(insts):
        manifest = {"name": inst["name"], "sample_rate": 48000, "pcm16": bool(pcm16), "clips": []}
        for j, sg in enumerate(segs_of[i]):
            c = {"segment": j, "start": int(sg[0]), "length": int(sg[1] - sg[0])}
            for kind in ("original", "denoised"):
                if (j, kind) in entries[i]:
                    c[kind] = entries[i][(j, kind)]
            if j in feats[i]:
                c["features"] = feats[i][j]
            manifest["clips"].append(c)
        manifest["original_skipped"], manifest["denoised_skipped"] = skipped[i]["original"], skipped[i]["denoised"]
        if features is not None:
            manifest["features_skipped"] = feats_skipped[i]
        out.append((segs_of[i], audits[i], manifest))
    return out


# ---------------------------------------------------------------- the denoised recordings themselves (fvad_egress)
DENOISED_FORMATS = {"pcm16": fv.INGEST_PCM16, "pcm24": fv.INGEST_PCM24, "f32": fv.INGEST_F32}


def _check_denoised_format(fmt):
    if fmt not in DENOISED_FORMATS:
        raise ValueError(f"denoised format: {fmt!r} (one of {', '.join(DENOISED_FORMATS)})")


def _denoised_resample(rate):
    """the filter of recordings written at `rate` (run_denoise(rate=...)): up/down = rate/48000 in lowest terms and
    fvad_resample_design's default taps, its parameters spelt out for the manifest; ValueError for a rate that has none"""
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or rate <= 0 or rate >= 1 << 32:
        raise ValueError(f"run_denoise: rate {rate!r} (None, 'source' or a sample rate)")
    try:
        up, down = fv.resample_ratio(48000, int(rate))
        taps = fv.resample_design(up, down)
    except fv.FvadError:
        raise ValueError(f"run_denoise: rate {rate!r}: no ratio to 48000 with up <= {fv.RESAMPLE_UP_MAX} whose default design fits "
                         f"{fv.RESAMPLE_TAPS_MAX} taps") from None
    m = max(up, down)
    return {"rate": int(rate), "up": up, "down": down, "half": 16, "cutoff": 0.45 / m, "beta": 6.0, "taps": taps}


def _check_denoised_rate(rate):
    if rate is None or (isinstance(rate, str) and rate == "source") or (not isinstance(rate, bool) and rate == 48000):
        return
    _denoised_resample(rate)


DENOISED_SOURCES = ("lanes", "network")
# The network's own samples in the 48 kHz lanes.  NSNet2 works at 16 kHz and K3 brings its output back to 48 kHz by x3 linear
# interpolation: network sample j lands unchanged at lane index 3 j + 2, the two samples in front of it are lerps.  So the stream
# lane[NETWORK_PHASE + NETWORK_STEP * j] is the network's output bit for bit, and source="network" reads nothing else.  (The
# delay D = fvad_nsnet2_delay(48000) of _denoise_share counts lane samples of the same clock.)
NETWORK_STEP, NETWORK_PHASE = 3, 2
NETWORK_RATE = 48000 // NETWORK_STEP


def _check_denoised_source(source, kinds):
    """run_denoise's source; ValueError for an unknown one and for "network" with a kind that reads the original"""
    if source not in DENOISED_SOURCES:
        raise ValueError(f"run_denoise: source {source!r} (one of {', '.join(DENOISED_SOURCES)})")
    if source == "network" and kinds is not None and any(k != "denoised" for k in kinds):
        raise ValueError(f"run_denoise: source 'network' with kinds {tuple(kinds)!r}: the kinds that read the original are written from the lanes")


def _network_resample(rate):
    """the filter of recordings written at `rate` from the network's 16 kHz stream (run_denoise(source="network")): up/down =
    rate/16000 in lowest terms.  At 16000 the single tap 1.0: the file holds the network's samples themselves.  Otherwise
    fvad_resample_design's default taps; when 3 divides up the file is put on the 48 kHz lanes' clock: stream sample j sits at
    lane time 3 j + 2, so output o belongs at fine index o down - L, L = 2 up / 3, and the lag goes into the taps -- L zeros on
    each side of the centre's move, taps' = [0] * 2 L + taps (centre K + L; they need not be symmetric): "lead" 0.  When 3 does
    not divide up (16000, 32000, 8000) no lag is applied -- a shift of 2/3 of a stream sample would cost the exactness that is
    the point at 16000 -- and the file's clock is "lead" = 2 samples of 48 kHz ahead.  ValueError for a rate that has no ratio
    with up <= 640 or whose lagged design passes FVAD_RESAMPLE_TAPS_MAX taps."""
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or rate <= 0 or rate >= 1 << 32:
        raise ValueError(f"run_denoise: rate {rate!r} (None, 'source' or a sample rate)")
    own = {"rate": int(rate), "source": "network", "step": NETWORK_STEP, "phase": NETWORK_PHASE}
    if int(rate) == NETWORK_RATE:
        return dict(own, up=1, down=1, taps=np.array([1.0], np.float32), lag=0, lead=NETWORK_PHASE, half=None)
    try:
        up, down = fv.resample_ratio(NETWORK_RATE, int(rate))
        taps = fv.resample_design(up, down)
    except fv.FvadError:
        raise ValueError(f"run_denoise: rate {rate!r}: no ratio to {NETWORK_RATE} with up <= {fv.RESAMPLE_UP_MAX} whose default design fits "
                         f"{fv.RESAMPLE_TAPS_MAX} taps") from None
    lag = NETWORK_PHASE * up // NETWORK_STEP if up % NETWORK_STEP == 0 else 0
    if taps.size + 2 * lag > fv.RESAMPLE_TAPS_MAX:
        raise ValueError(f"run_denoise: rate {rate!r}: the default design lagged by {lag} has {taps.size + 2 * lag} taps, more than "
                         f"{fv.RESAMPLE_TAPS_MAX}")
    taps = np.concatenate([np.zeros(2 * lag, np.float32), taps])
    return dict(own, up=up, down=down, half=16, cutoff=0.45 / max(up, down), beta=6.0, taps=taps, lag=lag,
                lead=0 if up % NETWORK_STEP == 0 else NETWORK_PHASE)


def _denoised_filters(rate, audio, dims, fmt, source="lanes"):
    """per instance the _denoised_resample filter its recording leaves through, None for one that leaves at 48 kHz (fvad_egress).
    With source "network" every instance has a filter, _network_resample's (rate None: 48000), over the network's stream.
    rate: an integer for every file, or "source" -- each instance at its own file's rate, which ingest="device" knows
    (_RawAudio.rate) and the host path, which takes 48 kHz files only, does not need.  ValueError, before any file exists, for a
    recording whose frames fit no tile of the kernel or whose data would pass 4 GB."""
    code, made, out = DENOISED_FORMATS[fmt], {}, []
    for a, (nch, n_frames) in zip(audio, dims):
        r = (a.rate if isinstance(a, _RawAudio) else 48000) if isinstance(rate, str) else 48000 if rate is None else int(rate)
        if r == 48000 and source == "lanes":
            out.append(None)
            continue
        if r not in made:
            made[r] = _network_resample(r) if source == "network" else _denoised_resample(r)
        f = made[r]
        if fv.egress_resample_tile(f["up"], f["down"], f["taps"].size, nch, code) == 0:
            raise ValueError(f"run_denoise: rate {r}: the filter's window fits no tile of the kernel for {nch} channels")
        frames = fv.resample_out_frames(n_frames // 24000 * (24000 // f.get("step", 1)), f["up"], f["down"])
        if frames * nch * fv.INGEST_SAMPLE_BYTES[code] > 0xFFFFFF00:
            raise ValueError(f"run_denoise: rate {r}: more than 4 GB of data in one file")
        out.append(f)
    return out


def _by_filter(pairs):
    """[(filter, x)] -> [(filter, [x])], one entry per distinct ratio (one ratio and one set of taps per fvad_egress_resample call)"""
    groups = {}
    for f, x in pairs:
        groups.setdefault(f["rate"], (f, []))[1].append(x)
    return list(groups.values())


DENOISED_KINDS = ("denoised", "original", "residual", "mix")


def _check_denoised_kinds(kinds, mix, rate):
    """run_denoise's kinds / mix -> None (today's single denoised file) or the kinds as a tuple; ValueError for an unknown or
    repeated kind, no kind at all, a mix outside (0, 1), a mix without the kind "mix" or the kind without a mix, and for
    another rate than the lanes' together with a kind that reads the original (the resampling egress has one source)"""
    if kinds is None:
        if mix is not None:
            raise ValueError("run_denoise: mix comes with the kind 'mix' (kinds=(..., 'mix'))")
        return None
    if isinstance(kinds, str) or not isinstance(kinds, (list, tuple)) or not kinds:
        raise ValueError(f"run_denoise: kinds {kinds!r} (a sequence of {', '.join(DENOISED_KINDS)})")
    for k in kinds:
        if k not in DENOISED_KINDS:
            raise ValueError(f"run_denoise: kind {k!r} (one of {', '.join(DENOISED_KINDS)})")
    if len(set(kinds)) != len(kinds):
        raise ValueError(f"run_denoise: kinds {kinds!r} name a kind twice")
    if "mix" in kinds:
        if isinstance(mix, bool) or not isinstance(mix, (int, float, np.integer, np.floating)) or not 0.0 < float(mix) < 1.0:
            raise ValueError(f"run_denoise: the kind 'mix' needs mix=W with 0 < W < 1 (mix: {mix!r})")
    elif mix is not None:
        raise ValueError("run_denoise: mix comes with the kind 'mix' (kinds=(..., 'mix'))")
    if any(k != "denoised" for k in kinds) and not (rate is None or (not isinstance(rate, (bool, str)) and rate == 48000)):
        raise ValueError(f"run_denoise: rate {rate!r} with kinds {tuple(kinds)!r}: the kinds that read the original are written at 48000 only")
    return tuple(kinds)


def _kind_weights(kind, mix):
    """(w_orig, w_den) of a kind of fvad_egress_mix, float32: the aligned original, what the denoiser removed, or W of the
    denoised and the rest (1 - W, in float32) of the aligned original"""
    if kind == "original":
        return np.float32(1.0), np.float32(0.0)
    if kind == "residual":
        return np.float32(1.0), np.float32(-1.0)
    return np.float32(1.0) - np.float32(mix), np.float32(mix)


def _kind_entry(f, kind, mix, delay):
    """a kind's entry of an instance's manifest: the file's own manifest without the name, the kind, its weights (None for the
    denoised file, which fvad_egress writes) and the delay of its frames behind the input file's"""
    w = (None, None) if kind == "denoised" else tuple(float(x) for x in _kind_weights(kind, mix))
    e = {k: v for k, v in f.manifest.items() if k != "name"}
    e.update(kind=kind, w_orig=w[0], w_den=w[1], delay=delay)
    return e


def _kind_manifests(insts, kinds, files, mix, delay):
    """[instance] {"name", "kinds": [entry per kind, in the order asked for]} from files {kind: [instance's _DenoisedFile]}"""
    return [{"name": inst["name"], "kinds": [_kind_entry(files[k][i], k, mix, delay) for k in kinds]} for i, inst in enumerate(insts)]


class _DenoisedFile:
    """NAME-denoised.wav of one instance (NAME-<kind>.wav for another kind of run_denoise), created at its final size -- fvad_wav_header's 44 bytes, then a hole of n_frames
    frames -- and mapped for fvad_egress to fill (`map`: the whole file as bytes, None for a file without frames).  With a
    filter `rs` (_denoised_resample) the file holds the ceil(n_frames up / down) frames of the stream of n_frames lane samples
    at the filter's rate, for fvad_egress_resample to fill.  A filter over the network's stream (_network_resample: it has a
    "step") counts the stream's samples, n_frames / step of them, and is filled by fvad_egress_resample_strided."""

    def __init__(self, out_dir, inst, fmt, n_channels, n_frames, rs=None, kind="denoised"):
        code = DENOISED_FORMATS[fmt]
        self.frame_bytes = n_channels * fv.INGEST_SAMPLE_BYTES[code]
        if rs is not None:
            n_frames //= rs.get("step", 1)
        self.rs, self.stream_frames, self.written, rate = rs, n_frames, 0, 48000
        if rs is not None:
            n_frames, rate = fv.resample_out_frames(n_frames, rs["up"], rs["down"]), rs["rate"]
        self.manifest = {"name": inst["name"], "file": os.path.join(out_dir, f"{inst['name']}-{kind}.wav"), "format": fmt,
                         "channels": n_channels, "frames": n_frames, "sample_rate": rate}
        if rs is not None and "source" in rs:
            self.manifest.update(source=rs["source"], lead=rs["lead"])
            if rs["half"] is not None:   # (the single tap at the network's own rate is no resampling)
                self.manifest["resample"] = {k: rs[k] for k in ("up", "down", "half", "cutoff", "beta", "lag")}
        elif rs is not None:
            self.manifest["resample"] = {k: rs[k] for k in ("up", "down", "half", "cutoff", "beta")}
        head = fv.wav_header(code, n_channels, rate, n_frames)   # (raises for more than 4 GB of data, like fvad_wav_write)
        size = len(head) + n_frames * self.frame_bytes
        with open(self.manifest["file"], "wb") as f:
            f.write(head)
            f.truncate(size)
        self.map = np.memmap(self.manifest["file"], dtype=np.uint8, mode="r+", shape=(size,)) if n_frames else None

    def sink(self, frame_from, n_frames, first_lane, src_offset):
        """the fvad_egress sink row of the file's frames [frame_from, frame_from + n_frames)"""
        n_channels, code = self.manifest["channels"], DENOISED_FORMATS[self.manifest["format"]]
        return (fv.WAV_HEADER_BYTES + frame_from * self.frame_bytes, n_frames, n_channels, code, first_lane, src_offset)

    def sink_mix(self, frame_from, n_frames, first_lane, src_offset, orig_offset, orig_zeros):
        """the fvad_egress_mix row of the file's frames [frame_from, frame_from + n_frames): sink()'s, then where the original
        lanes' partner of the first frame behind the orig_zeros leading zeros lies"""
        return self.sink(frame_from, n_frames, first_lane, src_offset) + (orig_offset, orig_zeros)

    def sink_resampled(self, out_to, first_lane, src_offset, frame_base, n_frames):
        """the fvad_egress_resample row of the file's outputs [written, out_to), which then count as written; the lanes hold the
        stream's samples [frame_base, frame_base + n_frames) from src_offset on (the network's stream: `step` apart)"""
        n_channels, code = self.manifest["channels"], DENOISED_FORMATS[self.manifest["format"]]
        out_from, self.written = self.written, max(out_to, self.written)
        return (fv.WAV_HEADER_BYTES + out_from * self.frame_bytes, self.written - out_from, n_channels, code, first_lane, src_offset,
                frame_base, n_frames, self.stream_frames, out_from)

    def ready(self, frames_have):
        """fvad_egress_resample_ready: the file's leading outputs that the stream's samples below frames_have can finish"""
        return fv.egress_resample_ready(self.rs["up"], self.rs["down"], self.rs["taps"].size, self.stream_frames, frames_have)

    def close(self):
        self.map = None   # unmapped without msync: the written pages are the page cache's, as after fvad_wav_write's fwrite + fclose


def _egress_resampled(ctx, rs, rows, out, lanes):
    """one filter's rows: fvad_egress_resample over the lanes, or fvad_egress_resample_strided over the network's stream in them"""
    if "step" in rs:
        ctx.egress_resample_strided(rows, rs["up"], rs["down"], rs["taps"], rs["step"], out=out, **lanes)
    else:
        ctx.egress_resample(rows, rs["up"], rs["down"], rs["taps"], out=out, **lanes)


def _denoise_share(ctx, plan, insts, audio, out_dir, fmt, filters=None, kinds=None, mix=None):
    """run_denoise for the instances of one context, resident: _denoise_resident's lanes, one fvad_egress over every file --
    with `filters` (_denoised_filters) over the files that leave at 48 kHz, and one fvad_egress_resample per other ratio.
    With `kinds`: the denoised files as before if they are asked for, and per other kind one fvad_egress_mix over the original
    and the denoised lanes, which both lie on the device: frame n of a file pairs denoised sample n with original sample n - D,
    D = fvad_nsnet2_delay(48000), zeros in front."""
    if not audio:
        return []
    held = []

    def dalloc(nbytes):
        held.append(ctx.device_alloc(max(int(nbytes), 4)))
        return held[-1]

    files, mixed = [], {}
    try:
        r = _denoise_resident(ctx, audio, plan["fft_size"], plan["vad_machine_config"], dalloc)
        lane0, l = {}, 0
        for i in r.order:
            lane0[i] = l
            l += _dims(audio[i])[0]
        if kinds is None or "denoised" in kinds:
            files = [_DenoisedFile(out_dir, inst, fmt, _dims(a)[0], n * 24000, rs)
                     for inst, a, n, rs in zip(insts, audio, r.n_chunks, filters or [None] * len(insts))]
        lanes = dict(d_lanes=r.d_den, n_lanes=r.n_lanes, lane_stride=r.n_den, n_samples=r.n_den)
        plain = [i for i, f in enumerate(files) if f.rs is None]
        if plain:
            ctx.egress([files[i].sink(0, files[i].manifest["frames"], lane0[i], 0) for i in plain], out=[files[i].map for i in plain], **lanes)
        for rs, idx in _by_filter([(f.rs, i) for i, f in enumerate(files) if f.rs is not None]):
            rows = [files[i].sink_resampled(files[i].manifest["frames"], lane0[i], rs.get("phase", 0), 0, files[i].stream_frames) for i in idx]
            _egress_resampled(ctx, rs, rows, [files[i].map for i in idx], lanes)
        if kinds is None:
            return [f.manifest for f in files]
        D = fv.nsnet2_delay(48000)
        both = dict(d_orig=r.d_pcm, orig_stride=r.stride, orig_samples=r.n_samples, d_den=r.d_den, den_stride=r.n_den, den_samples=r.n_den,
                    n_lanes=r.n_lanes)
        for kind in kinds:
            if kind == "denoised":
                continue
            mixed[kind] = [_DenoisedFile(out_dir, inst, fmt, _dims(a)[0], n * 24000, kind=kind) for inst, a, n in zip(insts, audio, r.n_chunks)]
            rows = [f.sink_mix(0, f.manifest["frames"], lane0[i], 0, 0, min(D, f.manifest["frames"])) for i, f in enumerate(mixed[kind])]
            w_orig, w_den = _kind_weights(kind, mix)
            ctx.egress_mix(rows, w_orig, w_den, out=[f.map for f in mixed[kind]], **both)
        return _kind_manifests(insts, kinds, dict(mixed, denoised=files), mix, D)
    finally:
        for f in files + [f for fs in mixed.values() for f in fs]:
            f.close()
        for d in held:
            ctx.device_free(d)


def _denoise_sliced_share(ctx, plan, insts, audio, out_dir, fmt, slice_chunks, filters=None, kinds=None, mix=None):
    """run_denoise(slice_chunks=N) for the instances of one context: channel-count group after group in time slices [s0, s1) of
    N chunks, read and denoised as a sliced grid's (_slice_denoise_and_bands, without bands; audio mapped or raw); each slice's
    frames go to their place in the files -- byte 44 + s0 * 24000 * frame bytes -- in one fvad_egress over the group's members
    that still have chunks there.  The device holds one slice and its halo.
    A member that leaves at another rate (`filters`) cannot finish, in a slice, the outputs whose filter window reaches into the
    next one: it writes the outputs [written, fvad_egress_resample_ready(frames up to the slice's end)) and leaves the others to
    the next slice, which reads their window's older part from its halo -- the slice buffer from chunk max(s0 - H, 0) on is what
    the row is given.  The halo's chunks from the third on are the resident run's (SLICE_HALO_CHUNKS' comment), and the filter
    reaches no further back than that.  A member's last slice has the stream's last sample and writes everything that is left."""
    if not audio:
        return []
    chunk, H, N, F = 24000, SLICE_HALO_CHUNKS, slice_chunks, plan["fft_size"]
    for rs in filters or ():
        # the outputs a slice defers read at most (2 K + down) / up + 1 samples below the slice's first: inside the halo's exact part
        # (a filter over the network's stream reaches `step` lane samples per stream sample)
        assert rs is None or rs.get("step", 1) * ((rs["taps"].size - 1 + rs["down"]) // rs["up"] + 1) <= (H - 2) * chunk, "the halo covers the filter's reach"
    dims = [_dims(a, mapped=True) for a in audio]
    n_chunks = [d[1] // chunk for d in dims]
    groups = {}
    for i, d in enumerate(dims):
        groups.setdefault(d[0], []).append(i)
    opts = _engine_opts(plan["vad_machine_config"], F)
    n_max = N + H
    lanes_max = max(len(m) * nch for nch, m in groups.items())
    own = {"pcm": lanes_max * n_max * chunk * 4, "den": lanes_max * n_max * chunk * 4, "band0": lanes_max * (n_max * chunk // F + 1) * 4,
           "rms": lanes_max * n_max * 4, "bands": 16}
    d, host, files, mixed = {}, None, [], {}
    D = fv.nsnet2_delay(48000) if kinds else 0
    times = collections.defaultdict(float)
    try:
        for k, nb in own.items():
            d[k] = ctx.device_alloc(max(nb, 16))
        if not _is_raw(audio):
            host = ctx.host_alloc(lanes_max * n_max * chunk)
        buf = _SliceBufs(d, host, opts, N * chunk // F)
        if kinds is None or "denoised" in kinds:
            files = [_DenoisedFile(out_dir, inst, fmt, dm[0], n * chunk, rs) for inst, dm, n, rs in zip(insts, dims, n_chunks, filters or [None] * len(insts))]
        for kind in kinds or ():
            if kind != "denoised":
                mixed[kind] = [_DenoisedFile(out_dir, inst, fmt, dm[0], n * chunk, kind=kind) for inst, dm, n in zip(insts, dims, n_chunks)]
        for nch, members in groups.items():
            L = len(members) * nch
            K = max(n_chunks[i] for i in members)
            for s0 in range(0, K, N):
                s1 = min(s0 + N, K)
                start = max(s0 - H, 0)
                n = s1 - start
                _slice_denoise_and_bands(ctx, audio, members, nch, s0, s1, buf, (), times)
                live = [(k, i) for k, i in enumerate(members) if n_chunks[i] > s0]
                lanes = dict(d_lanes=d["den"], n_lanes=L, lane_stride=n * chunk, n_samples=n * chunk)
                plain = [(k, i) for k, i in live if files and files[i].rs is None]
                if plain:
                    sinks = [files[i].sink(s0 * chunk, (min(n_chunks[i], s1) - s0) * chunk, k * nch, (s0 - start) * chunk) for k, i in plain]
                    ctx.egress(sinks, out=[files[i].map for _, i in plain], **lanes)
                for rs, ki in _by_filter([(files[i].rs, (k, i)) for k, i in live if files and files[i].rs is not None]):
                    # in stream samples: a chunk is `sc` of them (the network's stream: a slice begins at a multiple of 24000 lane
                    # samples, so the phase holds in every slice buffer)
                    sc = chunk // rs.get("step", 1)
                    rows = [files[i].sink_resampled(files[i].ready(min(s1, n_chunks[i]) * sc), k * nch, rs.get("phase", 0), start * sc,
                                                    (min(n_chunks[i], s1) - start) * sc) for k, i in ki]
                    _egress_resampled(ctx, rs, rows, [files[i].map for _, i in ki], lanes)
                # the other kinds: the slice's frames of the denoised buffer and their partners D samples earlier in the original
                # buffer, which starts at the same chunk -- in the halo for every slice but the first, whose first D frames are zeros
                if not mixed:
                    continue
                assert s0 == 0 or (s0 - start) * chunk >= D, "the halo covers the delay"
                both = dict(d_orig=d["pcm"], orig_stride=n * chunk, orig_samples=n * chunk, d_den=d["den"], den_stride=n * chunk,
                            den_samples=n * chunk, n_lanes=L)
                for kind, fs in mixed.items():
                    rows = []
                    for k, i in live:
                        frames = (min(n_chunks[i], s1) - s0) * chunk
                        at = ((s0 - start) * chunk, 0, min(D, frames)) if s0 == 0 else ((s0 - start) * chunk, (s0 - start) * chunk - D, 0)
                        rows.append(fs[i].sink_mix(s0 * chunk, frames, k * nch, *at))
                    w_orig, w_den = _kind_weights(kind, mix)
                    ctx.egress_mix(rows, w_orig, w_den, out=[fs[i].map for _, i in live], **both)
        if kinds is None:
            return [f.manifest for f in files]
        return _kind_manifests(insts, kinds, dict(mixed, denoised=files), mix, D)
    finally:
        for f in files + [f for fs in mixed.values() for f in fs]:
            f.close()
        for a in d.values():
            ctx.device_free(a)
        if host is not None:
            ctx.host_free(host)


def run_denoise(plan_path, out_dir, fmt="pcm16", ctx=None, synth_seed=None, devices=None, ingest="host", slice_chunks=None, rate=None,
                kinds=None, mix=None, source="lanes"):
    """The plan's recordings, denoised, as WAV files: per instance NAME-denoised.wav in out_dir with all of the instance's
    channels at 48 kHz, as PCM16 (fmt "pcm16": rint(clamp(y * 32768)), the rule of the PCM16 clips and of
    fvad_lane.denoised_i16, not fvad_wav_write's), 24-bit PCM ("pcm24") or float32 ("f32": the lanes' bits, the file
    fvad_wav_write writes).  A file has as many frames as the denoised lanes hold -- whole chunks of 24000, as run_clips
    documents: a partial last chunk is not denoised.  Each file is created at its final size with fvad_wav_header, mapped, and
    filled by fvad_egress: the GPU converts and interleaves, the host moves bytes.  Instances are dealt to `devices` like
    run_clips; the denoising is _denoise_resident's (the context option "reproducible" makes it agree bit for bit with every
    other path), or with slice_chunks N the sliced grid's, device memory bounded by a slice -- the same bytes.  ingest "device":
    the files' bytes are decoded on the GPU (run_grid); the same bytes again.  A bad fmt, ingest or slice_chunks raises before
    any work.  Returns a manifest per instance, in plan order: name, file, format, channels, frames, sample_rate.
    rate: None or 48000 write the lanes' own 48 kHz.  An integer R writes every file at R, and "source" each instance at its own
    file's rate (what ingest="device" resampled it from; 48000 otherwise): fvad_egress_resample with fvad_resample_design's
    default taps for up/down = R/48000, one call per distinct ratio, beside fvad_egress for the instances at 48000.  Such a file
    holds ceil(frames up / down) frames, output o at o / R seconds of the recording; its manifest says the resampled frames and
    sample_rate and gains "resample": {up, down, half, cutoff, beta}.  Sliced, device-ingested and resident runs write the same
    bytes on a "reproducible" context.  A rate without a ratio (up <= 640), a default design that does not fit, frames that
    fit no tile or more than 4 GB of data raise ValueError before any work.
    kinds: None is the above and returns what it always returned.  Otherwise a sequence of "denoised", "original", "residual",
    "mix": per instance and kind NAME-<kind>.wav in fmt, every one with the denoised file's frames, channels and rate.  The
    denoised samples lag the input's by D = fvad_nsnet2_delay(48000) = 482 samples (include/fvad.h has the derivation), and the
    input file is 10 ms early, maybe at another rate or format and a partial chunk longer: no partner for an A/B comparison.
    "original" is the input delayed by D -- frame n is x[n - D], zeros for n < D --, "residual" what the denoiser took out,
    x[n - D] - y[n], and "mix" (with mix=W, 0 < W < 1) W of the denoised and f32(1) - f32(W) of the delayed original.  They are
    written by fvad_egress_mix from the original and the denoised lanes where both lie on the device already, one call per
    kind, no lane memory of their own; the "denoised" kind is today's file, through fvad_egress.  With kinds the manifest of an
    instance is {"name", "kinds": [one entry per kind: file, kind, w_orig, w_den (None for "denoised"), delay, frames, format,
    channels, sample_rate]}.  An unknown kind, a mix out of range or without its kind, or a rate other than 48000 together with
    a kind other than "denoised" raise ValueError before any work.
    source: "lanes" is all of the above.  The 48 kHz lanes are the x3 LINEAR interpolation of NSNet2's 16 kHz output (a network
    tone at 6 kHz stands in them at -3.8 dB with an image at 10 kHz at -11.8 dB); "network" writes the denoised file
    from the network's own samples instead, lane[3 j + 2], with fvad_egress_resample_strided: at rate 16000 the samples
    themselves (a third of the bytes, nothing lost), at None / 48000 the default 3/1 design in place of the lerp, at another
    rate R one filter for R/16000 (_network_resample).  A file holds ceil(n * 8000 * up / down) frames for n chunks, the count
    source="lanes" gives at R.  Its manifest gains "source": "network", "lead" -- 0 when 3 divides up: the file is on the lanes'
    clock; otherwise 2: its clock is two 48 kHz samples (41.7 us) ahead -- and, except at 16000, "resample" with a "lag".
    "network" with a kind other than "denoised", an unknown source, a rate without a ratio to 16000 (up <= 640) or whose
    lagged design passes the tap limit (11025) raise ValueError before any work."""
    _check_ingest(ingest)
    _check_denoised_format(fmt)
    if source == "network" and not (rate is None or (isinstance(rate, str) and rate == "source")):
        _network_resample(rate)
    else:
        _check_denoised_rate(rate)
    kinds = _check_denoised_kinds(kinds, mix, None if source == "network" else rate)
    _check_denoised_source(source, kinds)
    plan = load_plan(plan_path)
    if slice_chunks is not None:
        check_slice_chunks(slice_chunks, plan["fft_size"])
    own_ctx = ctx is None
    ctxs = [_make_ctx(plan, d, synth_seed) for d in (devices or [0])] if own_ctx else [ctx]
    try:
        audio = [a for a, _ in _load_instances(plan, ingest, mapped=slice_chunks is not None)]
        filters = None
        if source == "network" or (rate is not None and (isinstance(rate, str) or rate != 48000)):
            filters = _denoised_filters(rate, audio, [_dims(a, mapped=slice_chunks is not None) for a in audio], fmt, source)
        os.makedirs(out_dir, exist_ok=True)
        parts = instance_shares(len(audio), len(ctxs))
        done, errs = [None] * len(ctxs), []

        def work(d):
            try:
                insts_d, audio_d = [plan["instances"][i] for i in parts[d]], [audio[i] for i in parts[d]]
                filters_d = None if filters is None else [filters[i] for i in parts[d]]
                if slice_chunks is None:
                    done[d] = _denoise_share(ctxs[d], plan, insts_d, audio_d, out_dir, fmt, filters_d, kinds, mix)
                else:
                    done[d] = _denoise_sliced_share(ctxs[d], plan, insts_d, audio_d, out_dir, fmt, slice_chunks, filters_d, kinds, mix)
            except Exception as e:  # re-raised below, in the caller's thread
                errs.append(e)

        th = [threading.Thread(target=work, args=(d,)) for d in range(len(ctxs))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if errs:
            raise errs[0]
        manifests = [None] * len(audio)
        for d, part in enumerate(parts):
            for i, m in zip(part, done[d]):
                manifests[i] = m
        return manifests
    finally:
        if own_ctx:
            for c in ctxs:
                c.close()


SWEEP_COLUMNS = ("P", "TP", "FP", "FN", "TPR", "PPV", "FNR", "FDR", "F", "FM")


def _agg_row(agg):
    return {"P": agg.total_positives_sec, "TP": agg.true_positives_sec, "FP": agg.false_positives_sec, "FN": agg.false_negatives_sec,
            "TPR": agg.true_positive_rate.overall, "PPV": agg.precision.overall, "FNR": agg.false_negative_rate.overall,
            "FDR": agg.false_discovery_rate.overall, "F": agg.f_score, "FM": agg.fm_index}


# configs from which the VAD machines run on the GPU when run_sweep is left to choose: the measured crossover against 16 host threads
# (tools/vad_sweep_time.py, 21 two-hour streams: the GPU machines are slower below 256 configs, about even at 256)
SWEEP_DEVICE_MIN_CONFIGS = 256
# the same threshold with vad_chain="coop" (the machines' exact long-term chains run by the whole wavefront)
SWEEP_DEVICE_MIN_CONFIGS_COOP = 192
VAD_CHAINS = ("lane", "coop")
# vad_avgs: where the device machines' short-term and channel-ratio averages come from (context option vad_avgs, DESIGN section
# 7.1): each machine's own rings, or tables filled frame-parallel before the launch -- only the cooperative kernel reads those
VAD_AVGS = ("ring", "table")
# vad_trigger: one full device machine per (stream, config), or one trigger machine per (stream, trigger key) that emits bits and
# a finishing kernel per config (context option vad_trigger) -- only the cooperative kernel emits
VAD_TRIGGERS = ("config", "shared")


def _check_vad_chain(vad_chain, vad_avgs=None, vad_trigger=None):
    if vad_trigger is not None and vad_trigger not in VAD_TRIGGERS:
        raise ValueError(f"vad_trigger: {vad_trigger!r} (one of {VAD_TRIGGERS})")
    if vad_trigger == "shared" and vad_chain != "coop":
        raise ValueError(f"vad_trigger='shared' needs vad_chain='coop' (vad_chain: {vad_chain!r}): only the cooperative form of the "
                         "machines' kernel emits the triggers' bits")
    if vad_chain is not None and vad_chain not in VAD_CHAINS:
        raise ValueError(f"vad_chain: {vad_chain!r} (one of {VAD_CHAINS})")
    if vad_avgs is not None and vad_avgs not in VAD_AVGS:
        raise ValueError(f"vad_avgs: {vad_avgs!r} (one of {VAD_AVGS})")
    if vad_avgs == "table" and vad_chain != "coop":
        raise ValueError(f"vad_avgs='table' needs vad_chain='coop' (vad_chain: {vad_chain!r}): only the cooperative form of the "
                         "machines' kernel reads the averages' tables")


_MAX_TIMES = ("avgs_form", "avgs_bytes", "trigger_form", "trigger_bytes", "trigger_keys")   # forms and sizes: the largest, not a sum


def _note_avgs(times, b):
    """times' avgs_form / avgs_bytes after a device launch of b: the largest form (2: a launch read the tables) and table size"""
    times["avgs_form"] = max(times.get("avgs_form", 0), b.avgs_form())
    times["avgs_bytes"] = max(times.get("avgs_bytes", 0), b.avgs_bytes())
    # the shared-trigger form of the launch: the largest form (2: shared), the bits' size, the keys of the configs it ran
    times["trigger_form"] = max(times.get("trigger_form", 0), b.trigger_form())
    times["trigger_bytes"] = max(times.get("trigger_bytes", 0), b.trigger_bytes())
    times["trigger_keys"] = max(times.get("trigger_keys", 0), len(b.trigger_keys()[1]))


def _auto_vad_on(n_configs, vad_chain):
    return "device" if n_configs >= (SWEEP_DEVICE_MIN_CONFIGS_COOP if vad_chain == "coop" else SWEEP_DEVICE_MIN_CONFIGS) else "host"


class _VadChain:
    """The context options vad_chain and vad_avgs on the contexts of one run_sweep / run_grid call: set on entry (nothing for
    one that is None), and on a caller's context (owned False) put back on exit to what it was set to before"""

    def __init__(self, vad_chain, vad_avgs=None, vad_trigger=None):
        self.values, self.restore = {"vad_chain": vad_chain, "vad_avgs": vad_avgs, "vad_trigger": vad_trigger}, []

    def apply(self, ctx, owned):
        if ctx is None:
            return
        for name, value in self.values.items():
            if value is None:
                continue
            prev = ctx.option_set(name)
            ctx.set_option(name, value)
            if not owned:
                self.restore.append((ctx, name, prev))

    def close(self):
        for ctx, name, prev in reversed(self.restore):
            ctx.set_option(name, prev)
        self.restore = []


def _engine_opts(config0, F):
    """the engine's options for a sweep's denoising pass: it sums config 0's band at F points (FFT.freqToBin as the library
    computes it); the sweep's bands come from their own pass"""
    probe = fv.VadSweep(1, [config0], fft_size=F)
    (min_bin, max_bin), = probe.bands()[0]
    probe.close()
    opts = fv.EngineOpts()
    fv.lib().fvad_engine_opts_default(fv.C.byref(opts))
    opts.min_bin, opts.max_bin, opts.fft_size = min_bin, max_bin, F
    return opts


_Resident = collections.namedtuple("_Resident", "groups order n_chunks n_lanes n_samples stride n_den nf_all d_pcm d_den d_band0 rms")


def _denoise_for_sweep(ctx, audio, F, config0, dalloc):
    """_denoise_resident as the sweeps take it: (groups, n_chunks, n_den, nf_all, d_den, chunk RMS)"""
    r = _denoise_resident(ctx, audio, F, config0, dalloc)
    return r.groups, r.n_chunks, r.n_den, r.nf_all, r.d_den, r.rms


def _denoise_resident(ctx, audio, F, config0, dalloc):
    """The denoising pass of a sweep: every channel of every instance is one lane of ONE device batch (ragged lengths padded to
    the longest: chunks are causal, so padding changes no real chunk), fvad_engine_enqueue_device with the denoised audio kept
    (device memory from dalloc).  Instances are grouped by channel count (a VAD batch has one channel count), each group's lanes
    side by side.  Returns a _Resident: groups {n_channels: [instance]}, order (the instances in lane order), n_chunks [instance],
    the original lanes d_pcm (n_lanes of n_samples f32, `stride` apart), the denoised lanes d_den (n_den samples each), config 0's
    band sums d_band0 [lane][nf_all], chunk RMS [lane][chunk] on the host."""
    chunk = 24000
    lens = [_dims(p)[1] for p in audio]
    n_chunks = [n // chunk for n in lens]
    L = max(lens)
    stride = (L + 3) // 4 * 4                        # 16-byte aligned lanes
    groups = {}
    for i, p in enumerate(audio):
        groups.setdefault(_dims(p)[0], []).append(i)
    order = [i for members in groups.values() for i in members]
    n_lanes = sum(_dims(audio[i])[0] for i in order)
    n_ck = L // chunk
    n_den = n_ck * chunk
    nf_all = n_den // F
    opts = _engine_opts(config0, F)
    if _is_raw(audio):   # ingest "device": one source per instance, the lanes decoded and padded to `stride` by the ingest kernel
        d_pcm = dalloc(n_lanes * stride * 4)
        rows, l = [], 0
        for i in order:
            rows.append(audio[i].source(0, audio[i].n_frames, l, 0, stride))
            l += audio[i].n_channels
        _ingest_rows(ctx, [audio[i] for i in order], rows, d_lanes=d_pcm, n_lanes=n_lanes, lane_stride=stride, n_samples=stride)
    else:
        host = np.zeros((n_lanes, stride), np.float32)   # filled channel by channel: no other f32 copy of the corpus
        l = 0
        for i in order:
            p = audio[i]
            for c in range(p.shape[0]):
                if p.dtype == np.int16:   # the kernel's PCM16 decode, exact in f32
                    np.multiply(p[c], np.float32(1.0 / 32768.0), out=host[l, :p.shape[1]], casting="unsafe")
                else:
                    host[l, :p.shape[1]] = p[c]
                l += 1
        d_pcm = dalloc(host.nbytes)
        ctx.to_device(d_pcm, host)
        del host
    d_den = dalloc(n_lanes * n_den * 4)
    d_band0 = dalloc(n_lanes * max(nf_all, 1) * 4)
    d_rms = dalloc(n_lanes * max(n_ck, 1) * 4)
    if n_ck:
        ctx._ck(fv.lib().fvad_engine_enqueue_device(ctx.h, fv.vp(d_pcm), n_lanes, stride, L, fv.vp(d_den), fv.vp(d_band0),
                                                    fv.vp(d_rms), fv.C.byref(opts)), "fvad_engine_enqueue_device")
    rms = np.zeros((n_lanes, max(n_ck, 1)), np.float32)
    if n_ck:
        ctx.to_host(rms, d_rms)
    return _Resident(groups, order, n_chunks, n_lanes, L, stride, n_den, nf_all, d_pcm, d_den, d_band0, rms)


# What every share of a sweep needs (run_grid makes one per call; run_sweep one without scoring): the configs, their Evaluator
# StatConfigs and frame sizes (sizes_of[c]; F, the plan's, for every config of a grid without "fft_size"), sized (the grid has
# "fft_size": the batches are made with fvad_vad_batch_create_sweep_sized), and run_grid's arguments of the same names, n_threads
# per share
_SweepJob = collections.namedtuple("_SweepJob", "configs stat_cfgs sizes_of sized F slice_chunks vad_on score_on n_threads overlap")


def _new_batch(job, n_streams, nch):
    """a batch of the job's configs; whichever kind it is, the run paths use its sizes, size_blocks() and sample-based calls"""
    if job.sized:
        return fv.VadSweepSized(n_streams, job.configs, job.sizes_of, n_channels=nch)
    return fv.VadSweep(n_streams, job.configs, n_channels=nch, fft_size=job.F)


def _group_band_sums(ctx, b, members, n_chunks, d_gden, n_lanes, n_den, dalloc):
    """The band sums of a channel-count group of an unsliced sweep, for batch b over the group's n_lanes lanes of denoised audio
    at d_gden: one fvad_engine_band_sums_device pass per frame size into its run of band blocks.  Returns (the bands' device
    address, their stride: the frames of the smallest size, the frames to run [size][stream])."""
    bstride = max(n_den // min(b.sizes), 1)
    d_gband = dalloc(len(b.size_of_band) * n_lanes * bstride * 4)
    for Fg, j0, bins_g in b.size_blocks():
        if n_den // Fg:
            ctx.band_sums_device(d_gden, n_lanes, n_den, n_den, bins_g, d_gband + j0 * n_lanes * bstride * 4, bstride, fft_size=Fg)
    return d_gband, bstride, [[n_chunks[i] * 24000 // Fg for i in members] for Fg in b.sizes]


def _group_machines(ctx, job, b, members, nch, d_gband, bstride, nf, g_rms, n_chunks, times, done, stop=None):
    """The machines of a group over _group_band_sums' output: in b on the device, or with vad_on "host" in one single-stream
    host batch per instance (instances differ in length), closed before the next is made.  done(batch, the instances it
    holds) is called once a batch's machines have run; their time is added to times["machines"].  With device scoring (the
    caller has set b's references) the context's kernel timing is on around the run if it was off, and the scoring kernel's
    time goes to times["scoring"] instead (a caller's own timing records are left alone: the machines' time then includes the
    scoring).  stop: checked before every host batch."""
    if job.vad_on == "device":
        timed = job.score_on == "device" and not ctx.timing
        if timed:
            ctx.enable_timing(True)
        try:
            t0 = time.perf_counter()
            b.run_device_sized(ctx, d_gband, bstride, nf, g_rms, [n_chunks[i] for i in members])
            wall = time.perf_counter() - t0
            score_s = ctx.kernel_times().get("vad_score", 0.0) / 1e3 if timed else 0.0
        finally:
            if timed:
                ctx.enable_timing(False)
        times["machines"] += wall - score_s
        times["scoring"] += score_s
        _note_avgs(times, b)
        done(b, members)
        return
    gband = ctx.to_host(np.empty((len(b.size_of_band), len(members) * nch, bstride), np.float32), d_gband)
    for k, i in enumerate(members):
        if stop is not None:
            _check_stop(stop)
        one = _new_batch(job, 1, nch)
        try:
            t0 = time.perf_counter()
            nf_i = [row[k] for row in nf]
            one.run_sized(np.ascontiguousarray(gband[:, k * nch:(k + 1) * nch, :max(max(nf_i), 1)]),
                          np.ascontiguousarray(g_rms[k * nch:(k + 1) * nch, :max(n_chunks[i], 1)]), nf_i, n_threads=job.n_threads)
            times["machines"] += time.perf_counter() - t0
            done(one, [i])
        finally:
            one.close()


def run_sweep(plan_path, ctx=None, synth_seed=None, configs=None, out=sys.stdout, json_path=None, vad_on="auto", n_threads=16,
              vad_chain=None, vad_avgs=None, vad_trigger=None, ingest="host"):
    """Scores many VADMachine configurations over one denoising pass of a plan's instances.

    configs: list of VADMachine.Config override dicts (vad_overrides' form); default: the plan's vad_machine_config followed by its
    alt_vad_machine_configs (VADPipeline.zig:110-122).  Flow: every channel of every instance is one lane of ONE device batch
    (ragged lengths padded to the longest: chunks are causal, so padding changes no real chunk) -> fvad_engine_enqueue_device with
    the denoised audio kept -> per channel-count group, fvad_engine_band_sums_device for the configs' distinct speech bands ->
    the VAD machines -> per (instance, config) the Evaluator statistics against the labels, aggregated in plan order like
    run_plan's report (statistics.zig:116-172).  vad_on: "device" (fvad_vad_batch_run_device, every (instance, config) machine on
    the GPU), "host" (fvad_vad_batch_run on n_threads host threads over the band sums, one call per instance) or "auto" (the GPU
    from SWEEP_DEVICE_MIN_CONFIGS configs on); both give the same bits.  vad_chain "lane" or "coop": the context option of that
    name for this call (how the device machines run their exact long-term chains; same bits; "auto" then takes
    SWEEP_DEVICE_MIN_CONFIGS_COOP for "coop"), set on the context the call makes, or on the caller's and put back afterwards;
    None leaves the context as it is; anything else is a ValueError before any device is touched.  vad_avgs "ring" or "table": the
    context option of that name, handled the same way (the device machines' short-term and channel-ratio averages from their
    own rings or from tables filled before the launch; same bits); "table" without vad_chain="coop" is a ValueError.

    Returns dict(configs, rows [one aggregate dict per config], aggregates [AggregateStats], segments [config][instance],
    stats [config][instance], avgs_form, avgs_bytes [VadSweep.avgs_form() / avgs_bytes(): the largest over the device
    launches; 0 with host machines]); prints one table row per config and writes the rows as JSON to json_path if given.
    ingest as in run_grid."""
    _check_vad_chain(vad_chain, vad_avgs, vad_trigger)
    _check_ingest(ingest)
    plan = load_plan(plan_path)
    if configs is None:
        configs = [plan["vad_machine_config"]] + list(plan["alt_vad_machine_configs"])
    configs = [dict(c) for c in configs]
    if vad_on == "auto":
        vad_on = _auto_vad_on(len(configs), vad_chain)
    if vad_on not in ("device", "host"):
        raise ValueError(f"vad_on: {vad_on!r}")
    F = plan["fft_size"]
    own_ctx = ctx is None
    if own_ctx:
        ctx = _make_ctx(plan, 0, synth_seed)
    chain = _VadChain(vad_chain, vad_avgs, vad_trigger)
    loaded = _load_instances(plan, ingest)
    audio = [a for a, _ in loaded]
    refs = [r for _, r in loaded]
    t0 = time.perf_counter()
    chunk = 24000
    allocs = []

    def dalloc(nbytes):
        a = ctx.device_alloc(max(int(nbytes), 16))
        allocs.append(a)
        return a

    segs = [[None] * len(audio) for _ in configs]
    job = _SweepJob(configs=configs, stat_cfgs=None, sizes_of=[F] * len(configs), sized=False, F=F, slice_chunks=None, vad_on=vad_on,
                    score_on="host", n_threads=n_threads, overlap=False)

    def keep_segments(batch, insts):
        for c in range(len(configs)):
            for i, per in zip(insts, batch.segments(c)):
                segs[c][i] = per

    times = {"machines": 0.0, "scoring": 0.0}
    try:
        chain.apply(ctx, own_ctx)
        groups, n_chunks, n_den, _, d_den, rms = _denoise_for_sweep(ctx, audio, F, configs[0], dalloc)
        l0 = 0
        for nch, members in groups.items():
            sweep = _new_batch(job, len(members), nch)
            try:
                g_lanes = list(range(l0, l0 + len(members) * nch))
                l0 += len(g_lanes)
                d_gband, bstride, nf = _group_band_sums(ctx, sweep, members, n_chunks, d_den + g_lanes[0] * n_den * 4, len(g_lanes),
                                                        n_den, dalloc)
                _group_machines(ctx, job, sweep, members, nch, d_gband, bstride, nf, np.ascontiguousarray(rms[g_lanes]), n_chunks,
                                times, keep_segments)
            finally:
                sweep.close()
    finally:
        for a in allocs:
            ctx.device_free(a)
        chain.close()
        if own_ctx:
            ctx.close()
    elapsed = time.perf_counter() - t0
    rows, aggs, all_stats = [], [], []
    for c, cfg in enumerate(configs):
        stat_cfg = {"ignore_shorter_than_sec": float(np.float32(cfg.get("min_vad_duration_sec", 0.7))),
                    "extrude_start": 5.0, "extrude_end": 10.0, "fill_gaps": 5.0}
        stats = []
        for i, ref in enumerate(refs):
            secs = [(float(np.float32(x[0]) / np.float32(48000)), float(np.float32(x[1]) / np.float32(48000))) for x in segs[c][i]]
            stats.append(fv.stats_from_segments(secs, ref, stat_cfg))
        agg = fv.stats_aggregate(stats)
        aggs.append(agg)
        all_stats.append(stats)
        rows.append(dict(config=c, **_agg_row(agg)))
    result = {"configs": configs, "rows": rows, "aggregates": aggs, "segments": segs, "stats": all_stats,
              "avgs_form": times.get("avgs_form", 0), "avgs_bytes": times.get("avgs_bytes", 0),
              "trigger_form": times.get("trigger_form", 0), "trigger_bytes": times.get("trigger_bytes", 0),
              "trigger_keys": times.get("trigger_keys", 0)}
    if json_path:
        with open(json_path, "w") as f:
            json.dump({"configs": configs, "rows": rows, "avgs_form": result["avgs_form"], "avgs_bytes": result["avgs_bytes"],
                       "trigger_form": result["trigger_form"], "trigger_bytes": result["trigger_bytes"], "trigger_keys": result["trigger_keys"],
                       "segments": [[[list(map(float, x)) for x in inst] for inst in per] for per in segs]}, f, indent=1)
    if out is not None:
        out.write("| config |      P |     TP |     FP |     FN |    TPR |    PPV |    FNR |    FDR | F-score |    FMI |\n")
        for r in rows:
            out.write("| {:>6} | {} | {} | {} | {} | {}% | {}% | {}% | {}% | {}% | {}% |\n".format(
                r["config"], _f(r["P"], 6, 1), _f(r["TP"], 6, 1), _f(r["FP"], 6, 1), _f(r["FN"], 6, 1),
                *[_f(np.float32(r[k]) * np.float32(100), 5, 1) for k in ("TPR", "PPV", "FNR", "FDR")],
                _f(np.float32(r["F"]) * np.float32(100), 6, 1), _f(np.float32(r["FM"]) * np.float32(100), 5, 1)))
        out.write(f"[{len(configs)} configs x {len(audio)} instances in {elapsed:.2f} s]\n")
    return result



def _stat_cfg(cfg):
    """the Evaluator's StatConfig of a config (simulator.zig:127-132): labels shorter than its min_vad_duration_sec are ignored"""
    return {"ignore_shorter_than_sec": float(np.float32(cfg.get("min_vad_duration_sec", 0.7))),
            "extrude_start": 5.0, "extrude_end": 10.0, "fill_gaps": 5.0}


# the largest grid run_grid accepts: every config is one VAD machine per instance, each with its own long-term ring on the device
# (34 KB at the default 180 s: 4096 configs x 21 instances are 2.9 GB)
GRID_MAX_CONFIGS = 16384


def expand_grid(grid):
    """Grid {"base": {overrides}, "axes": {field: [values]}} -> the configs (vad_overrides' form): the cartesian product of the
    axes in file order, the last axis fastest, each on top of base (both in the plan's vad_machine_config form).  Raises
    ValueError for an unknown field, an empty axis or more than GRID_MAX_CONFIGS configs."""
    if not isinstance(grid, dict):
        raise ValueError("a grid is a JSON object with \"base\" and \"axes\"")
    extra = [k for k in grid if k not in ("base", "axes")]
    if extra:
        raise ValueError(f"unknown grid key(s) {extra}: a grid has \"base\" and \"axes\"")
    base = grid.get("base") or {}
    axes = grid.get("axes") or {}
    if not isinstance(base, dict) or not isinstance(axes, dict):
        raise ValueError("grid \"base\" and \"axes\" are JSON objects")
    for k in list(base) + list(axes):
        if k not in VAD_FIELDS:
            raise ValueError(f"unknown VADMachine.Config field {k!r} in the grid; valid fields: {', '.join(VAD_FIELDS)}")
    n = 1
    for k, vals in axes.items():
        if not isinstance(vals, list) or not vals:
            raise ValueError(f"grid axis {k!r} is empty (an axis is a non-empty list of values)")
        n *= len(vals)
    if n > GRID_MAX_CONFIGS:
        raise ValueError(f"the grid has {n} configs, more than GRID_MAX_CONFIGS = {GRID_MAX_CONFIGS}")
    configs = []
    for combo in itertools.product(*axes.values()):
        c = dict(base)
        c.update(zip(axes.keys(), combo))
        try:
            configs.append(vad_overrides(c))
        except (TypeError, ValueError) as e:
            raise ValueError(f"grid values must be numbers (initial_long_term_avg may be null): {c}") from e
    return configs


FFT_SIZE_MIN, FFT_SIZE_MAX = 4, 16384


def expand_grid_sized(grid, plan_fft_size):
    """A grid that may also carry a top-level "fft_size": [sizes] next to "base" and "axes" (VADPipeline.Config.fft_size beside
    its vad_machine_config) -> (sizes, configs): sizes[c] is config c's frame size.  The size is the slowest axis: every config
    of expand_grid(grid without the key) at the first size, then at the second, ...; the product counts against
    GRID_MAX_CONFIGS.  Sizes are even integers in 4..16384 without duplicates.  Without the key every config runs at
    plan_fft_size (None: the caller fills it in) and the configs are expand_grid's.  Raises ValueError (before any GPU work)."""
    if not isinstance(grid, dict) or "fft_size" not in grid:
        configs = expand_grid(grid)
        return [plan_fft_size] * len(configs), configs
    sizes = grid["fft_size"]
    if not isinstance(sizes, list) or not sizes:
        raise ValueError(f"grid \"fft_size\" = {sizes!r}: a non-empty list of frame sizes")
    for f in sizes:
        if isinstance(f, bool) or not isinstance(f, int) or f < FFT_SIZE_MIN or f > FFT_SIZE_MAX or f % 2:
            raise ValueError(f"grid \"fft_size\" value {f!r}: a frame size is an even integer in {FFT_SIZE_MIN}..{FFT_SIZE_MAX}")
    if len(set(sizes)) != len(sizes):
        raise ValueError(f"grid \"fft_size\" = {sizes}: a size appears twice")
    base = expand_grid({k: v for k, v in grid.items() if k != "fft_size"})
    n = len(sizes) * len(base)
    if n > GRID_MAX_CONFIGS:
        raise ValueError(f"the grid has {n} configs ({len(sizes)} fft_size values x {len(base)}), more than "
                         f"GRID_MAX_CONFIGS = {GRID_MAX_CONFIGS}")
    return [f for f in sizes for _ in base], [dict(c) for _ in sizes for c in base]


def _ranked(rows):
    """rows by aggregate F-score, highest first (NaN last), ties by config index"""
    return sorted(rows, key=lambda r: (0, -r["F"], r["config"]) if r["F"] == r["F"] else (1, 0.0, r["config"]))


def slice_align(fft_size, chunk=24000):
    """the chunks a time slice of a sliced grid is a multiple of: lcm(chunk, fft_size) / chunk, so that every slice starts on a
    frame (16 at fft_size 1024)"""
    return math.lcm(chunk, int(fft_size)) // chunk


def check_slice_chunks(slice_chunks, fft_size):
    """ValueError unless slice_chunks is a positive multiple of slice_align(fft_size)"""
    a = slice_align(fft_size)
    if isinstance(slice_chunks, bool) or not isinstance(slice_chunks, (int, np.integer)) or slice_chunks <= 0 or slice_chunks % a:
        raise ValueError(f"slice_chunks = {slice_chunks!r}: a time slice is a positive multiple of {a} chunks at fft_size {fft_size} "
                         f"(lcm(24000, fft_size) / 24000: slices start on a frame)")


def check_slice_chunks_sized(slice_chunks, sizes):
    """ValueError unless slice_chunks is a positive multiple of the lcm of slice_align over the frame sizes"""
    sizes = sorted(set(int(f) for f in sizes))
    if len(sizes) == 1:
        return check_slice_chunks(slice_chunks, sizes[0])
    a = math.lcm(*[slice_align(f) for f in sizes])
    if isinstance(slice_chunks, bool) or not isinstance(slice_chunks, (int, np.integer)) or slice_chunks <= 0 or slice_chunks % a:
        raise ValueError(f"slice_chunks = {slice_chunks!r}: a time slice is a positive multiple of {a} chunks at fft_size {sizes} "
                         f"(the lcm of lcm(24000, fft_size) / 24000 over the sizes: slices start on a frame of every size)")


_Context = fv.Context   # the class, for run_grid's argument check


def _check_grid_contexts(ctx, devices):
    """run_grid's rules for ctx and devices (ValueError, before any context is made or GPU work done) -> the number of shares,
    or None for one context (ctx a Context or None and devices None)"""
    if ctx is not None and devices is not None:
        raise ValueError("run_grid takes ctx or devices, not both")
    if devices is not None:
        if not isinstance(devices, (list, tuple)) or not devices:
            raise ValueError(f"devices = {devices!r}: a non-empty list of HIP device indices")
        for d in devices:
            if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or d < 0:
                raise ValueError(f"devices: {d!r} is not a HIP device index (an integer >= 0)")
        return len(devices)
    if isinstance(ctx, (list, tuple)):
        if not ctx:
            raise ValueError("ctx = []: a list of contexts is not empty")
        for c in ctx:
            if not isinstance(c, _Context):
                raise ValueError(f"ctx: {c!r} is not a Context")
        if len({id(c) for c in ctx}) != len(ctx):
            raise ValueError("ctx: a context appears twice (each share runs on a context of its own; two contexts may share "
                             "a device)")
        return len(ctx)
    return None


def run_grid(plan_path, grid, top=20, vad_on="auto", score_on="auto", json_path=None, ctx=None, synth_seed=None, out=sys.stdout,
             n_threads=16, slice_chunks=None, halving_eta=None, halving_rungs=None, devices=None, overlap=False, vad_chain=None,
             vad_avgs=None, vad_trigger=None, ingest="host"):
    """A grid sweep: every config of a parameter grid (expand_grid; grid: the dict or a path to its JSON file) scored over one
    denoising pass of a plan's instances, without returning segments.  The flow is run_sweep's (one device batch for the
    denoising, per channel-count group a multi-band K4 pass and the VAD machines); then every (instance, config) machine is
    scored against the instance's labels -- score_on "device": on the GPU next to its segments (fvad_vad_batch_run_device with
    references set and keep_segments 0: only counts, audits and the statistics come back), "host": fvad_vad_batch_score on
    n_threads host threads; "auto": where the machines ran.  vad_on as in run_sweep.  Both scorers give run_sweep's bits.
    Per config, fvad_stats_aggregate over the instances in plan order.  The grid is checked before any GPU work.  With device
    scoring, the context's kernel timing is switched on around each fvad_vad_batch_run_device call (for the scoring kernel's
    time) if it was off, and off again after it; a caller that has it on keeps its records, and the machines' time then
    includes the scoring.  Labels must be numbers: the scorers walk them sorted, so a NaN label (fvad_parse_audacity reads
    "nan") is refused (ValueError, before any GPU work), where run_sweep's per-pair fvad_stats_from_segments takes it.

    slice_chunks = N runs the whole pipeline in time slices of N chunks (a positive multiple of slice_align(fft_size), 16 at
    fft_size 1024; ValueError before any GPU work otherwise), so that device and host memory are bounded by the slice, not the
    corpus (_grid_sliced): the audio is read slice by slice from the mapped files (wav_map), each slice denoised from zero
    history with its SLICE_HALO_CHUNKS-chunk halo, its band sums computed, and the machines run on in parts
    (fvad_vad_batch_run_device_part_sized, or fvad_vad_batch_run_sized with vad_on "host").  On a context with the option
    reproducible = 1 the statistics are the unsliced run's bit for bit; by default the NN kernels the engine selects depend on
    the launch size, which can move the gains by about 1e-6 and flip a decision.  None: everything in one pass, as above.

    Returns dict(configs, rows [one aggregate dict per config, config order], aggregates [AggregateStats], stats float32
    [config][instance][11] (fvad_single_stats), times {stage: s}, slices [number of time slices; 1 unsliced], device_bytes);
    prints the top rows by F-score and the stage times, and writes the configs and all rows as JSON to json_path if given.
    device_bytes is set when sliced (else None): the peak of the slice buffers run_grid allocates, plus the largest
    VadSweep.device_bytes() of a batch, plus the engine's launch workspace for a slice's chunks computed from shapes
    (ENGINE_WS_BYTES_PER_CHUNK).  It excludes the context's own buffers (weights, FFT plans, the K4 pass's job
    list), each part's frame ratios and the HIP runtime's overhead.

    halving_eta = eta, halving_rungs = R: successive halving over the time slices (both or neither; slice_chunks, vad_on "device"
    and score_on "device" required, eta >= 2, R >= 1; ValueError before any GPU work otherwise).  The slices run one after the
    other across the channel-count groups, every group's batch alive; at each rung of halving_schedule(longest instance in
    chunks, slice_chunks, eta, R) every config is scored on the prefix run so far against the labels cut to it, the
    ceil(n / eta) best by aggregate F-score (ties to the lower config index) are kept and the other configs' machines are
    dropped from the batches (VadSweep.retain), so that later slices run fewer machines in less memory.  The result then also
    has survivors (config indices), rung (per config: the rung it was dropped at, 1-based, None for survivors),
    evaluated_seconds (per config: the seconds of audio its machines ran over all instances) and rung_times (per rung: end
    chunk, configs in, configs kept, seconds; a last entry with rung None for the survivors' run to the end); stats holds the
    whole corpus's statistics for survivors and the last prefix's for dropped configs, and the rows carry rung and
    evaluated_seconds.  The table ranks the survivors, then prints one line per rung.

    Several devices: devices = [HIP device indices] (one context made and closed per entry, as run_plan makes them; an index
    may repeat) or ctx = [Context, ...] (the caller's, with the caller's options, left open) deals the instances to shares:
    instance i to share i % n in plan order (instance_shares, as run_plan).  One host thread per share runs the flow above
    on its own context over its own instances -- the denoising batch padded to the share's longest instance, its own
    channel-count groups, slice buffers sized for its own largest group -- and writes its instances' columns of stats; a
    share without instances makes no context and does no work.  Host machines and host scoring get max(1, n_threads //
    shares at work) threads each.  With halving, the rungs are those of the whole plan's longest instance: at each rung
    every share scores its batches, one thread aggregates stats over all instances in plan order and picks the configs to
    keep, and every share retains them, so survivors, rung, evaluated_seconds and the rung ends and counts are one
    context's.  The aggregates, ranking, table and JSON are built over all instances in plan order as above.  If a share
    fails, the others stop at their next slice or rung, everything is freed (the contexts run_grid made closed) and the
    first exception is raised here.  ValueError (before any context or GPU work) for both ctx and devices, an empty list,
    a device index that is not an integer >= 0, or a ctx list holding something other than a Context, or one twice.  On
    contexts with the option reproducible = 1 the statistics are the single context's bit for bit, sliced or not; by
    default the NN kernels the engine selects depend on the launch size, which can move the gains by about 1e-6 and flip
    a decision.  The result then also has share_times (per share: device, instances, wall seconds, stage times) and
    device_bytes_per_share (each share's device_bytes); times and slices are sums over the shares (times in GPU-seconds),
    device_bytes the largest share's, and with more than one share the summary line adds each share's wall time.  With one
    context (ctx a Context or None, devices None) no thread is started and the result is as described above.
    overlap=True (with slice_chunks, device machines and device scoring; ValueError otherwise): each slice's machines run beside the
    next slice's reading and denoising -- their frame ratios computed on the device from the engine's chunk RMS, the parts started
    with fvad_vad_batch_run_device_part_async on the context's second stream and waited for only when their buffers are needed
    again, at a rung and at the end.  Plain, sized and halving grids, and every share of a ctx / devices list on its own context.
    On reproducible contexts the statistics, survivors, rungs and evaluated_seconds are those of overlap=False bit for bit.
    times gains machines_wait (the host time inside the waits, counted in machines too); device_bytes counts the second set
    of the bands and rms buffers.
    vad_chain and vad_avgs as in run_sweep: set on every context the call makes, and on the caller's contexts for the call;
    times gains avgs_form and avgs_bytes (the largest over the shares' device launches: 2 once a launch read the tables, and
    the largest part's tables in bytes), which the JSON file carries too.
    ingest "host" (the default): the files are read, or with slice_chunks mapped, de-interleaved and converted to f32 on the
    host and uploaded as f32.  "device": every file's data chunk is mapped as bytes (wav_map_raw), sliced or not, and
    fvad_ingest takes the bytes to the GPU as they are -- PCM16 at 2 bytes per sample -- where one kernel de-interleaves,
    decodes and pads them into the same f32 lanes: the same bits downstream, hence the same result.  24-bit PCM files run with
    "device" only; "host" refuses them (FvadError naming --ingest device).  The same holds for files at another rate than 48 kHz
    (44.1 kHz, 32 kHz, 16 kHz ...: any rate whose ratio to 48000 has up <= 640): with "device" fvad_ingest_resample filters and
    re-times them into 48 kHz lanes while it decodes them (one call per rate beside the 48 kHz files' fvad_ingest), labels,
    segments and reports stay in 48 kHz terms, and a sliced run equals the unsliced one; "host" refuses them with status -9."""
    _check_vad_chain(vad_chain, vad_avgs, vad_trigger)
    _check_ingest(ingest)
    n_shares = _check_grid_contexts(ctx, devices)   # None: one context, today's path without a thread
    if isinstance(grid, str):
        with open(grid) as f:
            grid = json.load(f)
    sizes_of, configs = expand_grid_sized(grid, None)
    sized = "fft_size" in grid   # (a grid without the key runs every config at the plan's fft_size: expand_grid's configs)
    if vad_on == "auto":
        vad_on = _auto_vad_on(len(configs), vad_chain)
    if vad_on not in ("device", "host"):
        raise ValueError(f"vad_on: {vad_on!r}")
    if score_on == "auto":
        score_on = vad_on
    if score_on not in ("device", "host"):
        raise ValueError(f"score_on: {score_on!r}")
    if score_on == "device" and vad_on != "device":
        raise ValueError("score_on='device' scores next to the device machines: it needs vad_on='device'")
    if overlap:
        if slice_chunks is None:
            raise ValueError("overlap runs a slice's machines beside the next slice's denoising: it needs slice_chunks")
        if vad_on != "device" or score_on != "device":
            raise ValueError(f"overlap leaves the machines and their segments on the device: it needs vad_on='device' and "
                             f"score_on='device' (got {vad_on!r}, {score_on!r})")
    halving = None
    if halving_eta is not None or halving_rungs is not None:
        if halving_eta is None or halving_rungs is None:
            raise ValueError("halving_eta and halving_rungs go together")
        if slice_chunks is None:
            raise ValueError("successive halving drops configs between time slices: it needs slice_chunks")
        if vad_on != "device":
            raise ValueError(f"successive halving drops device machines: it needs vad_on='device' (got {vad_on!r})")
        if score_on != "device":
            raise ValueError(f"successive halving scores its rungs on the device: it needs score_on='device' (got {score_on!r})")
        halving_schedule(1, 1, halving_eta, halving_rungs)   # (eta and rungs checked)
        halving = {"eta": int(halving_eta), "rungs": int(halving_rungs)}
    plan = load_plan(plan_path)
    F = plan["fft_size"]
    sizes_of = [F if f is None else f for f in sizes_of]
    if slice_chunks is not None:
        check_slice_chunks_sized(slice_chunks, sizes_of)
    stat_cfgs = [_stat_cfg(c) for c in configs]
    loaded = _load_instances(plan, ingest, mapped=slice_chunks is not None)   # (sliced: the audio stays in its files, mapped)
    for inst, (_, ref) in zip(plan["instances"], loaded):
        if any(x != x for r in ref for x in r):
            raise ValueError(f"{inst['ref_path']}: a NaN label; grid scoring walks the labels sorted by start and needs "
                             "numbers (fvad_vad_batch_set_references refuses NaN)")
    audio = [a for a, _ in loaded]
    refs = [r for _, r in loaded]
    NC, n_inst = len(configs), len(audio)
    stats = np.empty((NC, n_inst, len(fv.SingleStats._fields_)), np.float32)
    shares = instance_shares(n_inst, n_shares or 1)
    workers = [s for s, share in enumerate(shares) if share]   # an empty share makes no context and does no work
    if n_shares is None:   # one context: no thread
        ctxs, owned = [ctx if ctx is not None else _make_ctx(plan, 0, synth_seed)], [ctx is None]
    elif devices is not None:
        ctxs, owned = [None] * n_shares, [True] * n_shares
        try:
            for s in workers:
                ctxs[s] = _make_ctx(plan, int(devices[s]), synth_seed)
        except BaseException:
            for c in ctxs:
                if c is not None:
                    c.close()
            raise
    else:
        ctxs, owned = list(ctx), [False] * n_shares
    rungs = None
    if halving is not None:   # the schedule over the longest instance of the whole plan, whatever the shares
        rungs = _Rungs(len(workers), halving, [_dims(a, mapped=True)[1] // 24000 for a in audio], int(slice_chunks), stats, stat_cfgs)
    share_times = [{"device": int(devices[s]) if devices is not None else getattr(ctxs[s], "device", None), "instances": shares[s],
                    "wall": 0.0, "times": {}} for s in range(len(shares))]
    share_out = [(0, None)] * len(shares)
    job = _SweepJob(configs=configs, stat_cfgs=stat_cfgs, sizes_of=sizes_of, sized=sized, F=F,
                    slice_chunks=None if slice_chunks is None else int(slice_chunks), vad_on=vad_on, score_on=score_on,
                    n_threads=max(1, n_threads // max(len(workers), 1)), overlap=bool(overlap))
    stop = threading.Event()   # set when a worker fails: the others stop at their next slice or rung
    errs, breaks = [], []
    t_all = time.perf_counter()
    chain = _VadChain(vad_chain, vad_avgs, vad_trigger)

    def work(s):
        t0 = time.perf_counter()
        st = share_times[s]["times"]
        st.update(denoise=0.0, bands=0.0, machines=0.0, scoring=0.0)
        ids = np.asarray(shares[s], np.intp)
        try:
            share_out[s] = _grid_share(ctxs[s], job, [audio[i] for i in shares[s]], [refs[i] for i in shares[s]], ids, stats, st,
                                       rungs, stop)
        except (threading.BrokenBarrierError, _Stopped) as e:   # another worker failed
            breaks.append(e)
        except BaseException as e:  # re-raised below, in the caller's thread
            errs.append(e)
            stop.set()
            if rungs is not None:
                rungs.barrier.abort()
        finally:
            share_times[s]["wall"] = time.perf_counter() - t0

    try:
        for c, own in zip(ctxs, owned):
            chain.apply(c, own)
        if len(workers) == 1:
            work(workers[0])
        else:
            th = [threading.Thread(target=work, args=(s,), name=f"run_grid share {s}") for s in workers]
            for t in th:
                t.start()
            for t in th:
                t.join()
    finally:
        chain.close()
        for c, own in zip(ctxs, owned):
            if own and c is not None:
                c.close()
    if errs or breaks:
        raise (errs or breaks)[0]
    times = {}
    for s in workers:
        for k, v in share_times[s]["times"].items():
            times[k] = max(times.get(k, 0), v) if k in _MAX_TIMES else times.get(k, 0.0) + v
    for k in _MAX_TIMES:
        times.setdefault(k, 0)
    n_slices = sum(share_out[s][0] for s in workers)
    bytes_per_share = [share_out[s][1] for s in range(len(shares))]
    dev_bytes = max((b for b in bytes_per_share if b is not None), default=None)
    if halving is not None:
        halving.update(survivors=rungs.alive, rung=rungs.rung_of, evaluated_seconds=rungs.evaluated.tolist(), rungs_run=rungs.log)
    aggs = [fv.stats_aggregate_array(stats[c]) for c in range(NC)]
    rows = [dict(config=c, **_agg_row(agg)) for c, agg in enumerate(aggs)]
    if sized:
        for r in rows:
            r["fft_size"] = sizes_of[r["config"]]
    if halving is not None:
        for r in rows:
            r["rung"] = halving["rung"][r["config"]]
            r["evaluated_seconds"] = halving["evaluated_seconds"][r["config"]]
    elapsed = time.perf_counter() - t_all
    if json_path:
        with open(json_path, "w") as f:
            doc = {"grid": grid, "configs": configs, "rows": rows, "avgs_form": times["avgs_form"], "avgs_bytes": times["avgs_bytes"],
                   "trigger_form": times["trigger_form"], "trigger_bytes": times["trigger_bytes"], "trigger_keys": times["trigger_keys"]}
            if halving is not None:
                doc.update(survivors=halving["survivors"], rung_times=halving["rungs_run"])
            json.dump(doc, f, indent=1)
    if out is not None:
        ranked = _ranked(rows) if halving is None else _ranked([r for r in rows if r["rung"] is None])
        if halving is None:
            out.write(f"top {min(top, NC)} of {NC} configs by F-score (β = 0.7):\n")
        else:
            out.write(f"top {min(top, len(ranked))} of {len(ranked)} surviving configs ({NC} in all, successive halving with "
                      f"eta {halving['eta']}) by F-score (β = 0.7):\n")
        out.write("| config |" + (" fft_size |" if sized else "") +
                  "      P |     TP |     FP |     FN |    TPR |    PPV |    FNR |    FDR | F-score |    FMI |\n")
        for r in ranked[:top]:
            out.write("| {:>6} |".format(r["config"]) + (" {:>8} |".format(r["fft_size"]) if sized else "") +
                      " {} | {} | {} | {} | {}% | {}% | {}% | {}% | {}% | {}% |\n".format(
                _f(r["P"], 6, 1), _f(r["TP"], 6, 1), _f(r["FP"], 6, 1), _f(r["FN"], 6, 1),
                *[_f(np.float32(r[k]) * np.float32(100), 5, 1) for k in ("TPR", "PPV", "FNR", "FDR")],
                _f(np.float32(r["F"]) * np.float32(100), 6, 1), _f(np.float32(r["FM"]) * np.float32(100), 5, 1)))
        per_share = ""
        if len(shares) > 1:   # the stage times are sums over the shares; each share's own wall time
            per_share = "; shares' wall times " + ", ".join(f"{t['wall']:.2f}" for t in share_times) + " s"
        out.write(f"[{NC} configs x {n_inst} instances in {elapsed:.2f} s: denoise {times['denoise']:.2f} s, bands "
                  f"{times['bands']:.2f} s, machines ({vad_on}) {times['machines']:.2f} s, scoring ({score_on}) "
                  f"{times['scoring']:.3f} s{per_share}]\n")
        if halving is not None:
            for g in halving["rungs_run"]:
                name = f"rung {g['rung']}" if g["rung"] is not None else "to the end"
                out.write(f"[{name} (chunk {g['end_chunk']}): {g['configs_in']} configs in, {g['configs_kept']} kept, "
                          f"{g['seconds']:.2f} s]\n")
    res = {"configs": configs, "rows": rows, "aggregates": aggs, "stats": stats, "times": times, "slices": n_slices,
           "device_bytes": dev_bytes}
    if halving is not None:
        res.update(survivors=halving["survivors"], rung=halving["rung"], evaluated_seconds=halving["evaluated_seconds"],
                   rung_times=halving["rungs_run"])
    if n_shares is not None:
        res.update(share_times=share_times, device_bytes_per_share=bytes_per_share)
    return res

class _Stopped(Exception):
    """a run_grid worker stopping because another one failed"""


def _check_stop(stop):
    if stop.is_set():
        raise _Stopped()


class _Rungs:
    """Successive halving's decisions, shared by the workers of one run_grid call (one per share of the instances, each with its
    own context and batches; a single worker on a single context).  The rungs are halving_schedule's over the longest instance
    of the whole plan.  At a rung every worker scores its own batches into the shared stats and waits at the barrier; the
    barrier's action, run by one thread once all have arrived, aggregates stats over all instances in plan order and picks the
    configs to keep.  A failing worker aborts the barrier, so that none is left waiting."""

    def __init__(self, n_workers, halving, n_chunks, slice_chunks, stats, stat_cfgs):
        self.eta = int(halving["eta"])
        self.n_chunks = n_chunks                 # every instance's, plan order
        self.K = max(n_chunks)
        self.ends = halving_schedule(self.K, slice_chunks, self.eta, int(halving["rungs"]))
        self.stats, self.stat_cfgs = stats, stat_cfgs
        NC = len(stat_cfgs)
        self.alive = list(range(NC))             # the original index of each config the batches hold
        self.rung_of = [None] * NC
        self.evaluated = np.zeros(NC)
        self.log = []
        self.keep, self.n_in = None, None        # the last rung's keep list (indices into alive as it was) and its length
        self.t_rung = time.perf_counter()
        self._step = None
        self.lock = threading.Lock()
        self.barrier = threading.Barrier(n_workers, action=lambda: self._step())

    def wait(self, step):
        """every worker passes the same step; it runs once, when the last worker arrives"""
        self._step = step
        self.barrier.wait()

    def count(self, ids, s0, s1):
        """add the seconds of audio the alive configs' machines ran over instances ids (plan indices) in slice [s0, s1)"""
        with self.lock:
            for i in ids:
                n = self.n_chunks[i]
                self.evaluated[self.alive] += (min(n, s1) - min(n, s0)) * 24000 / 48000.0

    def choose(self):
        """the ceil(n / eta) best alive configs by aggregate F-score over the prefix (ties to the lower config index)"""
        rows = [dict(config=c, F=_agg_row(fv.stats_aggregate_array(np.ascontiguousarray(self.stats[o])))["F"])
                for c, o in enumerate(self.alive)]
        n_keep = -(-len(self.alive) // self.eta)
        self.keep = sorted(r["config"] for r in _ranked(rows)[:n_keep])
        kept = set(self.keep)
        for c, o in enumerate(self.alive):
            if c not in kept:
                self.rung_of[o] = len(self.log) + 1
        self.n_in = len(self.alive)
        self.alive = [self.alive[c] for c in self.keep]

    def logged(self):
        now = time.perf_counter()
        self.log.append({"rung": len(self.log) + 1, "end_chunk": self.ends[len(self.log)], "configs_in": self.n_in,
                         "configs_kept": len(self.alive), "seconds": now - self.t_rung})
        self.t_rung = now

    def ended(self):
        self.log.append({"rung": None, "end_chunk": self.K, "configs_in": len(self.alive), "configs_kept": len(self.alive),
                         "seconds": time.perf_counter() - self.t_rung})


def _grid_share(ctx, job, audio, refs, ids, stats, times, rungs, stop):
    """run_grid's flow for one share of the instances on its own context: job the call's _SweepJob, audio / refs the share's
    instances, ids their plan indices (the columns of stats it fills); rungs a _Rungs for successive halving; stop an Event
    another worker sets when it fails.  Returns (slices run, device_bytes: None unsliced)."""
    if job.slice_chunks is not None:
        return _grid_sliced(ctx, job, audio, refs, ids, stats, times, rungs, stop)
    _grid_unsliced(ctx, job, audio, refs, ids, stats, times, stop)
    return 1, None


def _grid_unsliced(ctx, job, audio, refs, ids, stats, times, stop):
    """run_grid without slices over a share: one denoising batch of the share's instances (padded to its longest), then per
    channel-count group the band sums, the machines and the scoring (run_grid's docstring)"""
    allocs = []

    def dalloc(nbytes):
        a = ctx.device_alloc(max(int(nbytes), 16))
        allocs.append(a)
        return a

    def score(batch, insts):
        if job.score_on == "host":
            t0 = time.perf_counter()
            batch.set_references([refs[i] for i in insts], job.stat_cfgs)
            batch.score(job.n_threads)
            times["scoring"] += time.perf_counter() - t0
        for c in range(len(job.configs)):
            stats[c, ids[insts]] = batch.config_stats(c)

    try:
        t0 = time.perf_counter()
        groups, n_chunks, n_den, _, d_den, rms = _denoise_for_sweep(ctx, audio, job.F, job.configs[0], dalloc)
        times["denoise"] = time.perf_counter() - t0
        l0 = 0
        for nch, members in groups.items():
            _check_stop(stop)
            sweep = _new_batch(job, len(members), nch)
            try:
                t0 = time.perf_counter()
                g_lanes = list(range(l0, l0 + len(members) * nch))
                l0 += len(g_lanes)
                d_gband, bstride, nf = _group_band_sums(ctx, sweep, members, n_chunks, d_den + g_lanes[0] * n_den * 4, len(g_lanes),
                                                        n_den, dalloc)
                g_rms = np.ascontiguousarray(rms[g_lanes])
                times["bands"] += time.perf_counter() - t0
                if job.score_on == "device":
                    sweep.set_references([refs[i] for i in members], job.stat_cfgs)
                    sweep.keep_segments(False)
                _group_machines(ctx, job, sweep, members, nch, d_gband, bstride, nf, g_rms, n_chunks, times, score, stop)
            finally:
                sweep.close()
    finally:
        for a in allocs:
            ctx.device_free(a)


# the halo of a time slice: a slice is denoised from zero history this many chunks early (two are what NSNet2's cross-chunk state
# needs; shard.ALIGN_CHUNKS), and the halo's chunks are dropped
SLICE_HALO_CHUNKS = 16
# the engine's device intermediates per chunk of a launch (computed from shapes, not measured): features [54][176],
# spectrogram [50][161][2], gi [54][25][3][16], h1 and h2 [54][400], fc2 / fc3 outputs [50][608], gains [50][176], f32
ENGINE_WS_BYTES_PER_CHUNK = 4 * (54 * 176 + 50 * 161 * 2 + 54 * 25 * 3 * 16 + 2 * 54 * 400 + 50 * 608 + 50 * 176)
ENGINE_MAX_LAUNCH_CHUNKS = 49152


def halving_schedule(K, slice_chunks, eta, rungs):
    """The rungs of successive halving over a corpus whose longest instance is K chunks, run in slices of slice_chunks: rung k
    (k = 1 .. rungs) ends at the first slice boundary at or after K * eta^(k - 1 - rungs) chunks.  Rungs that land on the same
    boundary are merged and rungs at or past the end are skipped -> the rungs' ends in chunks, increasing.  ValueError unless
    eta >= 2 and rungs >= 1 (integers)."""
    for name, v, lo in (("eta", eta, 2), ("rungs", rungs, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError(f"halving {name} = {v!r}: an integer >= {lo}")
    ends = []
    for k in range(1, rungs + 1):
        div = int(slice_chunks) * int(eta) ** (rungs + 1 - k)
        end = -(-int(K) // div) * int(slice_chunks)   # ceil(K / eta^(rungs + 1 - k) / slice_chunks) slices
        if end < K and (not ends or end > ends[-1]):
            ends.append(end)
    return ends


def _clip_labels(ref, t):
    """labels [(from, to)] cut to [0, t) seconds: a label starting at or after t goes, one running past t ends at t"""
    a = np.asarray(ref, np.float32).reshape(-1, 2)
    a = a[a[:, 0] < np.float32(t)].copy()
    a[:, 1] = np.minimum(a[:, 1], np.float32(t))
    return a


class _DeviceParts:
    """a channel-count group's machines of a sliced grid: one device batch (b), run in parts.  sizes and blocks are the
    batch's frame sizes and size_blocks(), kept up by retain."""

    def __init__(self, ctx, job, nch, refs):
        self.ctx, self.job, self.refs = ctx, job, refs
        self.b = _new_batch(job, len(refs), nch)
        self.sizes, self.blocks = self.b.sizes, self.b.size_blocks()
        if job.score_on == "device":
            self.b.set_references(refs, job.stat_cfgs)
            self.b.keep_segments(False)

    def part(self, d_bands, stride, n_frames, rms, n_chunks, first_sample):
        """the slice from first_sample on: n_frames [size][stream] of the band sums at d_bands, chunk RMS [lanes][chunks] on the host"""
        self.b.run_device_part_sized(self.ctx, d_bands, stride, n_frames, rms, n_chunks, first_sample)

    def score(self, stats, cols, alive, refs=None):
        """everything run so far into stats[o, cols] for the batch's configs o = alive[c]: the device scorer, or with score_on
        "host" the host scorer on the segments the parts kept.  refs: labels to score against instead of the group's (a
        rung's, cut to its prefix)"""
        if refs is not None or self.job.score_on == "host":
            self.b.set_references(self.refs if refs is None else refs, [self.job.stat_cfgs[o] for o in alive])
        if self.job.score_on == "device":
            self.b.score_device(self.ctx)
        else:
            self.b.score(self.job.n_threads)
        for c, o in enumerate(alive):
            stats[o, cols] = self.b.config_stats(c)

    def retain(self, keep):
        """cut the batch to its configs keep"""
        self.b.retain(self.ctx, keep)
        self.sizes, self.blocks = self.b.sizes, self.b.size_blocks()

    def full_labels(self, alive):
        """the group's own labels back after a rung's cut ones, for the batch's configs alive"""
        self.b.set_references(self.refs, [self.job.stat_cfgs[o] for o in alive])

    def device_bytes(self):
        return self.b.device_bytes()

    def close(self):   # (closing a batch waits for its part)
        self.b.close()


class _HostParts:
    """_DeviceParts' shape for vad_on "host": one single-stream host batch per instance (instances differ in length), run on in
    parts over the slice's band sums copied back (fvad_vad_batch_run_sized).  No retain: halving needs device machines."""

    def __init__(self, ctx, job, nch, refs):
        self.ctx, self.job, self.nch, self.refs = ctx, job, nch, refs
        self.hosts = [_new_batch(job, 1, nch) for _ in refs]
        self.sizes, self.blocks = self.hosts[0].sizes, self.hosts[0].size_blocks()

    def part(self, d_bands, stride, n_frames, rms, n_chunks, first_sample):
        nch = self.nch
        n_bands = sum(len(bins) for _, _, bins in self.blocks)
        band = self.ctx.to_host(np.empty((n_bands, len(self.hosts) * nch, stride), np.float32), d_bands)
        for k, h in enumerate(self.hosts):
            nf_k = [row[k] for row in n_frames]
            if max(nf_k) == 0 and first_sample > 0:
                continue   # ended (its machines keep their results)
            h.run_sized(np.ascontiguousarray(band[:, k * nch:(k + 1) * nch, :max(max(nf_k), 1)]),
                        np.ascontiguousarray(rms[k * nch:(k + 1) * nch, :max(n_chunks[k], 1)]), nf_k, first_sample=first_sample,
                        n_threads=self.job.n_threads)

    def score(self, stats, cols, alive, refs=None):
        assert refs is None and len(alive) == len(self.job.configs)   # (rungs score device machines only)
        for k, h in enumerate(self.hosts):
            h.set_references([self.refs[k]], self.job.stat_cfgs)
            h.score(self.job.n_threads)
            for c, o in enumerate(alive):
                stats[o, cols[k]] = h.config_stats(c)[0]

    def device_bytes(self):
        return 0

    def close(self):
        for h in self.hosts:
            h.close()


def _run_slices(ctx, job, audio, refs, ids, groups, n_chunks, K, buf, stats, times, stop, ov=None, rungs=None):
    """The slice loop of a sliced grid over one share: the time slices [s0, s1) of job.slice_chunks chunks up to chunk K in
    the outer loop, the channel-count groups {n_channels: [instance]} in the inner one, every group's machines alive
    (_DeviceParts, or _HostParts with vad_on "host"); a group whose instances have all ended is skipped and not counted.  Each
    slice is read, denoised and its band sums computed (_slice_denoise_and_bands into buf, _grid_sliced's buffers), then the
    group's machines run on; an instance gets 0 frames once it has ended.  At the end every machine is scored into stats'
    columns ids[members].  Returns (slices run, the largest device memory the batches held together).
    ov (an _Overlap): the parts do not wait -- a slice's machines run beside the next slice's denoising, and every part is
    waited for before anything is scored.
    rungs (a _Rungs: successive halving, device machines and scoring; K its rungs.K, so that every rung sees every instance at
    the same point in time): at a rung's end (rungs.ends: the whole plan's) each group's machines are scored against its labels
    cut to the rung (or the instance's end); then, with every share's workers at the barrier, rungs.choose aggregates per
    config over all instances in plan order and keeps the ceil(n / eta) best by F-score (ties to the lower config index);
    every batch is cut to them (VadSweep.retain) and the full labels go back.  A share whose instances have all ended still
    scores and retains at every rung.  stats then holds the whole corpus for the survivors and, for a dropped config, the
    last prefix it was scored on; rungs holds the survivors, rung, evaluated seconds and log."""
    chunk, N = 24000, job.slice_chunks
    machines = {}
    peak, n_slices = 0, 0

    def held():
        return max(peak, sum(m.device_bytes() for m in machines.values()))

    try:
        for nch, members in groups.items():
            machines[nch] = (_DeviceParts if job.vad_on == "device" else _HostParts)(ctx, job, nch, [refs[i] for i in members])
        for s0 in range(0, K, N):
            _check_stop(stop)
            s1 = min(s0 + N, K)
            for nch, members in groups.items():
                if s0 >= max(n_chunks[i] for i in members):
                    continue   # every instance of the group has ended
                m = machines[nch]
                n_slices += 1
                dset = None if ov is None else ov.next_set()
                rms = _slice_denoise_and_bands(ctx, audio, members, nch, s0, s1, buf, m.blocks, times,
                                               None if ov is None else ov.sets[dset])
                nc = [max(0, min(n_chunks[i], s1) - s0) for i in members]
                # each size's frames of the slice, per instance
                nf = [[max(0, min(n_chunks[i] * chunk // Fg, s1 * chunk // Fg) - s0 * chunk // Fg) for i in members] for Fg in m.sizes]
                if ov is not None:
                    ov.launch(dset, m.b, buf.fr_slice, nf, rms, nc, s0 * chunk)
                    continue
                t0 = time.perf_counter()
                m.part(buf.d["bands"], buf.fr_slice, nf, rms, nc, s0 * chunk)
                times["machines"] += time.perf_counter() - t0
                if job.vad_on == "device":
                    _note_avgs(times, m.b)
            peak = held()
            if rungs is None:
                continue
            rungs.count(ids, s0, s1)
            if s1 not in rungs.ends:
                continue
            if ov is not None:
                ov.drain()
                peak = held()
            # ---- a rung: score the prefix [0, s1) against the labels cut to it, keep the best 1 / eta
            t0 = time.perf_counter()
            t_end = s1 * chunk / 48000.0
            for nch, members in groups.items():
                machines[nch].score(stats, ids[members], rungs.alive,
                                    [_clip_labels(refs[i], min(t_end, n_chunks[i] * chunk / 48000.0)) for i in members])
            times["scoring"] += time.perf_counter() - t0
            rungs.wait(rungs.choose)
            t0 = time.perf_counter()
            for m in machines.values():
                m.retain(rungs.keep)
            times["retain"] = times.get("retain", 0.0) + time.perf_counter() - t0
            for m in machines.values():
                m.full_labels(rungs.alive)
            rungs.wait(rungs.logged)
        # ---- scoring: everything run (with halving: the survivors over the whole corpus)
        if ov is not None:
            ov.drain()
            peak = held()
        t0 = time.perf_counter()
        for nch, members in groups.items():
            machines[nch].score(stats, ids[members], range(len(job.configs)) if rungs is None else rungs.alive)
        times["scoring"] += time.perf_counter() - t0
        if rungs is not None:
            rungs.wait(rungs.ended)
    finally:
        for m in machines.values():
            m.close()
    return n_slices, peak


# a sliced share's buffers, allocated once for its largest group and reused slice after slice: d {name: device address}, host
# (the slice's PCM, pinned), opts (the engine's), fr_slice (the band sums' stride: a full slice's frames at the smallest size)
_SliceBufs = collections.namedtuple("_SliceBufs", "d host opts fr_slice")


def _slice_denoise_and_bands(ctx, audio, members, nch, s0, s1, buf, blocks, times, dset=None):
    """one time slice [s0, s1) of a channel-count group (_run_slices): the slice and its SLICE_HALO_CHUNKS-chunk halo read
    from the mapped files into the pinned host buffer, denoised from zero history, the band sums of the slice's frames for
    blocks [(F, first band, bins)] written to d["bands"] (stride fr_slice); returns the slice's chunk RMS [lanes][s1 - s0].
    dset (overlap: a (bands, rms) pair of device buffers): the band sums and the RMS go there and nothing comes back to the
    host -- returns (device address of the slice's first chunk's RMS, its lane stride); the calls wait for the context's main
    stream only, never for a device part in flight."""
    chunk = 24000
    d, host, opts, fr_slice = buf
    start = max(s0 - SLICE_HALO_CHUNKS, 0)
    n = s1 - start
    L = len(members) * nch
    # ---- read and denoise [start, s1): lane l of the group at host[l * n * chunk]
    t0 = time.perf_counter()
    d_bands, d_rms = (d["bands"], d["rms"]) if dset is None else dset
    if _is_raw(audio):   # ingest "device": one source per member -- the slice and its halo, then zeros to the slice's end; waits for the main stream only
        rows = [audio[i].source(start * chunk, min(s1 * chunk, audio[i].n_frames), k * nch, 0, n * chunk) for k, i in enumerate(members)]
        _ingest_rows(ctx, [audio[i] for i in members], rows, d_lanes=d["pcm"], n_lanes=L, lane_stride=n * chunk, n_samples=n * chunk)
    else:
        pcm = host[:L * n * chunk].reshape(L, n * chunk)
        for k, i in enumerate(members):
            a = audio[i]
            lo, hi = start * chunk, min(s1 * chunk, a.shape[0])
            for c in range(nch):
                row = pcm[k * nch + c]
                if hi > lo:
                    if a.dtype == np.int16:   # the kernel's PCM16 decode, exact in f32
                        np.multiply(a[lo:hi, c], np.float32(1.0 / 32768.0), out=row[:hi - lo], casting="unsafe")
                    else:
                        row[:hi - lo] = a[lo:hi, c]
                row[max(hi - lo, 0):] = 0.0
        if dset is None:
            ctx.to_device(d["pcm"], pcm)
        else:   # queued in front of the engine call, which waits for the main stream (Context.synchronize would wait for the part too)
            ctx._ck(fv.lib().fvad_ctx_copy_to_device(ctx.h, fv.vp(d["pcm"]), pcm.ctypes.data, pcm.nbytes), "fvad_ctx_copy_to_device")
    ctx._ck(fv.lib().fvad_engine_enqueue_device(ctx.h, fv.vp(d["pcm"]), L, n * chunk, n * chunk, fv.vp(d["den"]),
                                                fv.vp(d["band0"]), fv.vp(d_rms), fv.C.byref(opts)),
            "fvad_engine_enqueue_device")
    if dset is None:
        rms = ctx.to_host(np.empty((L, n), np.float32), d["rms"])
        rms = np.ascontiguousarray(rms[:, s0 - start:])
    else:
        rms = (d_rms + (s0 - start) * 4, n)
    times["denoise"] += time.perf_counter() - t0
    # ---- band sums of the slice's frames: the denoised audio from chunk s0 on (frame-aligned: s0 is a
    # multiple of slice_align(F))
    t0 = time.perf_counter()
    for Fg, j0, bins_g in blocks:
        ctx.band_sums_device(d["den"] + (s0 - start) * chunk * 4, L, n * chunk, (s1 - s0) * chunk, bins_g,
                             d_bands + j0 * L * fr_slice * 4, fr_slice, fft_size=Fg)
    times["bands"] += time.perf_counter() - t0
    return rms


class _Overlap:
    """run_grid(overlap=True): the two sets of the per-slice buffers the machines read (bands, rms), used alternately, and the
    device parts in flight on them (fvad_vad_batch_run_device_part_async).  A set is written again only after the part that reads
    it has been waited for, and a batch has one part in flight at most."""

    def __init__(self, ctx, d, times):
        self.ctx, self.times = ctx, times
        self.sets = [(d["bands"], d["rms"]), (d["bands2"], d["rms2"])]
        self.busy = [None, None]   # the batch whose part reads the set
        self.turn = 0
        times.setdefault("machines_wait", 0.0)

    def _wait(self, i):
        b, self.busy[i] = self.busy[i], None
        if b is not None:
            t0 = time.perf_counter()
            b.part_wait(self.ctx)
            dt = time.perf_counter() - t0
            self.times["machines_wait"] += dt
            self.times["machines"] += dt
            _note_avgs(self.times, b)

    def next_set(self):
        """the buffer set of the next slice, free to be written"""
        i = self.turn % 2
        self.turn += 1
        self._wait(i)
        return i

    def launch(self, i, b, band_stride, n_frames, rms, n_chunks, first_sample):
        """b's part on set i (rms: _slice_denoise_and_bands' device address and stride), after b's previous part"""
        for j in (0, 1):
            if self.busy[j] is b:
                self._wait(j)
        t0 = time.perf_counter()
        b.run_device_part_async(self.ctx, self.sets[i][0], band_stride, n_frames, rms[0], rms[1], n_chunks, first_sample)
        self.times["machines"] += time.perf_counter() - t0
        self.busy[i] = b

    def drain(self):
        for j in (0, 1):
            self._wait(j)


def _grid_sliced(ctx, job, audio, refs, ids, stats, times, rungs, stop):
    """run_grid's pipeline in time slices of job.slice_chunks chunks over a share: each slice [s0, s1) and its
    SLICE_HALO_CHUNKS-chunk halo are read from the mapped files (audio[i]: [n_frames][n_channels]), denoised from zero history
    (fvad_engine_enqueue_device over [s0 - halo, s1), as shard.run_sliced_with_vad does), the band sums of the slice's frames
    computed from the denoised audio at chunk s0 (one fvad_engine_band_sums_device pass per frame size), and the machines run
    on in parts from sample s0 * chunk (_run_slices).  A plain grid runs one channel-count group after the other, each to its
    own longest instance, so that one batch is alive at a time; with successive halving (rungs) the slices run across all
    groups, every group's batch alive.  The device buffers are allocated once, for the largest group, and reused slice after
    slice.  Fills stats [config][instance][11] (the columns ids: the instances' plan indices) and times; returns (slices run,
    device_bytes as run_grid describes it).  stop: checked before every slice (_Stopped once another worker has failed).
    job.overlap (device machines and scoring): a second set of the bands and rms buffers, the frame ratios computed on the
    device and the parts not waited for (fvad_vad_batch_run_device_part_async): slice k's machines run beside slice k + 1's
    reading and denoising; times gains machines_wait, the host time spent waiting for parts (it is part of machines)."""
    chunk, H, N, F = 24000, SLICE_HALO_CHUNKS, job.slice_chunks, job.F
    n_chunks = [_dims(a, mapped=True)[1] // chunk for a in audio]
    groups = {}
    for i, a in enumerate(audio):
        groups.setdefault(_dims(a, mapped=True)[0], []).append(i)
    probe = _new_batch(job, 1, 1)
    n_bands, f_min = len(probe.size_of_band), min(probe.sizes)
    probe.close()
    opts = _engine_opts(job.configs[0], F)             # (config 0's band is unused: the bands come from K4)
    n_max = N + H                                      # chunks of a slice with its halo
    lanes_max = max([len(m) * nch for nch, m in groups.items()] + [1])
    fr_slice = N * chunk // f_min                      # frames of a full slice at the smallest size (N * chunk is a multiple of each)
    own = {"pcm": lanes_max * n_max * chunk * 4, "den": lanes_max * n_max * chunk * 4,
           "band0": lanes_max * (n_max * chunk // F + 1) * 4, "rms": lanes_max * n_max * 4,
           "bands": n_bands * lanes_max * fr_slice * 4}
    if job.overlap:
        own.update(bands2=own["bands"], rms2=own["rms"])
    d = {}
    host = None
    n_slices, batch_peak = 0, 0
    ws = ENGINE_WS_BYTES_PER_CHUNK * min(lanes_max * n_max, ENGINE_MAX_LAUNCH_CHUNKS)
    try:
        for k, nb in own.items():
            d[k] = ctx.device_alloc(max(nb, 16))
        if not _is_raw(audio):   # (ingest "device" stages through the context's own ring)
            host = ctx.host_alloc(lanes_max * n_max * chunk)   # the slice's PCM, pinned
        buf = _SliceBufs(d, host, opts, fr_slice)
        ov = _Overlap(ctx, d, times) if job.overlap else None
        # halving: every group in one loop to the plan's end; plain: a loop per group to the group's own end
        runs = [(groups, rungs.K)] if rungs is not None else [({nch: m}, max(n_chunks[i] for i in m)) for nch, m in groups.items()]
        for run_groups, K in runs:
            n, peak = _run_slices(ctx, job, audio, refs, ids, run_groups, n_chunks, K, buf, stats, times, stop, ov, rungs)
            n_slices, batch_peak = n_slices + n, max(batch_peak, peak)
    finally:
        for a in d.values():
            ctx.device_free(a)
        if host is not None:
            ctx.host_free(host)
    return n_slices, sum(own.values()) + batch_peak + ws


def frame_ratios(chunk_rms, n_frames, fft_size=1024, chunk=24000):
    """Per-frame volume_ratio exactly as the metadata flows through the three buffered stages
    (BufferedVolumeAnalyzer.zig:33-45 -> BufferedDenoiser.zig:83-86,115 -> BufferedFFT.zig:137-140,153):
    all f32, weights are sample counts."""
    rms = np.asarray(chunk_rms, np.float32)
    vmin = np.minimum(np.float32(1), rms.min(axis=1))
    vmax = np.maximum(np.float32(0), rms.max(axis=1))
    ratio = np.where(vmax == 0, np.float32(0), vmin / np.where(vmax == 0, np.float32(1), vmax)).astype(np.float32)
    w = np.float32(chunk)
    r2 = ((ratio * w) / w).astype(np.float32)     # analyzer stage
    r2 = ((r2 * w) / w).astype(np.float32)        # denoiser stage
    out = np.empty(n_frames, np.float32)
    for k in range(n_frames):
        # every chunk the frame overlaps, in order, weighted by the samples it gives the frame (a frame longer than a chunk
        # spans three or more)
        lo, hi = k * fft_size, (k + 1) * fft_size
        s, n = np.float32(0), np.float32(0)
        for c in range(lo // chunk, (hi - 1) // chunk + 1):
            w = np.float32(min(hi, (c + 1) * chunk) - max(lo, c * chunk))
            s = np.float32(s + r2[c] * w)
            n = np.float32(n + w)
        out[k] = s / n
    return out


def arg_parser():
    ap = argparse.ArgumentParser(description="Formula-VAD simulator harness on MI355X")
    ap.add_argument("-i", "--input", required=True, help="Simulation plan (path to JSON)")  # simulator.zig:78-82
    ap.add_argument("--synth-seed", type=int, default=None, help="use random-init NSNet2 weights")
    ap.add_argument("--devices", default=None, help="comma-separated HIP devices (default 0): one context + one thread each, "
                                                    "instances dealt round-robin (e.g. 0,1,2,3,4,5,6,7); for a plan run and "
                                                    "--sweep-grid")
    ap.add_argument("--sweep", action="store_true", help="score the plan's vad_machine_config and alt_vad_machine_configs over one "
                                                         "denoising pass: one table row per config (device 0)")
    ap.add_argument("--sweep-json", default=None, help="with --sweep: write the rows and segments to this JSON file; "
                                                       "with --sweep-grid: the configs and all rows")
    ap.add_argument("--sweep-vad", default="auto", choices=("auto", "device", "host"),
                    help="with --sweep / --sweep-grid: where the VAD machines run (auto: the GPU from %d configs on)" % SWEEP_DEVICE_MIN_CONFIGS)
    ap.add_argument("--sweep-grid", default=None, help="score every config of a grid file ({\"base\": {...}, \"axes\": {field: "
                                                          "[values]}}, optionally \"fft_size\": [sizes]) over one denoising pass; "
                                                          "print the top configs (on --devices, default device 0)")
    ap.add_argument("--top", type=int, default=20, help="with --sweep-grid: rows to print (by F-score)")
    ap.add_argument("--slice-chunks", type=int, default=None,
                    help="with --sweep-grid, --export-clips or --export-denoised: run in time slices of N chunks (a multiple of 16 at fft_size 1024; with several "
                         "sizes, of the lcm over them), device and host "
                         "memory bounded by the slice instead of the corpus")
    ap.add_argument("--halving-eta", type=int, default=None,
                    help="with --sweep-grid and --slice-chunks: successive halving, keeping the best 1/ETA of the configs at each "
                         "rung (the machines and scoring on the GPU)")
    ap.add_argument("--halving-rungs", type=int, default=None,
                    help="with --halving-eta: the number of rungs R (rung k ends at ETA^(k-1-R) of the corpus)")
    ap.add_argument("--vad-chain", default=None, choices=VAD_CHAINS,
                    help="with --sweep / --sweep-grid: how the device VAD machines run their exact long-term chains (context option "
                         "vad_chain): lane by lane (the default) or by the whole wavefront; same results")
    ap.add_argument("--vad-avgs", default=None, choices=VAD_AVGS,
                    help="with --sweep / --sweep-grid and --vad-chain coop: the device VAD machines' short-term and channel-ratio "
                         "averages from their own rings (the default) or from tables filled frame-parallel before the launch "
                         "(context option vad_avgs); same results")
    ap.add_argument("--vad-trigger", default=None, choices=VAD_TRIGGERS,
                    help="with --sweep / --sweep-grid and --vad-chain coop: one device VAD machine per config (the default) or one "
                         "trigger machine per distinct trigger and a finishing kernel per config (context option vad_trigger); "
                         "same results")
    ap.add_argument("--export-clips", default=None, metavar="DIR",
                    help="run the plan and write every completed segment's original and denoised clip (the quietest channel, cut and "
                         "picked on the GPU) and a NAME-clips.json manifest per instance into DIR")
    ap.add_argument("--clips-pcm16", action="store_true", help="with --export-clips: the clips as PCM16 (half the bytes over PCIe)")
    ap.add_argument("--clips-denoised-rate", type=int, default=48000, metavar="HZ",
                    help="with --export-clips: 48000 or 16000 -- at 16000 the denoised clips are NSNet2's own 16 kHz output (every third "
                         "sample, the ones K3's interpolator did not make up): a third of the bytes, nothing lost")
    ap.add_argument("--clips-original-rate", type=int, default=48000, metavar="HZ",
                    help="with --export-clips: 48000 or 16000 -- at 16000 the original clips are decimated as NSNet2's input is "
                         "(every third sample, no anti-alias filter: it aliases)")
    ap.add_argument("--clips-original-filter", default="none", choices=CLIP_FILTERS,
                    help="with --export-clips: fir -- the original clips are low-pass filtered while they are decimated (a Kaiser-windowed "
                         "sinc of 32 step + 1 taps on the GPU); --clips-original-rate may then be 24000, 16000 or 8000.  resample -- the "
                         "clips are resampled on the GPU (a polyphase Kaiser-windowed sinc): --clips-original-rate may then be any other "
                         "rate whose ratio to 48000 has up <= 640, such as 44100, 32000, 22050 or 11025")
    ap.add_argument("--clips-denoised-filter", default="none", choices=CLIP_FILTERS,
                    help="with --export-clips: fir -- the same for the denoised clips (at 16000 they need no filter: use it for 24000 or 8000); "
                         "resample -- the same for the denoised clips")
    ap.add_argument("--clips-features", default=None, metavar="KIND",
                    help="with --export-clips: logmel -- also write every denoised clip's log-mel features, computed on the GPU from the "
                         "network's own 16 kHz samples (400-point Hann, hop 160, 80 Slaney bands, log10), as NAME-####-denoised.logmel.npy; "
                         "fbank -- Kaldi's filter-bank features of the same samples (frames of 400 every 160, DC removed, pre-emphasis 0.97, "
                         "Povey window, 512-point transform, 80 HTK-mel bands from 20 Hz, ln), as NAME-####-denoised.fbank.npy; "
                         "with --slice-chunks only together with --clips-features-sliced")
    ap.add_argument("--clips-features-sliced", action="store_true",
                    help="with --clips-features and --slice-chunks: write the features from the sliced run too (the split-source feature "
                         "export, one call per slice); the same files and manifests as without --slice-chunks")
    ap.add_argument("--clips-features-norm", default=None, metavar="NORM",
                    help="with --clips-features logmel: whisper -- (max(x, max - 8) + 4) / 4, the maximum taken per clip; "
                         "with --clips-features fbank: cmn -- the clip's mean per band subtracted")
    ap.add_argument("--overlap", action="store_true",
                    help="with --sweep-grid and --slice-chunks (device machines and scoring): run each slice's machines beside the "
                         "next slice's denoising (a second stream and a second set of band buffers)")
    ap.add_argument("--export-denoised", default=None, metavar="DIR",
                    help="write every instance's denoised recording to DIR as NAME-denoised.wav (all its channels at 48 kHz, whole "
                         "chunks), converted and interleaved on the GPU (fvad_egress); not with --sweep, --sweep-grid or --export-clips; "
                         "takes --slice-chunks, --ingest and --devices")
    ap.add_argument("--denoised-format", default=None, choices=tuple(DENOISED_FORMATS),
                    help="with --export-denoised: pcm16 (the default), pcm24 or f32")
    ap.add_argument("--denoised-rate", default=None, metavar="R|source",
                    help="with --export-denoised: write the recordings at R Hz instead of 48000 (44100, 32000, 22050, 16000 ...: any rate "
                         "whose ratio to 48000 has up <= 640), or with `source` each at its own file's rate (known with --ingest device); "
                         "resampled on the GPU in front of the conversion (fvad_egress_resample)")
    ap.add_argument("--denoised-source", default=None, choices=DENOISED_SOURCES,
                    help="with --export-denoised: lanes (the default: the 48 kHz lanes, NSNet2's output linearly interpolated) or network "
                         "(NSNet2's own 16 kHz samples, every third lane sample: lossless at --denoised-rate 16000, band-limited "
                         "interpolation instead of the lerp at 48000, one filter at any other rate; fvad_egress_resample_strided)")
    ap.add_argument("--denoised-kinds", default=None, metavar="K[,K...]",
                    help="with --export-denoised: the files to write per instance, NAME-K.wav each, of denoised, original (the input "
                         "delayed by the denoiser's 482 samples, so that it lines up with the denoised file), residual (what the denoiser "
                         "took out: that original minus the denoised) and mix (see --denoised-mix); weighted and summed on the GPU in "
                         "front of the conversion (fvad_egress_mix); all but denoised at 48000 Hz only")
    ap.add_argument("--denoised-mix", default=None, type=float, metavar="W",
                    help="with --denoised-kinds ...,mix: W of the denoised and 1 - W of the aligned original, 0 < W < 1")
    ap.add_argument("--ingest", default="host", choices=INGESTS,
                    help="with --sweep / --sweep-grid / --export-clips / --export-denoised: where the files' samples are de-interleaved and decoded -- on "
                         "the host, uploaded as f32 (the default), or on the GPU from the files' own bytes (fvad_ingest: PCM16 crosses "
                         "PCIe at 2 bytes per sample, and 24-bit PCM files are taken); same results.  Files at other rates than 48 kHz "
                         "(44.1 kHz, 16 kHz ...) run with device only: they are resampled to 48 kHz while they are ingested")
    return ap


def check_modes(a):
    """--export-denoised is a mode of its own: ValueError, before any work, when it is combined with a sweep or the clip export,
    or when --denoised-format, --denoised-rate or --denoised-source comes without it"""
    if a.export_denoised:
        others = [name for name, on in (("--sweep", a.sweep), ("--sweep-grid", a.sweep_grid), ("--export-clips", a.export_clips)) if on]
        if others:
            raise ValueError(f"--export-denoised cannot be combined with {', '.join(others)} (one pass writes one kind of output)")
    elif a.denoised_format is not None:
        raise ValueError("--denoised-format needs --export-denoised")
    elif a.denoised_rate is not None:
        raise ValueError("--denoised-rate needs --export-denoised")
    elif a.denoised_source is not None:
        raise ValueError("--denoised-source needs --export-denoised")
    elif a.denoised_kinds is not None:
        raise ValueError("--denoised-kinds needs --export-denoised")
    elif a.denoised_mix is not None:
        raise ValueError("--denoised-mix needs --export-denoised")


def _parse_denoised_rate(text):
    """--denoised-rate's value: None, "source" or an integer (anything else: ValueError, as run_denoise says it)"""
    if text is None or text == "source":
        return text
    try:
        return int(text)
    except ValueError:
        raise ValueError(f"--denoised-rate {text!r}: a sample rate or `source`") from None


def main(argv=None):
    a = arg_parser().parse_args(argv)
    check_modes(a)
    if (a.clips_features is not None or a.clips_features_norm is not None or a.clips_features_sliced) and not a.export_clips:
        raise ValueError("--clips-features, --clips-features-norm and --clips-features-sliced need --export-clips")
    _check_features(a.clips_features, a.clips_features_norm, a.slice_chunks, a.clips_features_sliced)
    devices = None if a.devices is None else [int(d) for d in a.devices.split(",") if d != ""]
    if a.export_denoised:
        kinds = None if a.denoised_kinds is None else tuple(k for k in a.denoised_kinds.split(",") if k != "")
        for m in run_denoise(a.input, a.export_denoised, fmt=a.denoised_format or "pcm16", synth_seed=a.synth_seed, devices=devices,
                             ingest=a.ingest, slice_chunks=a.slice_chunks, rate=_parse_denoised_rate(a.denoised_rate), kinds=kinds,
                             mix=a.denoised_mix, source=a.denoised_source or "lanes"):
            for e in [m] if kinds is None else m["kinds"]:
                at = "" if e["sample_rate"] == 48000 else f" at {e['sample_rate']} Hz"
                sys.stdout.write(f"{e['file']}: {e['channels']} x {e['frames']} frames, {e['format']}{at}\n")
        return
    if a.sweep_grid:
        run_grid(a.input, a.sweep_grid, top=a.top, vad_on=a.sweep_vad, json_path=a.sweep_json, synth_seed=a.synth_seed,
                 slice_chunks=a.slice_chunks, halving_eta=a.halving_eta, halving_rungs=a.halving_rungs, devices=devices,
                 overlap=a.overlap, vad_chain=a.vad_chain, vad_avgs=a.vad_avgs, vad_trigger=a.vad_trigger, ingest=a.ingest)
        return
    if a.export_clips:
        info = {}
        text, _ = run_clips(a.input, a.export_clips, pcm16=a.clips_pcm16, synth_seed=a.synth_seed, devices=devices, ingest=a.ingest,
                            slice_chunks=a.slice_chunks, info=info, denoised_rate=a.clips_denoised_rate, original_rate=a.clips_original_rate,
                            original_filter=a.clips_original_filter, denoised_filter=a.clips_denoised_filter, features=a.clips_features,
                            features_norm=a.clips_features_norm, features_sliced=a.clips_features_sliced)
        sys.stdout.write(text)
        if info:
            sys.stdout.write(f"\n[{info['slices']} slices; held tails: {info['held_peak_bytes'] / 2 ** 20:.1f} MiB of device memory at most]\n")
        return
    if a.sweep:
        run_sweep(a.input, synth_seed=a.synth_seed, json_path=a.sweep_json, vad_on=a.sweep_vad, vad_chain=a.vad_chain, vad_avgs=a.vad_avgs,
                  vad_trigger=a.vad_trigger, ingest=a.ingest)
        return
    run_plan(a.input, synth_seed=a.synth_seed, devices=devices or [0])


if __name__ == "__main__":
    main()
