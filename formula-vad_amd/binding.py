"""ctypes binding of libfvad_hip.so (include/fvad.h).

Plumbing only: the arithmetic lives in the HIP kernels and the C++ host code behind the C ABI.
There is NO fallback: if the shared library is missing this module raises, and every GPU entry
point returns FVAD_ERR_NO_DEVICE (-101) when no gfx950 device is present.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FVAD_LIB_PATH") or os.path.join(_HERE, "libfvad_hip.so")  # the env override is a tuning aid (A/B builds)

c_float_p = C.POINTER(C.c_float)
vp = C.c_void_p
sz = C.c_size_t

FVAD_OK = 0
FVAD_ERR_NO_DEVICE = -101
FVAD_ERR_INVALID_ARGUMENT = -100
FVAD_ERR_OUT_OF_RANGE = -6
FVAD_ERR_NEGATIVE_FREQUENCY = -7
FVAD_ERR_BUFFER_TOO_SMALL = -106
FVAD_ERR_MODEL_FORMAT = -104
FVAD_ERR_NOT_AVAILABLE = -107
CLIP_F32, CLIP_PCM16 = 0, 1      # sample formats of fvad_clips_*
CLIP_FIELDS = 4                  # a clip: first_lane, n_channels, sample_from, sample_to (uint64 each)
CLIP_SPLIT_FIELDS = 7            # a split clip: n_channels, a_lane, a_from, a_len, b_lane, b_from, b_len (uint64 each)
CLIP_STEP_MAX = 16               # the largest step of the strided clip exports
CLIP_FIR_TAPS_MAX = 513          # the most taps of the filtered clip exports
CLIP_MEL_NFFT_MAX = 2048         # the largest n_fft of the log-mel clip exports
CLIP_MEL_BANDS_MAX = 128         # the most mel bands of the log-mel clip exports
FLT_EPSILON = float(2.0 ** -23)  # Kaldi's floor of a filter-bank energy
INGEST_F32, INGEST_PCM16, INGEST_PCM24 = 0, 1, 2   # source formats of fvad_ingest* (the first two are CLIP_*'s values)
INGEST_FIELDS = 7                # a source: byte_offset, n_frames, n_channels, format, first_lane, dst_offset, fill_to (uint64 each)
WAV_INFO_FIELDS = 6              # fvad_wav_probe: format, n_channels, sample_rate, data_offset, n_frames, bits
INGEST_SAMPLE_BYTES = {INGEST_F32: 4, INGEST_PCM16: 2, INGEST_PCM24: 3}
INGEST_TILE_BYTES = 16384        # kIngestTileBytes (csrc/kernels.h): the source bytes a workgroup of the ingest kernel takes
RESAMPLE_FIELDS = 11             # a resample source: INGEST_FIELDS' seven (n_frames: the frames given), then frame_base, file_frames, out_from, n_out
RESAMPLE_UP_MAX = 640            # FVAD_RESAMPLE_UP_MAX
RESAMPLE_TAPS_MAX = 20481        # FVAD_RESAMPLE_TAPS_MAX (= 2 * 16 * 640 + 1)
EGRESS_FIELDS = 6                # a sink: byte_offset, n_frames, n_channels, format (the file's), first_lane, src_offset (uint64 each)
EGRESS_STEP_MAX = 16             # the largest src_step of the strided resampling egress
EGRESS_RESAMPLE_FIELDS = 10      # a resampled sink: byte_offset, n_out, n_channels, format, first_lane, src_offset, frame_base, n_frames, stream_frames, out_from
EGRESS_MIX_FIELDS = 8            # a two-source sink: EGRESS_FIELDS' six (src_offset: into the denoised lanes), then orig_offset, orig_zeros
WAV_HEADER_BYTES = 44            # FVAD_WAV_HEADER_BYTES: fvad_wav_header's canonical header
INGEST_FILL_TILE = 8192          # kIngestFillTile: the zeros of one lane a workgroup writes
NN_TAP_LAYERS = {"h1": 0, "h2": 1, "f2": 2, "f3": 3, "gains": 4}


class FvadError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        name = lib().fvad_status_name(status).decode()
        super().__init__(f"{where}: error.{name} ({status}) {detail}".strip())


class Complex(C.Structure):
    _fields_ = [("r", C.c_float), ("i", C.c_float)]


class Weights(C.Structure):
    _fields_ = [("n_bins", C.c_int32), ("n_fc1", C.c_int32), ("n_hidden", C.c_int32),
                ("n_fc2", C.c_int32), ("n_fc3", C.c_int32)] + [
        (n, c_float_p) for n in (
            "fc1_w", "fc1_b", "gru1_w", "gru1_r", "gru1_b", "gru2_w", "gru2_r", "gru2_b",
            "fc2_w", "fc2_b", "fc3_w", "fc3_b", "fc4_w", "fc4_b")]


WEIGHT_NAMES = ("fc1_w", "fc1_b", "gru1_w", "gru1_r", "gru1_b", "gru2_w", "gru2_r", "gru2_b",
                "fc2_w", "fc2_b", "fc3_w", "fc3_b", "fc4_w", "fc4_b")


def weight_shapes(nb, f1, h, f2, f3):
    return {"fc1_w": (f1, nb), "fc1_b": (f1,),
            "gru1_w": (3 * h, f1), "gru1_r": (3 * h, h), "gru1_b": (6 * h,),
            "gru2_w": (3 * h, h), "gru2_r": (3 * h, h), "gru2_b": (6 * h,),
            "fc2_w": (f2, h), "fc2_b": (f2,), "fc3_w": (f3, f2), "fc3_b": (f3,),
            "fc4_w": (nb, f3), "fc4_b": (nb,)}


class VadConfig(C.Structure):
    _fields_ = [("speech_min_freq", C.c_float), ("speech_max_freq", C.c_float),
                ("long_term_speech_avg_sec", C.c_float),
                ("has_initial_long_term_avg", C.c_int32),
                ("initial_long_term_avg", C.c_double),
                ("short_term_speech_avg_sec", C.c_float),
                ("speech_threshold_factor", C.c_float),
                ("channel_vol_ratio_avg_sec", C.c_float),
                ("channel_vol_ratio_threshold", C.c_float),
                ("min_consecutive_sec_to_open", C.c_float),
                ("max_speech_gap_sec", C.c_float),
                ("min_vad_duration_sec", C.c_float)]


class SpeechSegment(C.Structure):
    _fields_ = [("sample_from", C.c_uint64), ("sample_to", C.c_uint64),
                ("avg_channel_vol_ratio", C.c_float), ("vad_met_sec", C.c_float)]


class VadResult(C.Structure):
    _fields_ = [("recording_state", C.c_int32), ("sample_number", C.c_uint64)]


class VadAudit(C.Structure):
    _fields_ = [("min_rel_threshold_margin", C.c_double), ("min_abs_ratio_margin", C.c_double),
                ("n_frames", C.c_uint64)]


class Lane(C.Structure):
    _fields_ = [("pcm", c_float_p), ("n_samples", sz), ("state", vp), ("denoised", c_float_p),
                ("band_sum", c_float_p), ("band_sum_capacity", sz),
                ("chunk_rms", c_float_p), ("chunk_rms_capacity", sz),
                ("fft_bins", c_float_p), ("pcm_i16", C.POINTER(C.c_int16)), ("denoised_i16", C.POINTER(C.c_int16)),
                ("spectrogram", c_float_p), ("features", c_float_p),
                ("n_chunks", sz), ("n_fft_frames", sz), ("first_frame_index", C.c_uint64)]


class EngineOpts(C.Structure):
    _fields_ = [("on_device", C.c_int32), ("min_bin", C.c_int32), ("max_bin", C.c_int32),
                ("max_chunks_per_launch", C.c_int32), ("fft_size", C.c_int32), ("no_wait", C.c_int32),
                ("use_graph", C.c_int32)]


class AudioBuffer(C.Structure):
    _fields_ = [("channel_pcm", C.POINTER(c_float_p)), ("n_channels", sz), ("length", sz),
                ("sample_rate", sz), ("duration_seconds", C.c_float),
                ("global_start_frame_number", C.c_uint64)]


RecordingCb = C.CFUNCTYPE(None, vp, C.POINTER(AudioBuffer))


class Callbacks(C.Structure):
    _fields_ = [("ctx", vp), ("on_original_recording", RecordingCb),
                ("on_denoised_recording", RecordingCb)]


class PipelineConfig(C.Structure):
    _fields_ = [("sample_rate", sz), ("n_channels", sz), ("buffer_length", sz),
                ("skip_processing", C.c_int32), ("fft_size", sz),
                ("vad_machine_config", VadConfig),
                ("alt_vad_machine_configs", C.POINTER(VadConfig)),
                ("n_alt_vad_machine_configs", sz)]


class SingleStats(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "total_positives_sec", "true_positives_sec", "false_positives_sec", "false_negatives_sec",
        "true_positive_rate", "false_negative_rate", "false_discovery_rate", "precision",
        "fm_index", "f_score", "f_score_beta")]


class AggStat(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("overall", "min", "max", "avg")]


class AggregateStats(C.Structure):
    _fields_ = [("total_positives_sec", C.c_float), ("true_positives_sec", C.c_float),
                ("false_positives_sec", C.c_float), ("false_negatives_sec", C.c_float),
                ("true_positive_rate", AggStat), ("false_negative_rate", AggStat),
                ("false_discovery_rate", AggStat), ("precision", AggStat),
                ("fm_index", C.c_float), ("f_score", C.c_float), ("f_score_beta", C.c_float)]


class StatConfig(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("ignore_shorter_than_sec", "extrude_start",
                                         "extrude_end", "fill_gaps")]


class SegmentSec(C.Structure):
    _fields_ = [("from_sec", C.c_float), ("to_sec", C.c_float)]


# every symbol include/fvad.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "fvad_status_name": (C.c_char_p, [C.c_int]),
    "fvad_abi_version": (C.c_int, []),
    "fvad_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
    "fvad_ctx_destroy": (None, [vp]),
    "fvad_last_error": (C.c_char_p, [vp]),
    "fvad_ctx_synchronize": (C.c_int, [vp]),
    "fvad_ctx_stream": (vp, [vp]),
    "fvad_ctx_copy_to_host": (C.c_int, [vp, vp, vp, sz]),
    "fvad_load_nsnet2_onnx": (C.c_int, [vp, C.c_char_p]),
    "fvad_load_nsnet2_weights": (C.c_int, [vp, C.POINTER(Weights)]),
    "fvad_load_nsnet2_synth": (C.c_int, [vp, C.c_uint64]),
    "fvad_get_nsnet2_weights": (C.c_int, [vp, C.POINTER(Weights)]),
    "fvad_onnx_read_nsnet2": (C.c_int, [C.c_char_p, C.POINTER(Weights), C.POINTER(vp)]),
    "fvad_synth_nsnet2": (C.c_int, [C.c_uint64, C.POINTER(Weights), C.POINTER(vp)]),
    "fvad_weights_free": (None, [vp]),
    "fvad_fft_create": (C.c_int, [vp, sz, sz, C.c_int, C.POINTER(vp)]),
    "fvad_fft_destroy": (None, [vp]),
    "fvad_fft_forward": (C.c_int, [vp, c_float_p, sz, c_float_p, sz, c_float_p, sz,
                                   C.POINTER(Complex), sz]),
    "fvad_fft_inverse": (C.c_int, [vp, C.POINTER(Complex), sz, c_float_p, sz]),
    "fvad_fft_bin_count": (sz, [vp]),
    "fvad_fft_bin_width": (C.c_float, [vp]),
    "fvad_fft_nyquist_freq": (C.c_float, [vp]),
    "fvad_fft_freq_to_bin": (C.c_int, [vp, C.c_float, C.POINTER(sz)]),
    "fvad_fft_bin_to_freq": (C.c_int, [vp, sz, c_float_p]),
    "fvad_fft_forward_batch": (C.c_int, [vp, vp, sz, vp, vp, vp, C.c_int]),
    "fvad_hann_window_periodic": (None, [c_float_p, sz]),
    "fvad_hann_window_symmetric": (None, [c_float_p, sz]),
    "fvad_window_norm_factor": (C.c_float, [c_float_p, sz]),
    "fvad_nsnet2_window": (None, [c_float_p]),
    "fvad_nsnet2_create": (C.c_int, [vp, sz, C.POINTER(vp)]),
    "fvad_nsnet2_destroy": (None, [vp]),
    "fvad_nsnet2_chunk_size": (sz, [sz]),
    "fvad_nsnet2_delay": (C.c_int, [sz, C.POINTER(C.c_uint64)]),
    "fvad_nsnet2_denoise": (C.c_int, [vp, c_float_p, sz, c_float_p, sz, c_float_p, sz]),
    "fvad_lane_state_create": (C.c_int, [vp, C.POINTER(vp)]),
    "fvad_lane_state_reset": (None, [vp]),
    "fvad_lane_state_destroy": (None, [vp]),
    "fvad_lane_state_seek": (C.c_int, [vp, C.c_uint64, sz]),
    "fvad_engine_opts_default": (None, [C.POINTER(EngineOpts)]),
    "fvad_engine_run": (C.c_int, [vp, C.POINTER(Lane), sz, C.POINTER(EngineOpts)]),
    "fvad_engine_enqueue_device": (C.c_int, [vp, vp, sz, sz, sz, vp, vp, vp,
                                             C.POINTER(EngineOpts)]),
    "fvad_engine_enqueue_device_i16": (C.c_int, [vp, vp, sz, sz, sz, vp, vp, vp, C.POINTER(EngineOpts)]),
    "fvad_engine_band_sums_device": (C.c_int, [vp, vp, sz, sz, sz, sz, C.POINTER(C.c_int32), sz, vp, sz]),
    "fvad_nsnet2_forward": (C.c_int, [vp, c_float_p, sz, sz, c_float_p]),
    "fvad_ctx_enable_timing": (C.c_int, [vp, C.c_int]),
    "fvad_ctx_set_nn_math": (C.c_int, [vp, C.c_int]),
    "fvad_ctx_nn_math_effective": (C.c_int, [vp]),
    "fvad_ctx_last_nn_path": (C.c_char_p, [vp]),
    "fvad_ctx_nn_tap": (C.c_int, [vp, C.c_int, sz, sz, c_float_p, C.POINTER(sz), C.POINTER(sz)]),
    "fvad_ctx_set_option": (C.c_int, [vp, C.c_char_p, C.c_char_p]),
    "fvad_ctx_ws_fallbacks": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "fvad_ctx_ws2_waits": (C.c_uint32, [vp, C.c_int]),
    "fvad_ctx_kernel_times": (C.c_int, [vp, C.POINTER(C.c_char_p), c_float_p, sz,
                                        C.POINTER(sz)]),
    "fvad_vad_config_default": (None, [C.POINTER(VadConfig)]),
    "fvad_vad_create": (C.c_int, [C.POINTER(VadConfig), sz, sz, sz, C.POINTER(vp)]),
    "fvad_vad_destroy": (None, [vp]),
    "fvad_vad_run": (C.c_int, [vp, C.c_uint64, c_float_p, C.c_int, C.c_float,
                               C.POINTER(VadResult)]),
    "fvad_vad_segment_count": (sz, [vp]),
    "fvad_vad_segments": (C.c_int, [vp, C.POINTER(SpeechSegment), sz, C.POINTER(sz)]),
    "fvad_host_alloc": (C.c_int, [vp, sz, C.POINTER(vp)]),
    "fvad_host_free": (None, [vp, vp]),
    "fvad_device_alloc": (C.c_int, [vp, sz, C.POINTER(vp)]),
    "fvad_device_free": (None, [vp, vp]),
    "fvad_ctx_copy_to_device": (C.c_int, [vp, vp, vp, sz]),
    "fvad_vad_audit_get": (C.c_int, [vp, C.POINTER(VadAudit)]),
    "fvad_vad_lazy_stats": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_vad_run_many": (C.c_int, [C.POINTER(vp), sz, C.POINTER(c_float_p),
                                    C.POINTER(c_float_p), C.POINTER(sz), sz,
                                    C.POINTER(C.c_uint64), sz, C.c_int]),
    "fvad_vad_batch_create": (C.c_int, [C.POINTER(VadConfig), sz, sz, sz, sz, C.POINTER(vp)]),
    "fvad_vad_batch_destroy": (None, [vp]),
    "fvad_vad_batch_run": (C.c_int, [vp, c_float_p, sz, sz, c_float_p, sz, sz, sz, C.c_int]),
    "fvad_vad_batch_run_part": (C.c_int, [vp, c_float_p, sz, sz, c_float_p, sz, sz, sz, C.c_uint64, C.c_int]),
    "fvad_vad_batch_total_segments": (sz, [vp]),
    "fvad_vad_batch_segments": (C.c_int, [vp, C.POINTER(SpeechSegment), sz, C.POINTER(sz)]),
    "fvad_vad_batch_audit": (C.c_int, [vp, sz, C.POINTER(VadAudit)]),
    "fvad_vad_batch_create_sweep": (C.c_int, [C.POINTER(VadConfig), sz, sz, sz, sz, sz, C.POINTER(vp)]),
    "fvad_vad_batch_n_configs": (sz, [vp]),
    "fvad_vad_batch_bands": (C.c_int, [vp, C.POINTER(C.c_int32), sz, C.POINTER(sz), C.POINTER(C.c_uint32)]),
    "fvad_vad_batch_config_segments": (C.c_int, [vp, sz, C.POINTER(SpeechSegment), sz, C.POINTER(sz)]),
    "fvad_vad_batch_config_audit": (C.c_int, [vp, sz, sz, C.POINTER(VadAudit)]),
    "fvad_vad_batch_lazy_stats": (C.c_int, [vp, sz, sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_vad_batch_hold_from": (C.c_int, [vp, sz, C.POINTER(C.c_uint64)]),
    "fvad_vad_batch_run_device": (C.c_int, [vp, vp, vp, sz, C.POINTER(sz), c_float_p, sz, C.POINTER(sz), sz]),
    "fvad_vad_batch_run_device_part": (C.c_int, [vp, vp, vp, sz, C.POINTER(sz), c_float_p, sz, C.POINTER(sz), sz, C.c_uint64]),
    "fvad_vad_batch_score_device": (C.c_int, [vp, vp]),
    "fvad_vad_batch_device_bytes": (sz, [vp]),
    "fvad_vad_batch_chain_form": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "fvad_vad_batch_retain_configs": (C.c_int, [vp, vp, C.POINTER(C.c_uint32), sz]),
    "fvad_vad_batch_create_sweep_sized": (C.c_int, [C.POINTER(VadConfig), C.POINTER(sz), sz, sz, sz, sz, C.POINTER(vp)]),
    "fvad_vad_batch_frame_sizes": (C.c_int, [vp, C.POINTER(sz), sz, C.POINTER(sz), C.POINTER(C.c_uint32)]),
    "fvad_vad_batch_run_sized": (C.c_int, [vp, c_float_p, sz, C.POINTER(sz), c_float_p, sz, sz, sz, C.c_uint64, C.c_int]),
    "fvad_vad_batch_run_device_sized": (C.c_int, [vp, vp, vp, sz, C.POINTER(sz), c_float_p, sz, C.POINTER(sz), sz]),
    "fvad_vad_batch_run_device_part_sized": (C.c_int, [vp, vp, vp, sz, C.POINTER(sz), c_float_p, sz, C.POINTER(sz), sz, C.c_uint64]),
    "fvad_vad_batch_run_device_part_async": (C.c_int, [vp, vp, vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz), sz, C.c_uint64]),
    "fvad_vad_batch_part_wait": (C.c_int, [vp, vp]),
    "fvad_vad_batch_frame_ratios_device": (C.c_int, [vp, vp, vp, sz, C.POINTER(sz), C.POINTER(sz), sz, C.c_uint64, vp, sz]),
    "fvad_vad_batch_frame_ratios": (C.c_int, [vp, c_float_p, sz, C.POINTER(sz), C.POINTER(sz), sz, C.c_uint64, c_float_p, sz]),
    "fvad_vad_batch_avgs_form": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "fvad_vad_batch_avgs_bytes": (sz, [vp]),
    "fvad_vad_batch_avg_keys": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), sz, C.POINTER(sz), C.POINTER(sz),
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fvad_vad_batch_averages_device": (C.c_int, [vp, vp, vp, sz, C.POINTER(sz), c_float_p, sz, C.POINTER(sz), sz, C.c_uint64,
                                                 C.POINTER(C.c_double), C.POINTER(C.c_double), sz]),
    "fvad_vad_batch_trigger_keys": (C.c_int, [vp, C.POINTER(C.c_uint32), sz, C.POINTER(sz), C.POINTER(C.c_uint32)]),
    "fvad_vad_batch_trigger_form": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "fvad_vad_batch_trigger_bytes": (sz, [vp]),
    "fvad_vad_batch_trigger_launches": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_vad_batch_trigger_bits": (C.c_int, [vp, vp, C.POINTER(C.c_uint64), sz]),
    "fvad_vad_finish_bits": (C.c_int, [C.POINTER(VadConfig), sz, sz, C.POINTER(C.c_uint64), c_float_p, sz, C.c_uint64,
                                       C.POINTER(C.c_uint64), C.POINTER(SpeechSegment), sz, C.POINTER(sz)]),
    "fvad_vad_avg_chain": (C.c_int, [c_float_p, sz, sz, C.c_uint32, c_float_p, C.POINTER(C.c_double)]),
    "fvad_ra_create": (C.c_int, [sz, C.c_int, C.c_double, C.POINTER(vp)]),
    "fvad_ra_destroy": (None, [vp]),
    "fvad_ra_push": (C.c_double, [vp, C.c_float]),
    "fvad_ra_last_avg": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "fvad_pipeline_config_default": (None, [C.POINTER(PipelineConfig)]),
    "fvad_pipeline_create": (C.c_int, [vp, C.POINTER(PipelineConfig), C.POINTER(Callbacks),
                                       C.POINTER(vp)]),
    "fvad_pipeline_destroy": (None, [vp]),
    "fvad_pipeline_push_samples": (C.c_int, [vp, C.POINTER(c_float_p), sz,
                                             C.POINTER(C.c_uint64)]),
    "fvad_pipeline_total_write_count": (C.c_uint64, [vp]),
    "fvad_pipeline_segment_count": (sz, [vp]),
    "fvad_pipeline_segments": (C.c_int, [vp, C.POINTER(SpeechSegment), sz, C.POINTER(sz)]),
    "fvad_pipeline_alt_segments": (C.c_int, [vp, sz, C.POINTER(SpeechSegment), sz,
                                             C.POINTER(sz)]),
    "fvad_pipeline_audit": (C.c_int, [vp, C.POINTER(VadAudit)]),
    "fvad_pipeline_enable_trace": (C.c_int, [vp, C.c_int]),
    "fvad_pipeline_n_fft_frames": (sz, [vp]),
    "fvad_pipeline_trace": (C.c_int, [vp, c_float_p, c_float_p, sz]),
    "fvad_segment_to_sec": (SegmentSec, [C.POINTER(SpeechSegment), sz]),
    "fvad_stats_from_segments": (C.c_int, [C.POINTER(SegmentSec), sz, C.POINTER(SegmentSec), sz,
                                           C.POINTER(StatConfig), C.POINTER(SingleStats)]),
    "fvad_stats_aggregate": (C.c_int, [C.POINTER(SingleStats), sz, C.POINTER(AggregateStats)]),
    "fvad_vad_batch_set_references": (C.c_int, [vp, C.POINTER(SegmentSec), C.POINTER(sz), C.POINTER(StatConfig)]),
    "fvad_vad_batch_set_keep_segments": (C.c_int, [vp, C.c_int]),
    "fvad_vad_batch_score": (C.c_int, [vp, C.c_int]),
    "fvad_vad_batch_config_stats": (C.c_int, [vp, sz, C.POINTER(SingleStats)]),
    "fvad_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8), sz]),
    "fvad_comm_create": (C.c_int, [vp, C.POINTER(C.c_uint8), sz, C.c_int, C.c_int, C.POINTER(vp)]),
    "fvad_comm_destroy": (None, [vp]),
    "fvad_comm_world": (C.c_int, [vp]),
    "fvad_comm_rank": (C.c_int, [vp]),
    "fvad_stats_allgather": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(SingleStats), sz, sz, C.POINTER(SingleStats)]),
    "fvad_parse_audacity": (C.c_int, [C.c_char_p, sz, C.POINTER(SegmentSec), sz, C.POINTER(sz)]),
    "fvad_wav_read": (C.c_int, [C.c_char_p, C.POINTER(C.POINTER(c_float_p)), C.POINTER(sz),
                                C.POINTER(sz), C.POINTER(sz)]),
    "fvad_wav_free": (None, [C.POINTER(c_float_p), sz]),
    "fvad_wav_read_i16": (C.c_int, [C.c_char_p, C.POINTER(C.POINTER(C.POINTER(C.c_int16))), C.POINTER(sz),
                                    C.POINTER(sz), C.POINTER(sz)]),
    "fvad_wav_free_i16": (None, [C.POINTER(C.POINTER(C.c_int16)), sz]),
    "fvad_wav_write": (C.c_int, [C.c_char_p, C.POINTER(c_float_p), sz, sz, sz, C.c_int]),
    "fvad_wav_write_i16": (C.c_int, [C.c_char_p, C.POINTER(C.POINTER(C.c_int16)), sz, sz, sz]),
    "fvad_clips_plan": (C.c_int, [C.POINTER(C.c_uint64), sz, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_clips_from_segments": (C.c_int, [C.POINTER(SpeechSegment), sz, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), sz,
                                           C.POINTER(sz), C.POINTER(sz)]),
    "fvad_clips_export_device": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.POINTER(C.c_int32),
                                           c_float_p, c_float_p, C.POINTER(C.c_uint64)]),
    "fvad_clips_export": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.POINTER(C.c_int32),
                                    c_float_p, c_float_p, C.POINTER(C.c_uint64)]),
    "fvad_clips_split_check": (C.c_int, [vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.c_int,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_clips_export_split_device": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz,
                                                 C.POINTER(C.c_int32), c_float_p, c_float_p, C.POINTER(C.c_uint64)]),
    "fvad_clips_export_split": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz,
                                          C.POINTER(C.c_int32), c_float_p, c_float_p, C.POINTER(C.c_uint64)]),
    "fvad_clips_phase_skips": (C.c_int, [C.POINTER(C.c_uint64), sz, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fvad_clips_plan_strided": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), sz, C.c_uint32, C.c_int, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_clips_export_strided_device": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.POINTER(C.c_int32),
                                                   c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]),
    "fvad_clips_export_strided": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.POINTER(C.c_int32),
                                            c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]),
    "fvad_clips_export_split_strided_device": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz,
                                                         C.POINTER(C.c_int32), c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_uint32,
                                                         C.POINTER(C.c_uint32)]),
    "fvad_clips_export_split_strided": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz,
                                                  C.POINTER(C.c_int32), c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_uint32,
                                                  C.POINTER(C.c_uint32)]),
    "fvad_clips_fir_design": (C.c_int, [C.c_uint32, C.c_uint32, C.c_double, C.c_double, c_float_p]),
    "fvad_clips_fir_check": (C.c_int, [c_float_p, C.c_uint32]),
    "fvad_clips_export_fir_device": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.POINTER(C.c_int32),
                                               c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32), c_float_p,
                                               C.c_uint32]),
    "fvad_clips_export_fir": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.POINTER(C.c_int32),
                                        c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32), c_float_p,
                                        C.c_uint32]),
    "fvad_clips_export_split_fir_device": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz,
                                                     C.POINTER(C.c_int32), c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_uint32,
                                                     C.POINTER(C.c_uint32), c_float_p, C.c_uint32]),
    "fvad_clips_export_split_fir": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz,
                                              C.POINTER(C.c_int32), c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_uint32,
                                              C.POINTER(C.c_uint32), c_float_p, C.c_uint32]),
    "fvad_mel_design": (C.c_int, [C.c_double, C.c_uint32, C.c_uint32, C.c_double, C.c_double, c_float_p]),
    "fvad_clips_plan_mel": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), sz, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_clips_mel_check": (C.c_int, [vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.c_int, C.c_uint32,
                                       C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, c_float_p, C.c_float, c_float_p,
                                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_clips_export_mel_device": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.POINTER(C.c_int32),
                                               c_float_p, c_float_p, C.POINTER(C.c_uint64),
                                               C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, c_float_p, C.c_float, c_float_p,
                                               C.POINTER(C.c_uint64), c_float_p]),
    "fvad_clips_export_mel": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.POINTER(C.c_int32),
                                        c_float_p, c_float_p, C.POINTER(C.c_uint64),
                                               C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, c_float_p, C.c_float, c_float_p,
                                               C.POINTER(C.c_uint64), c_float_p]),
    "fvad_mel_design_kaldi": (C.c_int, [C.c_double, C.c_uint32, C.c_uint32, C.c_double, C.c_double, c_float_p]),
    "fvad_clips_plan_fbank": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), sz, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_clips_fbank_check": (C.c_int, [vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.c_int, C.c_uint32,
                                         C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, c_float_p,
                                         C.c_float, C.c_float, C.c_int, C.c_float, C.c_int,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_clips_export_fbank_device": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.POINTER(C.c_int32),
                                                 c_float_p, c_float_p, C.POINTER(C.c_uint64),
                                                 C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, c_float_p,
                                                 C.c_float, C.c_float, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_uint64), c_float_p]),
    "fvad_clips_export_fbank": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.POINTER(C.c_int32),
                                          c_float_p, c_float_p, C.POINTER(C.c_uint64),
                                          C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, c_float_p,
                                          C.c_float, C.c_float, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_uint64), c_float_p]),
    "fvad_clips_split_mel_check": (C.c_int, [vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.c_int,
                                             C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, c_float_p, C.c_float, c_float_p,
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_clips_export_split_mel_device": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz,
                                                     C.POINTER(C.c_int32), c_float_p, c_float_p, C.POINTER(C.c_uint64),
                                                     C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, c_float_p, C.c_float, c_float_p,
                                                     C.POINTER(C.c_uint64), c_float_p]),
    "fvad_clips_export_split_mel": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz,
                                              C.POINTER(C.c_int32), c_float_p, c_float_p, C.POINTER(C.c_uint64),
                                              C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, c_float_p, C.c_float, c_float_p,
                                              C.POINTER(C.c_uint64), c_float_p]),
    "fvad_clips_split_fbank_check": (C.c_int, [vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.c_int,
                                               C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, c_float_p,
                                               C.c_float, C.c_float, C.c_int, C.c_float, C.c_int,
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_clips_export_split_fbank_device": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz,
                                                       C.POINTER(C.c_int32), c_float_p, c_float_p, C.POINTER(C.c_uint64),
                                                       C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, c_float_p,
                                                       C.c_float, C.c_float, C.c_int, C.c_float, C.c_int,
                                                       C.POINTER(C.c_uint64), c_float_p]),
    "fvad_clips_export_split_fbank": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz,
                                                C.POINTER(C.c_int32), c_float_p, c_float_p, C.POINTER(C.c_uint64),
                                                C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, c_float_p,
                                                C.c_float, C.c_float, C.c_int, C.c_float, C.c_int,
                                                C.POINTER(C.c_uint64), c_float_p]),
    "fvad_clips_resample_check": (C.c_int, [C.c_uint32, C.c_uint32, c_float_p, C.c_uint32]),
    "fvad_clips_resample_tile": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "fvad_clips_plan_resampled": (C.c_int, [C.POINTER(C.c_uint64), sz, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_clips_export_resampled_device": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.POINTER(C.c_int32),
                                                     c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, c_float_p,
                                                     C.c_uint32]),
    "fvad_clips_export_resampled": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, C.POINTER(C.c_int32),
                                              c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, c_float_p,
                                              C.c_uint32]),
    "fvad_clips_export_split_resampled_device": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz,
                                                           C.POINTER(C.c_int32), c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_uint32,
                                                           C.c_uint32, c_float_p, C.c_uint32]),
    "fvad_clips_export_split_resampled": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, sz, sz, C.c_int, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz,
                                                    C.POINTER(C.c_int32), c_float_p, c_float_p, C.POINTER(C.c_uint64), C.c_uint32,
                                                    C.c_uint32, c_float_p, C.c_uint32]),
    "fvad_wav_probe": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint64)]),
    "fvad_ingest_check": (C.c_int, [C.POINTER(C.c_uint64), sz, C.c_uint64, C.c_int, sz, sz, sz]),
    "fvad_ingest_device": (C.c_int, [vp, vp, C.c_uint64, C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, sz, sz]),
    "fvad_ingest": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_uint64), sz, C.c_int, vp, sz, sz, sz]),
    "fvad_wav_header": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, vp, sz, C.POINTER(sz)]),
    "fvad_egress_check": (C.c_int, [C.POINTER(C.c_uint64), sz, C.c_uint64, C.c_int, sz, sz, sz]),
    "fvad_egress_device": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, vp, C.c_uint64]),
    "fvad_egress": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.POINTER(vp)]),
    "fvad_egress_mix_check": (C.c_int, [C.POINTER(C.c_uint64), sz, C.c_uint64, C.c_int, C.c_float, C.c_float, sz, sz, sz, sz, sz]),
    "fvad_egress_mix_device": (C.c_int, [vp, vp, sz, sz, vp, sz, sz, C.c_int, sz, C.c_float, C.c_float, C.POINTER(C.c_uint64), sz, vp, C.c_uint64]),
    "fvad_egress_mix": (C.c_int, [vp, vp, sz, sz, vp, sz, sz, C.c_int, sz, C.c_float, C.c_float, C.POINTER(C.c_uint64), sz, C.POINTER(vp)]),
    "fvad_egress_resample_tile": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "fvad_egress_resample_ready": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]),
    "fvad_egress_resample_check": (C.c_int, [C.POINTER(C.c_uint64), sz, C.c_uint64, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, C.c_int, sz, sz, sz]),
    "fvad_egress_resample_device": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, vp, C.c_uint64]),
    "fvad_egress_resample": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, C.POINTER(vp)]),
    "fvad_egress_resample_strided_check": (C.c_int, [C.POINTER(C.c_uint64), sz, C.c_uint64, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, C.c_uint32, C.c_int, sz, sz, sz]),
    "fvad_egress_resample_strided_device": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, C.c_uint32, vp, C.c_uint64]),
    "fvad_egress_resample_strided": (C.c_int, [vp, vp, C.c_int, sz, sz, sz, C.POINTER(C.c_uint64), sz, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
    "fvad_resample_ratio": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fvad_resample_out_frames": (C.c_uint64, [C.c_uint64, C.c_uint32, C.c_uint32]),
    "fvad_resample_design": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, c_float_p, C.POINTER(C.c_uint32)]),
    "fvad_resample_window": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fvad_ingest_resample_tile": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "fvad_ingest_resample_check": (C.c_int, [C.POINTER(C.c_uint64), sz, C.c_uint64, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, C.c_int, sz, sz, sz]),
    "fvad_ingest_resample_device": (C.c_int, [vp, vp, C.c_uint64, C.POINTER(C.c_uint64), sz, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, vp, sz, sz, sz]),
    "fvad_ingest_resample": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_uint64), sz, C.c_uint32, C.c_uint32, c_float_p, C.c_uint32, vp, sz, sz, sz]),
}

_lib = None


def lib():
    """Load libfvad_hip.so (built in-tree by formula-vad_amd/csrc/Makefile). Raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `make -C formula-vad_amd/csrc` "
                "(__graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def fptr(a):
    if a is None:
        return None
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_float_p)


def check(status, where, ctx=None):
    if status != FVAD_OK:
        detail = lib().fvad_last_error(ctx).decode() if ctx else ""
        raise FvadError(status, where, detail)


def weights_to_dict(w):
    """Weights struct (borrowed pointers) -> dict of numpy copies"""
    shapes = weight_shapes(w.n_bins, w.n_fc1, w.n_hidden, w.n_fc2, w.n_fc3)
    return {k: np.ctypeslib.as_array(getattr(w, k), shape=shapes[k]).copy() for k in WEIGHT_NAMES}


def dict_to_weights(wd):
    w = Weights()
    w.n_bins = wd["fc1_w"].shape[1]
    w.n_fc1 = wd["fc1_w"].shape[0]
    w.n_hidden = wd["gru1_r"].shape[1]
    w.n_fc2 = wd["fc2_w"].shape[0]
    w.n_fc3 = wd["fc3_w"].shape[0]
    keep = {}
    for k in WEIGHT_NAMES:
        keep[k] = np.ascontiguousarray(wd[k], dtype=np.float32)
        setattr(w, k, fptr(keep[k]))
    return w, keep


def synth_weights(seed):
    """Host-only: the library's seeded NSNet2-shaped weights as a dict of numpy arrays"""
    w = Weights()
    owner = vp()
    check(lib().fvad_synth_nsnet2(seed, C.byref(w), C.byref(owner)), "fvad_synth_nsnet2")
    try:
        return weights_to_dict(w)
    finally:
        lib().fvad_weights_free(owner)


def read_onnx(path):
    w = Weights()
    owner = vp()
    check(lib().fvad_onnx_read_nsnet2(path.encode(), C.byref(w), C.byref(owner)),
          "fvad_onnx_read_nsnet2")
    try:
        return weights_to_dict(w)
    finally:
        lib().fvad_weights_free(owner)


class Context:
    """fvad_ctx: one HIP device + stream (+ the loaded NSNet2 model)"""

    def __init__(self, device=0):
        self.h = vp()
        check(lib().fvad_ctx_create(device, C.byref(self.h)), "fvad_ctx_create")
        self.device = int(device)

    def close(self):
        if self.h:
            lib().fvad_ctx_destroy(self.h)
            self.h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, status, where):
        check(status, where, self.h)

    def load_synth(self, seed):
        self._ck(lib().fvad_load_nsnet2_synth(self.h, seed), "fvad_load_nsnet2_synth")

    def load_weights(self, wd):
        w, keep = dict_to_weights(wd)
        self._ck(lib().fvad_load_nsnet2_weights(self.h, C.byref(w)), "fvad_load_nsnet2_weights")

    def load_onnx(self, path):
        self._ck(lib().fvad_load_nsnet2_onnx(self.h, path.encode()), "fvad_load_nsnet2_onnx")

    def weights(self):
        w = Weights()
        self._ck(lib().fvad_get_nsnet2_weights(self.h, C.byref(w)), "fvad_get_nsnet2_weights")
        return weights_to_dict(w)

    def synchronize(self):
        self._ck(lib().fvad_ctx_synchronize(self.h), "fvad_ctx_synchronize")

    def set_nn_math(self, mode):
        """'f32' (default: the reference's arithmetic) or 'f16x3' (emulation on the f16 matrix cores): arithmetic of the
        NSNet2 matrix products at every batch size; returns the previous mode"""
        m = {"f32": 0, "f16x3": 1, "bf16x3": 2}[mode]
        prev = lib().fvad_ctx_set_nn_math(self.h, m)
        if prev < 0:
            self._ck(prev, "fvad_ctx_set_nn_math")
        return ("f32", "f16x3", "bf16x3")[prev]

    def set_nn_math_raw(self, mode):
        return self._ck(lib().fvad_ctx_set_nn_math(self.h, int(mode)), "fvad_ctx_set_nn_math")

    def nn_math_effective(self):
        """what the context uses with the loaded model: 'f32' or 'f16x3'"""
        m = lib().fvad_ctx_nn_math_effective(self.h)
        if m < 0:
            self._ck(m, "fvad_ctx_nn_math_effective")
        return ("f32", "f16x3", "bf16x3")[m]

    def last_nn_path(self):
        return lib().fvad_ctx_last_nn_path(self.h).decode()

    def nn_tap(self, layer, first, n):
        """fvad_ctx_nn_tap (a test tap): layer "h1" | "h2" | "f2" | "f3" | "gains" of the last NSNet2 pass for its sequences
        [first, first + n) as a float32 array [n][rows][width]; None where the pass's kernels do not keep that layer"""
        code = int(NN_TAP_LAYERS.get(layer, layer))
        L = lib()
        L.fvad_debug_nn_tap_shape.restype = C.c_int
        L.fvad_debug_nn_tap_shape.argtypes = [vp, C.c_int, C.POINTER(sz), C.POINTER(sz)]
        rows, width = sz(0), sz(0)
        # the entry point takes no capacity: ask for the pass's shape first and size the buffer from it
        st = L.fvad_debug_nn_tap_shape(self.h, code, C.byref(rows), C.byref(width))
        if st == FVAD_ERR_NOT_AVAILABLE:
            return None
        self._ck(st, "fvad_ctx_nn_tap")
        buf = np.empty((max(int(n), 1), rows.value, width.value), np.float32)
        st = L.fvad_ctx_nn_tap(self.h, code, int(first), int(n), fptr(buf), C.byref(rows), C.byref(width))
        if st == FVAD_ERR_NOT_AVAILABLE:
            return None
        self._ck(st, "fvad_ctx_nn_tap")
        assert buf.shape[1:] == (rows.value, width.value)
        return buf[: int(n)]

    def set_option(self, name, value=None):
        """testing / tuning aid (fvad_ctx_set_option); value None restores the default"""
        v = None if value is None else str(value).encode()
        self._ck(lib().fvad_ctx_set_option(self.h, name.encode(), v), "fvad_ctx_set_option")
        self.__dict__.setdefault("_options_set", {})[name] = None if value in (None, "") else str(value)

    def option_set(self, name):
        """the value last given to set_option for name on this object (None: the default, or never set); for an option never set
        here, what fvad_ctx_create read from the environment variable FVAD_<NAME>"""
        opts = self.__dict__.get("_options_set", {})
        if name in opts:
            return opts[name]
        return os.environ.get("FVAD_" + name.upper()) or None

    def options(self, **kv):
        """context manager: set the options, restore the defaults on exit"""
        ctx = self

        class _Opts:
            def __enter__(self_):
                for k, v in kv.items():
                    ctx.set_option(k, v)
                return ctx

            def __exit__(self_, *exc):
                for k in kv:
                    ctx.set_option(k, None)
                return False
        return _Opts()

    def ws_fallbacks(self):
        n = C.c_uint64(0)
        self._ck(lib().fvad_ctx_ws_fallbacks(self.h, C.byref(n)), "fvad_ctx_ws_fallbacks")
        return n.value

    def ws2_waits(self, wait_class):
        """(layer 1, layer 2) first-poll waits of gru_ws2k in 10 ns ticks for a group-shape class (fvad_ctx_ws2_waits)"""
        w = lib().fvad_ctx_ws2_waits(self.h, wait_class)
        return w & 0xFFFF, w >> 16

    def enable_timing(self, on=True):
        self._ck(lib().fvad_ctx_enable_timing(self.h, 1 if on else 0), "fvad_ctx_enable_timing")
        self._timing = bool(on)

    @property
    def timing(self):
        """whether kernel timing is on (as set through enable_timing; off in a new context)"""
        return getattr(self, "_timing", False)

    def kernel_times(self):
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = sz()
        self._ck(lib().fvad_ctx_kernel_times(self.h, names, ms, cap, C.byref(n)),
                 "fvad_ctx_kernel_times")
        return {names[i].decode(): ms[i] for i in range(min(n.value, cap))}

    def nsnet2_forward(self, features):
        f = np.ascontiguousarray(features, dtype=np.float32)
        assert f.ndim == 3 and f.shape[2] == 161
        g = np.zeros_like(f)
        self._ck(lib().fvad_nsnet2_forward(self.h, fptr(f), f.shape[0], f.shape[1], fptr(g)),
                 "fvad_nsnet2_forward")
        return g

    def engine_run(self, lanes_pcm, want_denoised=False, want_bins=False, states=None,
                   max_chunks_per_launch=0, min_bin=11, max_bin=43, want_taps=False, want_denoised_i16=False, fft_size=1024):
        """lanes_pcm: list of 1-D host arrays, float32 or int16 (PCM16: converted on the GPU). Returns list of dicts."""
        n = len(lanes_pcm)
        arr = (Lane * n)()
        keep = []
        for i, x in enumerate(lanes_pcm):
            x = np.ascontiguousarray(x) if np.asarray(x).dtype == np.int16 else np.ascontiguousarray(x, dtype=np.float32)
            n_chunks = x.shape[0] // 24000
            cap_frames = (n_chunks * 24000 + fft_size) // fft_size + 1
            band = np.zeros(cap_frames, np.float32)
            rms = np.zeros(max(n_chunks, 1), np.float32)
            den = np.zeros(n_chunks * 24000, np.float32) if want_denoised else None
            bins = np.zeros((cap_frames, fft_size // 2 + 1), np.float32) if want_bins else None
            spec = np.zeros((n_chunks, 50, 161, 2), np.float32) if want_taps else None
            feat = np.zeros((n_chunks, 54, 161), np.float32) if want_taps else None
            den16 = np.zeros(n_chunks * 24000, np.int16) if want_denoised_i16 else None
            keep.append((x, band, rms, den, bins, spec, feat, den16))
            L = arr[i]
            if x.dtype == np.int16:
                L.pcm = None
                L.pcm_i16 = x.ctypes.data_as(C.POINTER(C.c_int16))
            else:
                L.pcm = fptr(x)
            L.denoised_i16 = den16.ctypes.data_as(C.POINTER(C.c_int16)) if den16 is not None and den16.size else None
            L.n_samples = x.shape[0]
            L.state = states[i] if states else None
            L.denoised = fptr(den) if den is not None and den.size else None
            L.band_sum = fptr(band)
            L.band_sum_capacity = cap_frames
            L.chunk_rms = fptr(rms)
            L.chunk_rms_capacity = rms.shape[0]
            L.fft_bins = fptr(bins) if bins is not None else None
            L.spectrogram = fptr(spec) if spec is not None and spec.size else None
            L.features = fptr(feat) if feat is not None and feat.size else None
        opts = EngineOpts()
        lib().fvad_engine_opts_default(C.byref(opts))
        opts.max_chunks_per_launch = max_chunks_per_launch
        opts.min_bin = min_bin
        opts.max_bin = max_bin
        opts.fft_size = fft_size
        self._ck(lib().fvad_engine_run(self.h, arr, n, C.byref(opts)), "fvad_engine_run")
        out = []
        for i in range(n):
            x, band, rms, den, bins, spec, feat, den16 = keep[i]
            nf = arr[i].n_fft_frames
            nc = arr[i].n_chunks
            out.append({"n_chunks": nc, "n_fft_frames": nf,
                        "first_frame_index": arr[i].first_frame_index,
                        "band_sum": band[:nf].copy(), "chunk_rms": rms[:nc].copy(),
                        "denoised": den, "fft_bins": None if bins is None else bins[:nf].copy(),
                        "spectrogram": None if spec is None else spec.view(np.complex64)[..., 0],
                        "features": feat, "denoised_i16": den16})
        return out

    def host_alloc(self, n_floats):
        """page-locked float32 buffer (fvad_host_alloc) as a numpy array; release with host_free(arr)"""
        p = vp()
        self._ck(lib().fvad_host_alloc(self.h, int(n_floats) * 4, C.byref(p)), "fvad_host_alloc")
        arr = np.ctypeslib.as_array(C.cast(p, c_float_p), shape=(int(n_floats),))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = self._pinned.pop(arr.ctypes.data)
        lib().fvad_host_free(self.h, p)

    def device_alloc(self, n_bytes):
        """HBM on the context's device (fvad_device_alloc); returns the device address as an int"""
        p = vp()
        self._ck(lib().fvad_device_alloc(self.h, int(n_bytes), C.byref(p)), "fvad_device_alloc")
        return p.value

    def device_free(self, addr):
        lib().fvad_device_free(self.h, vp(addr))

    def to_device(self, addr, arr):
        """copy a C-contiguous numpy array to device address `addr` (returns after the copy completed)"""
        assert arr.flags["C_CONTIGUOUS"]
        self._ck(lib().fvad_ctx_copy_to_device(self.h, vp(addr), arr.ctypes.data, arr.nbytes), "fvad_ctx_copy_to_device")
        self.synchronize()

    def to_host(self, arr, addr):
        """fill a C-contiguous numpy array from device address `addr`"""
        assert arr.flags["C_CONTIGUOUS"]
        self._ck(lib().fvad_ctx_copy_to_host(self.h, arr.ctypes.data, vp(addr), arr.nbytes), "fvad_ctx_copy_to_host")
        self.synchronize()
        return arr

    def enqueue_device(self, d_pcm, n_lanes, lane_stride, n_samples, d_den, d_band, d_rms, max_chunks_per_launch=0,
                       no_wait=False, use_graph=False):
        opts = EngineOpts()
        lib().fvad_engine_opts_default(C.byref(opts))
        opts.max_chunks_per_launch = max_chunks_per_launch
        opts.no_wait = 1 if no_wait else 0
        opts.use_graph = 1 if use_graph else 0
        self._ck(lib().fvad_engine_enqueue_device(self.h, vp(d_pcm), n_lanes, lane_stride, n_samples,
                                                  vp(d_den) if d_den else None, vp(d_band), vp(d_rms) if d_rms else None,
                                                  C.byref(opts)), "fvad_engine_enqueue_device")

    def band_sums_device(self, d_den, n_lanes, lane_stride, n_samples, bins, d_band, band_stride, fft_size=1024):
        """fvad_engine_band_sums_device: bins = [(min_bin, max_bin), ...]; band j of lane l at d_band + (j * n_lanes + l) *
        band_stride floats (device addresses as ints)"""
        b = np.ascontiguousarray(np.asarray(bins, np.int32).reshape(-1, 2))
        self._ck(lib().fvad_engine_band_sums_device(self.h, vp(d_den), n_lanes, lane_stride, n_samples, fft_size,
                                                    b.ctypes.data_as(C.POINTER(C.c_int32)), b.shape[0], vp(d_band), band_stride),
                 "fvad_engine_band_sums_device")

    def clips_export(self, d_src, src_pcm16, n_lanes, lane_stride, n_samples, clips, out_pcm16=False, d_out=None, out_capacity=None,
                     step=1, skips=None, taps=None, up=None, down=None):
        """fvad_clips_export (d_out None: the packed clips come back as a numpy array of the output format) or
        fvad_clips_export_device (d_out: a device address with room for out_capacity samples).  clips: [n][CLIP_FIELDS] uint64.
        Returns dict(best_channel, best_rms, runner_up_rms, offsets, total[, out]).
        step != 1 or skips: fvad_clips_export_strided(_device) -- of clip i the samples skips[i], skips[i] + step, ... (skips None:
        all 0); the dict then has "out_lens" too.
        taps (an odd number of float32, at most CLIP_FIR_TAPS_MAX): fvad_clips_export_fir(_device) -- the same clips, skips and slots,
        output q of a clip being sum_k taps[k] * x[skips[i] + q * step + k - (len(taps) - 1) / 2] over the zero-extended clip.
        up, down (with taps, an odd number of float32, at most RESAMPLE_TAPS_MAX; step 1 and no skips):
        fvad_clips_export_resampled(_device) -- clip i leaves as ceil(len * up / down) samples at up / down of the lanes' rate."""
        clips = _clip_rows(clips)
        n = clips.shape[0]
        if up is not None or down is not None:
            return self._clips_export_resampled("fvad_clips_export_resampled", (vp(d_src), CLIP_PCM16 if src_pcm16 else CLIP_F32, n_lanes, lane_stride, n_samples),
                                                clips, clips[:, 3] - clips[:, 2], out_pcm16, d_out, out_capacity, step, skips, taps, up, down)
        if step != 1 or skips is not None or taps is not None:
            return self._clips_export_strided("fvad_clips_export_fir" if taps is not None else "fvad_clips_export_strided", (vp(d_src), CLIP_PCM16 if src_pcm16 else CLIP_F32, n_lanes, lane_stride, n_samples),
                                              clips, clips[:, 3] - clips[:, 2], out_pcm16, d_out, out_capacity, step, skips, taps)
        offsets, total = clips_plan(clips, out_pcm16)
        best, rms, runner, offs = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint64)
        args = (self.h, vp(d_src), CLIP_PCM16 if src_pcm16 else CLIP_F32, n_lanes, lane_stride, n_samples,
                clips.ctypes.data_as(C.POINTER(C.c_uint64)), n, CLIP_PCM16 if out_pcm16 else CLIP_F32)
        info = (best.ctypes.data_as(C.POINTER(C.c_int32)), fptr(rms), fptr(runner), offs.ctypes.data_as(C.POINTER(C.c_uint64)))
        res = {"best_channel": best, "best_rms": rms, "runner_up_rms": runner, "offsets": offs, "total": total}
        if d_out is not None:
            self._ck(lib().fvad_clips_export_device(*args, vp(d_out), total if out_capacity is None else out_capacity, *info),
                     "fvad_clips_export_device")
            return res
        out = np.zeros(max(total, 1), np.int16 if out_pcm16 else np.float32)
        self._ck(lib().fvad_clips_export(*args, out.ctypes.data, total if out_capacity is None else out_capacity, *info),
                 "fvad_clips_export")
        res["out"] = out[:total]
        return res

    def clips_export_mel(self, d_src, src_pcm16, n_lanes, lane_stride, n_samples, clips, window, matrix, step=1, skips=None, hop=160,
                         floor=1e-10, norm=None, d_out=None, out_capacity=None):
        """fvad_clips_export_mel (d_out None: the features come back as a float32 array) or fvad_clips_export_mel_device (d_out:
        a device address with room for out_capacity floats): log-mel features of the clips' picked channels.  window: [n_fft]
        float32, matrix: [n_mels][n_fft / 2 + 1] float32, norm: None or (range, offset, scale).
        Returns dict(best_channel, best_rms, runner_up_rms, offsets, total, n_frames, feat_max[, out]); clip i's features are
        out[offsets[i] : offsets[i] + n_frames[i] * n_mels].reshape(n_frames[i], n_mels)."""
        def params(n_fft, window, n_mels, matrix):
            norm_ = None if norm is None else np.ascontiguousarray(np.asarray(norm, np.float32).reshape(3))
            return (n_fft, hop, fptr(window), n_mels, fptr(matrix), floor, None if norm_ is None else fptr(norm_)), norm_
        return self._clips_export_features("mel", (d_src, src_pcm16, n_lanes, lane_stride, n_samples), clips, window, matrix, None,
                                           "matrix must be [n_mels][n_fft / 2 + 1] for the window's n_fft", step, skips, hop, params,
                                           "feat_max", d_out, out_capacity)

    def clips_export_split_mel(self, a, b, src_pcm16, clips, window, matrix, step=1, skips=None, hop=160, floor=1e-10, norm=None,
                               d_out=None, out_capacity=None):
        """fvad_clips_export_split_mel (d_out None) or fvad_clips_export_split_mel_device: clips_export_mel over the split source
        of clips_export_split (a, b, [n][CLIP_SPLIT_FIELDS] rows).  Returns what clips_export_mel returns."""
        def params(n_fft, window, n_mels, matrix):
            norm_ = None if norm is None else np.ascontiguousarray(np.asarray(norm, np.float32).reshape(3))
            return (n_fft, hop, fptr(window), n_mels, fptr(matrix), floor, None if norm_ is None else fptr(norm_)), norm_
        return self._clips_export_features("mel", (a, b, src_pcm16), clips, window, matrix, None,
                                           "matrix must be [n_mels][n_fft / 2 + 1] for the window's n_fft", step, skips, hop, params,
                                           "feat_max", d_out, out_capacity)

    def clips_export_fbank(self, d_src, src_pcm16, n_lanes, lane_stride, n_samples, clips, window, matrix, n_fft=512, step=1, skips=None,
                           hop=160, scale=32768.0, preemph=0.97, remove_dc=True, floor=FLT_EPSILON, cmn=False, d_out=None, out_capacity=None):
        """fvad_clips_export_fbank (d_out None: the features come back as a float32 array) or fvad_clips_export_fbank_device:
        Kaldi-style filter-bank features of the clips' picked channels.  window: [win_length] float32, matrix:
        [n_mels][n_fft / 2 + 1] float32.
        Returns dict(best_channel, best_rms, runner_up_rms, offsets, total, n_frames, means[, out]); clip i's features are
        out[offsets[i] : offsets[i] + n_frames[i] * n_mels].reshape(n_frames[i], n_mels), means[i] its per-band mean."""
        def params(win, window, n_mels, matrix):
            return (win, int(n_fft), hop, fptr(window), n_mels, fptr(matrix), scale, preemph, int(remove_dc), floor, int(cmn)), None
        return self._clips_export_features("fbank", (d_src, src_pcm16, n_lanes, lane_stride, n_samples), clips, window, matrix, n_fft,
                                           "matrix must be [n_mels][n_fft / 2 + 1]", step, skips, hop, params, "means", d_out, out_capacity)

    def clips_export_split_fbank(self, a, b, src_pcm16, clips, window, matrix, n_fft=512, step=1, skips=None, hop=160, scale=32768.0,
                                 preemph=0.97, remove_dc=True, floor=FLT_EPSILON, cmn=False, d_out=None, out_capacity=None):
        """fvad_clips_export_split_fbank (d_out None) or fvad_clips_export_split_fbank_device: clips_export_fbank over the split
        source of clips_export_split.  Returns what clips_export_fbank returns."""
        def params(win, window, n_mels, matrix):
            return (win, int(n_fft), hop, fptr(window), n_mels, fptr(matrix), scale, preemph, int(remove_dc), floor, int(cmn)), None
        return self._clips_export_features("fbank", (a, b, src_pcm16), clips, window, matrix, n_fft,
                                           "matrix must be [n_mels][n_fft / 2 + 1]", step, skips, hop, params, "means", d_out, out_capacity)

    def _clips_export_features(self, family, src, clips, window, matrix, n_fft, matrix_why, step, skips, hop, params, extra, d_out, out_capacity):
        """the two feature exports: fvad_clips_export_<family> (+ "_device" with d_out) after fvad_clips_plan_<family>.  n_fft None:
        the window's length; params(taps, window, n_mels, matrix) -> (the family's arguments between skips and n_frames, what
        they point into); extra: the result's own key, "feat_max" [n] or "means" [n][n_mels].  src: (d_src, src_pcm16, n_lanes,
        lane_stride, n_samples), or (a, b, src_pcm16) as for clips_export_split -- fvad_clips_export_split_<family>(_device) over
        [n][CLIP_SPLIT_FIELDS] rows"""
        split = len(src) == 3
        if split:
            a, b, src_pcm16 = src
            clips = _clip_split_rows(clips)
            lens, src_args = clips[:, 3] + clips[:, 6], (vp(a[0]), a[1], a[2], a[3], vp(b[0]), b[1], b[2], b[3], CLIP_PCM16 if src_pcm16 else CLIP_F32)
        else:
            d_src, src_pcm16, n_lanes, lane_stride, n_samples = src
            clips = _clip_rows(clips)
            lens, src_args = clips[:, 3] - clips[:, 2], (vp(d_src), CLIP_PCM16 if src_pcm16 else CLIP_F32, n_lanes, lane_stride, n_samples)
        n = clips.shape[0]
        window = np.ascontiguousarray(np.asarray(window, np.float32).reshape(-1))
        matrix = np.ascontiguousarray(np.asarray(matrix, np.float32))
        taps, n_mels = window.shape[0], matrix.shape[0]
        if matrix.ndim != 2 or matrix.shape[1] != (taps if n_fft is None else n_fft) // 2 + 1:
            raise ValueError(matrix_why)
        skips = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32).reshape(n))
        own, keep = params(taps, window, n_mels, matrix)
        frames, offsets, total = _clips_plan_features("fvad_clips_plan_" + family, lens, skips, step, taps, hop, n_mels) if n else (np.zeros(0, np.uint64), None, 0)
        best, rms, runner, offs = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint64)
        n_frames, per_clip = np.zeros(n, np.uint64), np.zeros((n, n_mels) if extra == "means" else n, np.float32)
        args = (self.h, *src_args, clips.ctypes.data_as(C.POINTER(C.c_uint64)), n, CLIP_F32)
        info = (best.ctypes.data_as(C.POINTER(C.c_int32)), fptr(rms), fptr(runner), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                step, None if skips is None else skips.ctypes.data_as(C.POINTER(C.c_uint32)), *own,
                n_frames.ctypes.data_as(C.POINTER(C.c_uint64)), fptr(per_clip))
        res = {"best_channel": best, "best_rms": rms, "runner_up_rms": runner, "offsets": offs, "total": total, "n_frames": n_frames,
               extra: per_clip}
        name = ("fvad_clips_export_split_" if split else "fvad_clips_export_") + family
        if d_out is not None:
            self._ck(getattr(lib(), name + "_device")(*args, vp(d_out), total if out_capacity is None else out_capacity, *info), name + "_device")
            return res
        out = np.zeros(max(total, 1), np.float32)
        self._ck(getattr(lib(), name)(*args, out.ctypes.data, total if out_capacity is None else out_capacity, *info), name)
        res["out"] = out[:total]
        return res

    def _clips_export_strided(self, name, src_args, clips, lens, out_pcm16, d_out, out_capacity, step, skips, taps=None):
        """the four strided calls and the four filtered ones (taps): `name` (+ "_device" with d_out), src_args the arguments
        between ctx and the clips"""
        n = clips.shape[0]
        skips = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32).reshape(n))
        out_lens, offsets, total = clips_plan_strided(lens, skips, step, out_pcm16) if n else (np.zeros(0, np.uint64), None, 0)
        best, rms, runner, offs = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint64)
        args = (self.h, *src_args, clips.ctypes.data_as(C.POINTER(C.c_uint64)), n, CLIP_PCM16 if out_pcm16 else CLIP_F32)
        info = (best.ctypes.data_as(C.POINTER(C.c_int32)), fptr(rms), fptr(runner), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                step, None if skips is None else skips.ctypes.data_as(C.POINTER(C.c_uint32)))
        if taps is not None:
            taps = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
            info += (fptr(taps), taps.shape[0])
        res = {"best_channel": best, "best_rms": rms, "runner_up_rms": runner, "offsets": offs, "total": total, "out_lens": out_lens}
        if d_out is not None:
            self._ck(getattr(lib(), name + "_device")(*args, vp(d_out), total if out_capacity is None else out_capacity, *info), name + "_device")
            return res
        out = np.zeros(max(total, 1), np.int16 if out_pcm16 else np.float32)
        self._ck(getattr(lib(), name)(*args, out.ctypes.data, total if out_capacity is None else out_capacity, *info), name)
        res["out"] = out[:total]
        return res

    def _clips_export_resampled(self, name, src_args, clips, lens, out_pcm16, d_out, out_capacity, step, skips, taps, up, down):
        """the four resampled calls: `name` (+ "_device" with d_out), src_args the arguments between ctx and the clips"""
        if up is None or down is None or taps is None or step != 1 or skips is not None:
            raise ValueError("a resampled clip export takes up, down and taps, and neither step nor skips")
        n = clips.shape[0]
        out_lens, offsets, total = clips_plan_resampled(lens, up, down, out_pcm16) if n else (np.zeros(0, np.uint64), None, 0)
        best, rms, runner, offs = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint64)
        taps = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
        args = (self.h, *src_args, clips.ctypes.data_as(C.POINTER(C.c_uint64)), n, CLIP_PCM16 if out_pcm16 else CLIP_F32)
        info = (best.ctypes.data_as(C.POINTER(C.c_int32)), fptr(rms), fptr(runner), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                int(up), int(down), fptr(taps), taps.shape[0])
        res = {"best_channel": best, "best_rms": rms, "runner_up_rms": runner, "offsets": offs, "total": total, "out_lens": out_lens}
        if d_out is not None:
            self._ck(getattr(lib(), name + "_device")(*args, vp(d_out), total if out_capacity is None else out_capacity, *info), name + "_device")
            return res
        out = np.zeros(max(total, 1), np.int16 if out_pcm16 else np.float32)
        self._ck(getattr(lib(), name)(*args, out.ctypes.data, total if out_capacity is None else out_capacity, *info), name)
        res["out"] = out[:total]
        return res

    def clips_export_split(self, a, b, src_pcm16, clips, out_pcm16=False, d_out=None, out_capacity=None, step=1, skips=None, taps=None,
                           up=None, down=None):
        """fvad_clips_export_split (d_out None) or fvad_clips_export_split_device: a and b are the two source buffers as
        (device address or None, n_lanes, lane_stride, n_samples); clips: [n][CLIP_SPLIT_FIELDS] uint64, channel c of a clip
        being a[a_lane + c][a_from, a_from + a_len) followed by b[b_lane + c][b_from, b_from + b_len).  Returns what
        clips_export does; step / skips / taps / up / down as there (fvad_clips_export_split_strided(_device),
        fvad_clips_export_split_fir(_device), fvad_clips_export_split_resampled(_device))."""
        clips = _clip_split_rows(clips)
        n = clips.shape[0]
        if up is not None or down is not None:
            return self._clips_export_resampled("fvad_clips_export_split_resampled", (vp(a[0]), a[1], a[2], a[3], vp(b[0]), b[1], b[2], b[3],
                                                CLIP_PCM16 if src_pcm16 else CLIP_F32), clips, clips[:, 3] + clips[:, 6], out_pcm16, d_out,
                                                out_capacity, step, skips, taps, up, down)
        if step != 1 or skips is not None or taps is not None:
            return self._clips_export_strided("fvad_clips_export_split_fir" if taps is not None else "fvad_clips_export_split_strided", (vp(a[0]), a[1], a[2], a[3], vp(b[0]), b[1], b[2], b[3],
                                              CLIP_PCM16 if src_pcm16 else CLIP_F32), clips, clips[:, 3] + clips[:, 6], out_pcm16, d_out,
                                              out_capacity, step, skips, taps)
        offsets, total = clips_plan([(0, 1, 0, int(r[3]) + int(r[6])) for r in clips], out_pcm16) if n else (None, 0)
        best, rms, runner, offs = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint64)
        args = (self.h, vp(a[0]), a[1], a[2], a[3], vp(b[0]), b[1], b[2], b[3], CLIP_PCM16 if src_pcm16 else CLIP_F32,
                clips.ctypes.data_as(C.POINTER(C.c_uint64)), n, CLIP_PCM16 if out_pcm16 else CLIP_F32)
        info = (best.ctypes.data_as(C.POINTER(C.c_int32)), fptr(rms), fptr(runner), offs.ctypes.data_as(C.POINTER(C.c_uint64)))
        res = {"best_channel": best, "best_rms": rms, "runner_up_rms": runner, "offsets": offs, "total": total}
        if d_out is not None:
            self._ck(lib().fvad_clips_export_split_device(*args, vp(d_out), total if out_capacity is None else out_capacity, *info),
                     "fvad_clips_export_split_device")
            return res
        out = np.zeros(max(total, 1), np.int16 if out_pcm16 else np.float32)
        self._ck(lib().fvad_clips_export_split(*args, out.ctypes.data, total if out_capacity is None else out_capacity, *info),
                 "fvad_clips_export_split")
        res["out"] = out[:total]
        return res

    def ingest(self, sources, out_pcm16=False, d_lanes=None, n_lanes=0, lane_stride=0, n_samples=0, raw=None, raw_bytes=None):
        """fvad_ingest_device (raw: a device address holding raw_bytes bytes) or fvad_ingest (raw: a list with one C-contiguous
        numpy / memmap byte buffer per source, or None for a source without frames; a source's byte_offset is relative to its
        own buffer): sources [n][INGEST_FIELDS] uint64 -> the planar lanes at device address d_lanes (float32, or int16 with
        out_pcm16), n_lanes of n_samples, lane_stride apart.  Returns when the lanes are written."""
        sources = _ingest_rows(sources)
        n = sources.shape[0]
        fmt = INGEST_PCM16 if out_pcm16 else INGEST_F32
        rows = sources.ctypes.data_as(C.POINTER(C.c_uint64))
        if isinstance(raw, (list, tuple)):
            ptrs = _host_buffers("ingest", "source", "reads", sources, raw, writable=False)
            self._ck(lib().fvad_ingest(self.h, ptrs, rows, n, fmt, vp(d_lanes), n_lanes, lane_stride, n_samples), "fvad_ingest")
            return
        self._ck(lib().fvad_ingest_device(self.h, vp(raw), int(raw_bytes or 0), rows, n, fmt, vp(d_lanes), n_lanes, lane_stride,
                                          n_samples), "fvad_ingest_device")

    def ingest_resample(self, sources, up, down, taps, d_lanes=None, n_lanes=0, lane_stride=0, n_samples=0, raw=None, raw_bytes=None):
        """fvad_ingest_resample_device (raw: a device address holding raw_bytes bytes) or fvad_ingest_resample (raw: a list with
        one byte buffer per source, as for `ingest`; a source's byte_offset is where its frame frame_base lies in its own
        buffer): sources [n][RESAMPLE_FIELDS] uint64 of files at 1 / (up / down) of the lanes' rate -> float32 lanes at device
        address d_lanes.  One ratio and one set of taps (float32, an odd count) per call."""
        sources = _resample_rows(sources)
        n = sources.shape[0]
        rows = sources.ctypes.data_as(C.POINTER(C.c_uint64))
        taps = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
        tail = (up, down, fptr(taps), taps.shape[0], vp(d_lanes), n_lanes, lane_stride, n_samples)
        if isinstance(raw, (list, tuple)):
            ptrs = _host_buffers("ingest_resample", "source", "reads", sources, raw, writable=False)
            self._ck(lib().fvad_ingest_resample(self.h, ptrs, rows, n, *tail), "fvad_ingest_resample")
            return
        self._ck(lib().fvad_ingest_resample_device(self.h, vp(raw), int(raw_bytes or 0), rows, n, *tail), "fvad_ingest_resample_device")

    def egress(self, sinks, src_pcm16=False, d_lanes=None, n_lanes=0, lane_stride=0, n_samples=0, out=None, out_bytes=None):
        """fvad_egress_device (out: a device address holding out_bytes bytes) or fvad_egress (out: a list with one writable
        C-contiguous numpy / memmap byte buffer per sink, or None for a sink without frames; a sink's byte_offset is relative to
        its own buffer): sinks [n][EGRESS_FIELDS] uint64 <- the planar lanes at device address d_lanes (float32, or int16 with
        src_pcm16), n_lanes of n_samples, lane_stride apart, converted to each sink's file format and interleaved.  Returns
        when the bytes are written."""
        sinks = _egress_rows(sinks)
        n = sinks.shape[0]
        fmt = INGEST_PCM16 if src_pcm16 else INGEST_F32
        rows = sinks.ctypes.data_as(C.POINTER(C.c_uint64))
        if isinstance(out, (list, tuple)):
            ptrs = _host_buffers("egress", "sink", "writes", sinks, out, writable=True)
            self._ck(lib().fvad_egress(self.h, vp(d_lanes), fmt, n_lanes, lane_stride, n_samples, rows, n, ptrs), "fvad_egress")
            return
        self._ck(lib().fvad_egress_device(self.h, vp(d_lanes), fmt, n_lanes, lane_stride, n_samples, rows, n, vp(out), int(out_bytes or 0)),
                 "fvad_egress_device")

    def egress_mix(self, sinks, w_orig, w_den, d_orig=None, orig_stride=0, orig_samples=0, d_den=None, den_stride=0, den_samples=0, n_lanes=0,
                   src_pcm16=False, out=None, out_bytes=None):
        """fvad_egress_mix_device (out: a device address holding out_bytes bytes) or fvad_egress_mix (out: a list with one
        writable C-contiguous numpy / memmap byte buffer per sink, or None for a sink without frames; a sink's byte_offset is
        relative to its own buffer): sinks [n][EGRESS_MIX_FIELDS] uint64 <- w_orig * the original lanes at device address d_orig
        (n_lanes of orig_samples float32, orig_stride apart) + w_den * the denoised lanes at d_den, converted to each sink's file
        format and interleaved.  The lanes of a zero weight are not read and may be None (src_pcm16 lanes are refused by the
        library).  Returns when the bytes are written."""
        sinks = _egress_mix_rows(sinks)
        n = sinks.shape[0]
        rows = sinks.ctypes.data_as(C.POINTER(C.c_uint64))
        head = (self.h, vp(d_orig), orig_stride, orig_samples, vp(d_den), den_stride, den_samples, INGEST_PCM16 if src_pcm16 else INGEST_F32,
                n_lanes, float(w_orig), float(w_den), rows, n)
        if isinstance(out, (list, tuple)):
            ptrs = _host_buffers("egress_mix", "sink", "writes", sinks, out, writable=True)
            self._ck(lib().fvad_egress_mix(*head, ptrs), "fvad_egress_mix")
            return
        self._ck(lib().fvad_egress_mix_device(*head, vp(out), int(out_bytes or 0)), "fvad_egress_mix_device")

    def egress_resample(self, sinks, up, down, taps, src_pcm16=False, d_lanes=None, n_lanes=0, lane_stride=0, n_samples=0, out=None, out_bytes=None):
        """fvad_egress_resample_device (out: a device address holding out_bytes bytes) or fvad_egress_resample (out: a list with
        one writable C-contiguous numpy / memmap byte buffer per row, or None for a row without outputs; a row's byte_offset is
        relative to its own buffer): sinks [n][EGRESS_RESAMPLE_FIELDS] uint64 <- the planar float32 lanes at device address
        d_lanes, resampled by up / down with `taps` (float32, an odd count), converted to each row's file format and
        interleaved.  One ratio and one set of taps per call (src_pcm16 lanes are refused by the library).  Returns when the
        bytes are written."""
        self._egress_resample("fvad_egress_resample", (), sinks, up, down, taps, src_pcm16, d_lanes, n_lanes, lane_stride, n_samples, out, out_bytes)

    def egress_resample_strided(self, sinks, up, down, taps, src_step, src_pcm16=False, d_lanes=None, n_lanes=0, lane_stride=0, n_samples=0, out=None,
                                out_bytes=None):
        """fvad_egress_resample_strided_device / fvad_egress_resample_strided: egress_resample over the stream that lies src_step
        (1 .. EGRESS_STEP_MAX) apart in the lanes: stream sample n of a row is lane sample src_offset + (n - frame_base) * src_step,
        and the row's stream_frames, out_from, frame_base and n_frames count strided samples."""
        self._egress_resample("fvad_egress_resample_strided", (int(src_step),), sinks, up, down, taps, src_pcm16, d_lanes, n_lanes, lane_stride,
                              n_samples, out, out_bytes)

    def _egress_resample(self, name, step, sinks, up, down, taps, src_pcm16, d_lanes, n_lanes, lane_stride, n_samples, out, out_bytes):
        """the two call forms of egress_resample and egress_resample_strided (step: () or (src_step,), behind the taps)"""
        sinks = _egress_resample_rows(sinks)
        n = sinks.shape[0]
        fmt = INGEST_PCM16 if src_pcm16 else INGEST_F32
        rows = sinks.ctypes.data_as(C.POINTER(C.c_uint64))
        taps = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
        head = (self.h, vp(d_lanes), fmt, n_lanes, lane_stride, n_samples, rows, n, up, down, fptr(taps), taps.shape[0]) + step
        if isinstance(out, (list, tuple)):
            ptrs = _host_buffers("egress_resample", "row", "writes", sinks, out, writable=True, where=name)
            self._ck(getattr(lib(), name)(*head, ptrs), name)
            return
        self._ck(getattr(lib(), name + "_device")(*head, vp(out), int(out_bytes or 0)), name + "_device")

    def lane_state(self):
        s = vp()
        self._ck(lib().fvad_lane_state_create(self.h, C.byref(s)), "fvad_lane_state_create")
        return s


class FFT:
    """fvad_fft <-> reference src/FFT.zig"""

    def __init__(self, ctx, n_fft, sample_rate, inverse=False):
        self.ctx = ctx
        self.h = vp()
        ctx._ck(lib().fvad_fft_create(ctx.h, n_fft, sample_rate, 1 if inverse else 0,
                                      C.byref(self.h)), "FFT.init")
        self.n_fft = n_fft

    def bin_count(self):
        return lib().fvad_fft_bin_count(self.h)

    def fft(self, first, window, second=None, n_bins=None):
        first = np.ascontiguousarray(first, np.float32)
        second = np.ascontiguousarray(second, np.float32) if second is not None else None
        window = np.ascontiguousarray(window, np.float32)
        nb = self.bin_count() if n_bins is None else n_bins
        out = np.zeros((nb, 2), np.float32)
        rc = lib().fvad_fft_forward(self.h, fptr(first), first.shape[0],
                                    fptr(second) if second is not None else None,
                                    0 if second is None else second.shape[0],
                                    fptr(window), window.shape[0],
                                    out.ctypes.data_as(C.POINTER(Complex)), nb)
        self.ctx._ck(rc, "FFT.fft")
        return out.view(np.complex64)[:, 0]

    def inv_fft(self, bins, n_result=None):
        b = np.ascontiguousarray(np.asarray(bins, np.complex64)).view(np.float32).reshape(-1, 2)
        n = self.n_fft if n_result is None else n_result
        out = np.zeros(n, np.float32)
        rc = lib().fvad_fft_inverse(self.h, b.ctypes.data_as(C.POINTER(Complex)), b.shape[0],
                                    fptr(out), n)
        self.ctx._ck(rc, "FFT.invFft")
        return out

    def fft_batch(self, frames, window, want_bins=True, want_mag=True):
        frames = np.ascontiguousarray(frames, np.float32)
        window = np.ascontiguousarray(window, np.float32)
        nb = self.bin_count()
        bins = np.zeros((frames.shape[0], nb, 2), np.float32) if want_bins else None
        mag = np.zeros((frames.shape[0], nb), np.float32) if want_mag else None
        rc = lib().fvad_fft_forward_batch(
            self.h, frames.ctypes.data, frames.shape[0], window.ctypes.data,
            bins.ctypes.data if bins is not None else None,
            mag.ctypes.data if mag is not None else None, 0)
        self.ctx._ck(rc, "FFT.fft(batch)")
        return (bins.view(np.complex64)[..., 0] if bins is not None else None), mag

    def freq_to_bin(self, freq):
        b = sz()
        rc = lib().fvad_fft_freq_to_bin(self.h, freq, C.byref(b))
        if rc != FVAD_OK:
            raise FvadError(rc, "FFT.freqToBin")
        return b.value

    def close(self):
        if self.h:
            lib().fvad_fft_destroy(self.h)
            self.h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NSNet2:
    """fvad_nsnet2 <-> reference src/NSNet2.zig (one object per channel)"""

    def __init__(self, ctx, sample_rate=48000):
        self.ctx = ctx
        self.h = vp()
        ctx._ck(lib().fvad_nsnet2_create(ctx.h, sample_rate, C.byref(self.h)), "NSNet2.init")
        self.chunk = lib().fvad_nsnet2_chunk_size(sample_rate)

    def denoise(self, x, split=None):
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros(self.chunk, np.float32)
        if split is None:
            rc = lib().fvad_nsnet2_denoise(self.h, fptr(x), x.shape[0], None, 0, fptr(out),
                                           out.shape[0])
        else:
            a, b = np.ascontiguousarray(x[:split]), np.ascontiguousarray(x[split:])
            rc = lib().fvad_nsnet2_denoise(self.h, fptr(a), a.shape[0], fptr(b), b.shape[0],
                                           fptr(out), out.shape[0])
        self.ctx._ck(rc, "NSNet2.denoise")
        return out

    def close(self):
        if self.h:
            lib().fvad_nsnet2_destroy(self.h)
            self.h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AudioPipeline:
    """fvad_pipeline <-> reference src/AudioPipeline.zig"""

    def __init__(self, ctx, n_channels=1, sample_rate=48000, fft_size=1024, vad_overrides=None,
                 alt_configs=None, skip_processing=False, record=False, trace=True, buffer_length=0):
        self.ctx = ctx
        cfg = PipelineConfig()
        lib().fvad_pipeline_config_default(C.byref(cfg))
        cfg.buffer_length = buffer_length
        cfg.n_channels = n_channels
        cfg.sample_rate = sample_rate
        cfg.fft_size = fft_size
        cfg.skip_processing = 1 if skip_processing else 0
        for k, v in (vad_overrides or {}).items():
            setattr(cfg.vad_machine_config, k, v)
        self._alts = None
        if alt_configs:
            self._alts = (VadConfig * len(alt_configs))()
            for i, ov in enumerate(alt_configs):
                lib().fvad_vad_config_default(C.byref(self._alts[i]))
                for k, v in ov.items():
                    setattr(self._alts[i], k, v)
            cfg.alt_vad_machine_configs = self._alts
            cfg.n_alt_vad_machine_configs = len(alt_configs)
        self.h = vp()
        self.recordings = {"original": [], "denoised": []}
        cbs = None
        if record:
            def mk(kind):
                def cb(_ctx, ab):
                    a = ab.contents
                    assert a.n_channels == 1
                    pcm = np.ctypeslib.as_array(a.channel_pcm[0], shape=(a.length,)).copy()
                    self.recordings[kind].append((a.global_start_frame_number, pcm, a.duration_seconds))
                return RecordingCb(cb)
            self._cb_keep = (mk("original"), mk("denoised"))
            self._cbs = Callbacks(None, self._cb_keep[0], self._cb_keep[1])
            cbs = C.byref(self._cbs)
        ctx._ck(lib().fvad_pipeline_create(ctx.h, C.byref(cfg), cbs, C.byref(self.h)),
                "AudioPipeline.init")
        if trace:   # per-frame band sums / ratios for parity tests (the library keeps none by default)
            lib().fvad_pipeline_enable_trace(self.h, 1)
        self.n_channels = n_channels

    def push_samples(self, pcm):
        pcm = np.ascontiguousarray(pcm, np.float32)
        assert pcm.ndim == 2 and pcm.shape[0] == self.n_channels
        ptrs = (c_float_p * self.n_channels)(*[fptr(pcm[c]) for c in range(self.n_channels)])
        first = C.c_uint64()
        self.ctx._ck(lib().fvad_pipeline_push_samples(self.h, ptrs, pcm.shape[1], C.byref(first)),
                     "AudioPipeline.pushSamples")
        return first.value

    def segments(self, alt=None):
        n = sz()
        cap = 4096
        buf = (SpeechSegment * cap)()
        if alt is None:
            rc = lib().fvad_pipeline_segments(self.h, buf, cap, C.byref(n))
        else:
            rc = lib().fvad_pipeline_alt_segments(self.h, alt, buf, cap, C.byref(n))
        self.ctx._ck(rc, "vad_segments")
        return [(buf[i].sample_from, buf[i].sample_to, buf[i].avg_channel_vol_ratio,
                 buf[i].vad_met_sec) for i in range(n.value)]

    def trace(self):
        n = lib().fvad_pipeline_n_fft_frames(self.h)
        band = np.zeros((max(n, 1), self.n_channels), np.float32)
        ratio = np.zeros(max(n, 1), np.float32)
        self.ctx._ck(lib().fvad_pipeline_trace(self.h, fptr(band), fptr(ratio), max(n, 1)),
                     "trace")
        return band[:n], ratio[:n]

    def audit(self):
        a = VadAudit()
        self.ctx._ck(lib().fvad_pipeline_audit(self.h, C.byref(a)), "audit")
        return a.min_rel_threshold_margin, a.min_abs_ratio_margin, a.n_frames

    def close(self):
        if self.h:
            lib().fvad_pipeline_destroy(self.h)
            self.h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VadMachine:
    """fvad_vad <-> reference src/AudioPipeline/VADMachine.zig (host)"""

    def __init__(self, n_channels=1, sample_rate=48000, fft_size=1024, overrides=None):
        cfg = VadConfig()
        lib().fvad_vad_config_default(C.byref(cfg))
        for k, v in (overrides or {}).items():
            setattr(cfg, k, v)
        self.h = vp()
        check(lib().fvad_vad_create(C.byref(cfg), sample_rate, n_channels, fft_size,
                                    C.byref(self.h)), "VADMachine.init")
        self.n_channels = n_channels

    def run(self, index, volumes, ratio):
        v = np.ascontiguousarray(volumes, np.float32)
        res = VadResult()
        has = 0 if ratio is None else 1
        check(lib().fvad_vad_run(self.h, index, fptr(v), has, 0.0 if ratio is None else ratio,
                                 C.byref(res)), "VADMachine.run")
        return res.recording_state, res.sample_number

    def segments(self):
        n = sz()
        cap = max(1, lib().fvad_vad_segment_count(self.h))
        buf = (SpeechSegment * cap)()
        check(lib().fvad_vad_segments(self.h, buf, cap, C.byref(n)), "vad_segments")
        return [(buf[i].sample_from, buf[i].sample_to, buf[i].avg_channel_vol_ratio,
                 buf[i].vad_met_sec) for i in range(n.value)]

    def audit(self):
        a = VadAudit()
        check(lib().fvad_vad_audit_get(self.h, C.byref(a)), "audit")
        return a.min_rel_threshold_margin, a.min_abs_ratio_margin, a.n_frames

    def lazy_stats(self):
        """(exact evaluations of the long-term chain, pushes absorbed lazily)"""
        e, p = C.c_uint64(), C.c_uint64()
        check(lib().fvad_vad_lazy_stats(self.h, C.byref(e), C.byref(p)), "lazy_stats")
        return e.value, p.value

    def close(self):
        if self.h:
            lib().fvad_vad_destroy(self.h)
            self.h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VadBatch:
    """fvad_vad_batch: the host stage (frame metadata + VAD state machines) for many streams in one call"""

    def __init__(self, n_streams, n_channels=1, sample_rate=48000, fft_size=1024, overrides=None):
        cfg = VadConfig()
        lib().fvad_vad_config_default(C.byref(cfg))
        for k, v in (overrides or {}).items():
            setattr(cfg, k, v)
        self.h = vp()
        check(lib().fvad_vad_batch_create(C.byref(cfg), sample_rate, n_channels, fft_size, n_streams, C.byref(self.h)),
              "fvad_vad_batch_create")
        self.n_streams, self.n_channels = n_streams, n_channels

    def run(self, band, chunk_rms, n_threads=1, chunk_size=24000):
        """band [n_streams * n_channels][n_frames], chunk_rms [n_streams * n_channels][n_chunks] (float32, C order)
        -> list of per-stream segment lists [(from, to, avg_ratio, vad_met_sec)]"""
        assert band.dtype == np.float32 and chunk_rms.dtype == np.float32 and band.flags["C_CONTIGUOUS"] and chunk_rms.flags["C_CONTIGUOUS"]
        assert band.shape[0] == chunk_rms.shape[0] == self.n_streams * self.n_channels
        check(lib().fvad_vad_batch_run(self.h, fptr(band), band.shape[1], band.shape[1], fptr(chunk_rms), chunk_rms.shape[1],
                                       chunk_rms.shape[1], chunk_size, n_threads), "fvad_vad_batch_run")
        n = lib().fvad_vad_batch_total_segments(self.h)
        arr = (SpeechSegment * max(n, 1))()
        offs = (sz * (self.n_streams + 1))()
        check(lib().fvad_vad_batch_segments(self.h, arr, max(n, 1), offs), "fvad_vad_batch_segments")
        flat = [(a.sample_from, a.sample_to, a.avg_channel_vol_ratio, a.vad_met_sec) for a in arr[:n]]
        return [flat[offs[s]:offs[s + 1]] for s in range(self.n_streams)]

    def _segments(self):
        n = lib().fvad_vad_batch_total_segments(self.h)
        arr = (SpeechSegment * max(n, 1))()
        offs = (sz * (self.n_streams + 1))()
        check(lib().fvad_vad_batch_segments(self.h, arr, max(n, 1), offs), "fvad_vad_batch_segments")
        flat = [(a.sample_from, a.sample_to, a.avg_channel_vol_ratio, a.vad_met_sec) for a in arr[:n]]
        return [flat[offs[s]:offs[s + 1]] for s in range(self.n_streams)]

    def run_part(self, band, chunk_rms, first_frame, n_threads=1, chunk_size=24000, want_segments=True):
        """fvad_vad_batch_run_part: `band` [lanes][n_frames] holds the frames from `first_frame` on, `chunk_rms` [lanes][n_chunks] the
        chunks from the one that frame starts in (float32 views with a contiguous last axis: nothing is copied; a part off the
        chunk grid is refused by the library).  -> the segments of everything run so far (or None)."""
        assert band.dtype == np.float32 and chunk_rms.dtype == np.float32
        assert (band.shape[1] <= 1 or band.strides[1] == 4) and (chunk_rms.shape[1] <= 1 or chunk_rms.strides[1] == 4)
        assert band.shape[0] == chunk_rms.shape[0] == self.n_streams * self.n_channels
        bp = C.cast(band.ctypes.data, c_float_p)
        rp = C.cast(chunk_rms.ctypes.data, c_float_p)
        check(lib().fvad_vad_batch_run_part(self.h, bp, band.strides[0] // 4, band.shape[1], rp, chunk_rms.strides[0] // 4, chunk_rms.shape[1],
                                            chunk_size, first_frame, n_threads), "fvad_vad_batch_run_part")
        return self._segments() if want_segments else None

    def hold_from(self):
        """fvad_vad_batch_hold_from: per stream the smallest sample_from a segment not yet reported can still get --
        the audio a run sliced in time must keep.  Defined after host runs only."""
        out = (C.c_uint64 * self.n_streams)()
        st = lib().fvad_vad_batch_hold_from(self.h, 0, out)
        if st == FVAD_ERR_INVALID_ARGUMENT:
            raise FvadError(st, "fvad_vad_batch_hold_from", "a bad config, a part in flight, or the last run was a device run: "
                            "the machines' state is not on the host")
        check(st, "fvad_vad_batch_hold_from")
        return list(out)

    def audit(self, stream):
        a = VadAudit()
        check(lib().fvad_vad_batch_audit(self.h, stream, C.byref(a)), "fvad_vad_batch_audit")
        return a.min_rel_threshold_margin, a.min_abs_ratio_margin, a.n_frames

    def close(self):
        if self.h:
            lib().fvad_vad_batch_destroy(self.h)
            self.h = vp()


def _config_array(configs):
    """the VadConfig array of a list of override dicts (defaults for the fields a dict leaves out)"""
    arr = (VadConfig * len(configs))()
    for i, ov in enumerate(configs):
        lib().fvad_vad_config_default(C.byref(arr[i]))
        for k, v in (ov or {}).items():
            setattr(arr[i], k, v)
    return arr


class VadSweep:
    """fvad_vad_batch with several configs (fvad_vad_batch_create_sweep): one VAD machine per (stream, config), each on its
    config's speech band.  configs: list of VadConfig overrides dicts (defaults for the fields a dict leaves out).  sizes (the
    distinct frame sizes, here [fft_size]) and size_of_band (each band's index into sizes) are those of frame_sizes()."""

    def __init__(self, n_streams, configs, n_channels=1, sample_rate=48000, fft_size=1024):
        self.h = vp()
        check(lib().fvad_vad_batch_create_sweep(_config_array(configs), len(configs), sample_rate, n_channels, fft_size, n_streams,
                                                C.byref(self.h)), "fvad_vad_batch_create_sweep")
        self._created(n_streams, n_channels, len(configs))

    def _created(self, n_streams, n_channels, n_configs):
        self.n_streams, self.n_channels, self.n_configs = n_streams, n_channels, n_configs
        assert lib().fvad_vad_batch_n_configs(self.h) == self.n_configs
        self.sizes, self.size_of_band = self.frame_sizes()

    def frame_sizes(self):
        """-> (the distinct sizes in first-seen config order, the size index of each band)"""
        n = sz()
        sizes = (sz * self.n_configs)()
        sob = (C.c_uint32 * self.n_configs)()
        check(lib().fvad_vad_batch_frame_sizes(self.h, sizes, self.n_configs, C.byref(n), sob), "fvad_vad_batch_frame_sizes")
        n_bands = sz()
        lib().fvad_vad_batch_bands(self.h, None, 0, C.byref(n_bands), None)
        return [sizes[g] for g in range(n.value)], [sob[j] for j in range(n_bands.value)]

    def bands(self):
        """-> (bins [(min_bin, max_bin)] of the distinct bands, band_of [config])"""
        n = sz()
        cap = 2 * self.n_configs
        bins = (C.c_int32 * cap)()
        band_of = (C.c_uint32 * self.n_configs)()
        check(lib().fvad_vad_batch_bands(self.h, bins, self.n_configs, C.byref(n), band_of), "fvad_vad_batch_bands")
        return [(bins[2 * j], bins[2 * j + 1]) for j in range(n.value)], list(band_of)

    def size_blocks(self):
        """-> [(fft_size, first band, [(min_bin, max_bin)])] per size: the run of band blocks of each size"""
        bins, _ = VadSweep.bands(self)
        out = []
        for g, F in enumerate(self.sizes):
            js = [j for j in range(len(bins)) if self.size_of_band[j] == g]
            out.append((F, js[0], [bins[j] for j in js]))
        return out

    def run(self, band, chunk_rms, n_threads=1, chunk_size=24000):
        """band [n_bands][n_streams * n_channels][n_frames] (bands() order), chunk_rms [n_streams * n_channels][n_chunks], float32"""
        assert band.dtype == np.float32 and chunk_rms.dtype == np.float32 and band.flags["C_CONTIGUOUS"] and chunk_rms.flags["C_CONTIGUOUS"]
        assert band.shape[1] == chunk_rms.shape[0] == self.n_streams * self.n_channels
        check(lib().fvad_vad_batch_run(self.h, fptr(band), band.shape[2], band.shape[2], fptr(chunk_rms), chunk_rms.shape[1],
                                       chunk_rms.shape[1], chunk_size, n_threads), "fvad_vad_batch_run")

    def run_sized(self, band, chunk_rms, n_frames, first_sample=0, n_threads=1, chunk_size=24000):
        """fvad_vad_batch_run_sized: band [n_bands][n_streams * n_channels][stride] (bands() order, C-contiguous),
        n_frames[g] frames of size g (one size: the count itself will do) from sample first_sample on, chunk_rms [lanes][n_chunks]
        from the part's first chunk.  first_sample = 0 starts fresh machines; a later part goes on where the last one ended."""
        assert band.dtype == np.float32 and chunk_rms.dtype == np.float32
        assert band.flags["C_CONTIGUOUS"]   # (not by the strides: numpy leaves an axis of length 1 whatever stride it had)
        assert chunk_rms.shape[1] <= 1 or chunk_rms.strides[1] == 4
        assert band.shape[1] == chunk_rms.shape[0] == self.n_streams * self.n_channels
        n_frames = [int(x) for x in np.atleast_1d(n_frames)]
        assert len(n_frames) == len(self.sizes)
        nf = (sz * len(n_frames))(*n_frames)
        check(lib().fvad_vad_batch_run_sized(self.h, C.cast(band.ctypes.data, c_float_p), band.shape[2], nf,
                                             C.cast(chunk_rms.ctypes.data, c_float_p), chunk_rms.strides[0] // 4, chunk_rms.shape[1],
                                             chunk_size, int(first_sample), n_threads), "fvad_vad_batch_run_sized")

    def run_device(self, ctx, d_band, band_stride, n_frames, chunk_rms, n_chunks, chunk_size=24000):
        """fvad_vad_batch_run_device: d_band as Context.band_sums_device writes it (device address), n_frames / n_chunks per
        stream, chunk_rms [n_streams * n_channels][>= max n_chunks] float32 on the host"""
        assert chunk_rms.dtype == np.float32 and chunk_rms.flags["C_CONTIGUOUS"] and chunk_rms.shape[0] == self.n_streams * self.n_channels
        nf = (sz * self.n_streams)(*[int(x) for x in n_frames])
        nc = (sz * self.n_streams)(*[int(x) for x in n_chunks])
        ctx._ck(lib().fvad_vad_batch_run_device(ctx.h, self.h, vp(d_band), band_stride, nf, fptr(chunk_rms), chunk_rms.shape[1], nc,
                                                chunk_size), "fvad_vad_batch_run_device")

    def run_device_part(self, ctx, d_band, band_stride, n_frames, chunk_rms, n_chunks, first_frame, chunk_size=24000):
        """fvad_vad_batch_run_device_part: frames [first_frame, first_frame + n_frames[s]) of every stream, the machines' state
        kept in device memory between the parts; d_band / chunk_rms hold the part's frames / chunks as run_device takes them.
        first_frame = 0 starts fresh machines.  After each part, segments (keep_segments on), audits and lazy statistics cover
        everything run so far."""
        assert chunk_rms.dtype == np.float32 and chunk_rms.flags["C_CONTIGUOUS"] and chunk_rms.shape[0] == self.n_streams * self.n_channels
        nf = (sz * self.n_streams)(*[int(x) for x in n_frames])
        nc = (sz * self.n_streams)(*[int(x) for x in n_chunks])
        ctx._ck(lib().fvad_vad_batch_run_device_part(ctx.h, self.h, vp(d_band) if d_band else None, band_stride, nf, fptr(chunk_rms),
                                                     chunk_rms.shape[1], nc, chunk_size, int(first_frame)),
                "fvad_vad_batch_run_device_part")

    def _sized_counts(self, n_frames, n_chunks):
        """n_frames [stream] (one size) or [size][stream], n_chunks [stream] as the sized calls take them"""
        flat = [int(x) for row in n_frames for x in (row if hasattr(row, "__len__") else [row])]
        assert len(flat) == len(self.sizes) * self.n_streams and len(n_chunks) == self.n_streams
        return (sz * len(flat))(*flat), (sz * self.n_streams)(*[int(x) for x in n_chunks])

    def run_device_sized(self, ctx, d_band, band_stride, n_frames, chunk_rms, n_chunks, chunk_size=24000):
        """fvad_vad_batch_run_device_sized: run_device with n_frames [stream] (one size) or [size][stream]; d_band as bands()
        orders the blocks"""
        assert chunk_rms.dtype == np.float32 and chunk_rms.flags["C_CONTIGUOUS"] and chunk_rms.shape[0] == self.n_streams * self.n_channels
        nf, nc = self._sized_counts(n_frames, n_chunks)
        ctx._ck(lib().fvad_vad_batch_run_device_sized(ctx.h, self.h, vp(d_band), band_stride, nf, fptr(chunk_rms), chunk_rms.shape[1], nc,
                                                      chunk_size), "fvad_vad_batch_run_device_sized")

    def run_device_part_sized(self, ctx, d_band, band_stride, n_frames, chunk_rms, n_chunks, first_sample, chunk_size=24000):
        """fvad_vad_batch_run_device_part_sized: run_device_part in samples -- the frames of every size from sample first_sample on,
        n_frames [stream] (one size) or [size][stream]"""
        assert chunk_rms.dtype == np.float32 and chunk_rms.flags["C_CONTIGUOUS"] and chunk_rms.shape[0] == self.n_streams * self.n_channels
        nf, nc = self._sized_counts(n_frames, n_chunks)
        ctx._ck(lib().fvad_vad_batch_run_device_part_sized(ctx.h, self.h, vp(d_band) if d_band else None, band_stride, nf,
                                                           fptr(chunk_rms), chunk_rms.shape[1], nc, chunk_size, int(first_sample)),
                "fvad_vad_batch_run_device_part_sized")

    def run_device_part_async(self, ctx, d_band, band_stride, n_frames, d_chunk_rms, rms_stride, n_chunks, first_sample, chunk_size=24000):
        """fvad_vad_batch_run_device_part_async: the sized part call (n_frames [stream] with one size, else [size][stream]) with
        the chunk RMS on the device (lane l's chunks at d_chunk_rms + 4 * l * rms_stride); returns once the part is queued on the
        context's second stream.  d_band and d_chunk_rms stay untouched, and the batch is not to be used, until part_wait."""
        nf, nc = self._sized_counts(n_frames, n_chunks)
        ctx._ck(lib().fvad_vad_batch_run_device_part_async(ctx.h, self.h, vp(d_band) if d_band else None, band_stride, nf,
                                                           vp(d_chunk_rms) if d_chunk_rms else None, rms_stride, nc, chunk_size,
                                                           int(first_sample)), "fvad_vad_batch_run_device_part_async")

    def part_wait(self, ctx):
        """fvad_vad_batch_part_wait: finish the part run_device_part_async started (nothing in flight: nothing to do)"""
        ctx._ck(lib().fvad_vad_batch_part_wait(ctx.h, self.h), "fvad_vad_batch_part_wait")

    def frame_ratios_device(self, ctx, d_chunk_rms, rms_stride, n_frames, n_chunks, first_sample, d_ratio, ratio_stride, chunk_size=24000):
        """fvad_vad_batch_frame_ratios_device: the frame ratios a device part computes, row (size, stream) at
        d_ratio + 4 * row * ratio_stride"""
        nf, nc = self._sized_counts(n_frames, n_chunks)
        ctx._ck(lib().fvad_vad_batch_frame_ratios_device(ctx.h, self.h, vp(d_chunk_rms), rms_stride, nf, nc, chunk_size, int(first_sample),
                                                         vp(d_ratio), ratio_stride), "fvad_vad_batch_frame_ratios_device")

    def frame_ratios(self, chunk_rms, n_frames, n_chunks, first_sample=0, chunk_size=24000):
        """fvad_vad_batch_frame_ratios: the same rows on the host from chunk_rms [lanes][chunks] -> float32 [rows][max frames]"""
        assert chunk_rms.dtype == np.float32 and chunk_rms.flags["C_CONTIGUOUS"] and chunk_rms.shape[0] == self.n_streams * self.n_channels
        nf, nc = self._sized_counts(n_frames, n_chunks)
        out = np.zeros((len(nf), max(1, max(nf))), np.float32)
        check(lib().fvad_vad_batch_frame_ratios(self.h, fptr(chunk_rms), chunk_rms.shape[1], nf, nc, chunk_size, int(first_sample),
                                                fptr(out), out.shape[1]), "fvad_vad_batch_frame_ratios")
        return out

    def score_device(self, ctx):
        """fvad_vad_batch_score_device: score the segments the device parts left on the device (keep_segments off); read the
        statistics with config_stats"""
        ctx._ck(lib().fvad_vad_batch_score_device(ctx.h, self.h), "fvad_vad_batch_score_device")

    def device_bytes(self):
        """fvad_vad_batch_device_bytes: device memory the batch holds between device parts (0 when it holds none)"""
        return lib().fvad_vad_batch_device_bytes(self.h)

    def chain_form(self):
        """fvad_vad_batch_chain_form: 0 before the first device launch, 1 when the last device launch ran the lane form of the
        machines' kernel, 2 when it ran the cooperative form (context option vad_chain)"""
        f = C.c_int(0)
        rc = lib().fvad_vad_batch_chain_form(self.h, C.byref(f))
        if rc:
            raise FvadError(rc, "fvad_vad_batch_chain_form")
        return f.value

    def avgs_form(self):
        """fvad_vad_batch_avgs_form: 0 before the first device launch, 1 when the last device launch pushed the short-term and
        channel-ratio rings, 2 when it read them from the tables (context option vad_avgs)"""
        f = C.c_int(0)
        rc = lib().fvad_vad_batch_avgs_form(self.h, C.byref(f))
        if rc:
            raise FvadError(rc, "fvad_vad_batch_avgs_form")
        return f.value

    def avgs_bytes(self):
        """fvad_vad_batch_avgs_bytes: the tables and min_volume rows of the last device launch's part (0 with the rings)"""
        return lib().fvad_vad_batch_avgs_bytes(self.h)

    def avg_keys(self):
        """fvad_vad_batch_avg_keys -> (short keys [(band, ring length)], ratio keys [(size index, ring length)], st_key [config],
        cr_key [config]), the keys in first-seen config order"""
        n_st, n_cr = sz(), sz()
        cap = self.n_configs
        st, cr = (C.c_uint32 * (2 * cap))(), (C.c_uint32 * (2 * cap))()
        st_key, cr_key = (C.c_uint32 * cap)(), (C.c_uint32 * cap)()
        check(lib().fvad_vad_batch_avg_keys(self.h, st, cr, cap, C.byref(n_st), C.byref(n_cr), st_key, cr_key), "fvad_vad_batch_avg_keys")
        return ([(st[2 * j], st[2 * j + 1]) for j in range(n_st.value)], [(cr[2 * j], cr[2 * j + 1]) for j in range(n_cr.value)],
                list(st_key), list(cr_key))

    def trigger_keys(self):
        """fvad_vad_batch_trigger_keys -> (key_of [config], rep [key]): each config's trigger key in first-seen config order and
        each key's first config (context option vad_trigger)"""
        n = sz()
        key_of, rep = (C.c_uint32 * self.n_configs)(), (C.c_uint32 * self.n_configs)()
        check(lib().fvad_vad_batch_trigger_keys(self.h, key_of, self.n_configs, C.byref(n), rep), "fvad_vad_batch_trigger_keys")
        return list(key_of), [rep[k] for k in range(n.value)]

    def trigger_form(self):
        """fvad_vad_batch_trigger_form: 0 before a device launch, 1 per-config machines, 2 shared triggers"""
        f = C.c_int()
        check(lib().fvad_vad_batch_trigger_form(self.h, C.byref(f)), "fvad_vad_batch_trigger_form")
        return f.value

    def trigger_bytes(self):
        """fvad_vad_batch_trigger_bytes: the bits of the last shared part"""
        return lib().fvad_vad_batch_trigger_bytes(self.h)

    def trigger_launches(self):
        """fvad_vad_batch_trigger_launches -> (emitting machines' launches, finishing launches), cumulative, shared form"""
        m, f = C.c_uint64(), C.c_uint64()
        check(lib().fvad_vad_batch_trigger_launches(self.h, C.byref(m), C.byref(f)), "fvad_vad_batch_trigger_launches")
        return m.value, f.value

    def trigger_bits(self, ctx, n_words):
        """fvad_vad_batch_trigger_bits (a test tap): the last shared part's bits -> uint64 [key][stream][n_words]"""
        n_keys = len(self.trigger_keys()[1])
        out = np.zeros((n_keys, self.n_streams, int(n_words)), np.uint64)
        ctx._ck(lib().fvad_vad_batch_trigger_bits(ctx.h, self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), int(n_words)),
                "fvad_vad_batch_trigger_bits")
        return out

    def averages_device(self, ctx, d_band, band_stride, n_frames, chunk_rms, n_chunks, first_sample=0, chunk_size=24000):
        """fvad_vad_batch_averages_device (a test tap): only the averages' table kernels for the frames a part call with these
        arguments would run (n_frames [stream] with one size, else [size][stream]; chunk_rms on the host) -> dict(st float64
        [short key][stream][max frames], cr [ratio key][stream][max frames] -- entries past a stream's frames are NaN --, and
        avg_keys()' st_keys, cr_keys, st_key, cr_key).  first_sample > 0 reads the earlier frames from the batch's part state."""
        assert chunk_rms.dtype == np.float32 and chunk_rms.flags["C_CONTIGUOUS"] and chunk_rms.shape[0] == self.n_streams * self.n_channels
        nf, nc = self._sized_counts(n_frames, n_chunks)
        st_keys, cr_keys, st_key, cr_key = self.avg_keys()
        stride = max(1, max(nf))
        st = np.full((len(st_keys), self.n_streams, stride), np.nan, np.float64)
        cr = np.full((len(cr_keys), self.n_streams, stride), np.nan, np.float64)
        dp = C.POINTER(C.c_double)
        ctx._ck(lib().fvad_vad_batch_averages_device(ctx.h, self.h, vp(d_band) if d_band else None, band_stride, nf, fptr(chunk_rms),
                                                     chunk_rms.shape[1], nc, chunk_size, int(first_sample), st.ctypes.data_as(dp),
                                                     cr.ctypes.data_as(dp), stride), "fvad_vad_batch_averages_device")
        return {"st": st, "cr": cr, "st_keys": st_keys, "cr_keys": cr_keys, "st_key": st_key, "cr_key": cr_key}

    def retain(self, ctx, keep):
        """fvad_vad_batch_retain_configs: keep configs keep (strictly increasing indices) and drop the rest, between runs or
        device parts; new config c is old config keep[c].  ctx: the parts' Context when the batch holds device part state,
        else None or any Context"""
        keep = [int(k) for k in keep]
        arr = (C.c_uint32 * max(len(keep), 1))(*keep)
        if ctx is None:
            check(lib().fvad_vad_batch_retain_configs(None, self.h, arr, len(keep)), "fvad_vad_batch_retain_configs")
        else:
            ctx._ck(lib().fvad_vad_batch_retain_configs(ctx.h, self.h, arr, len(keep)), "fvad_vad_batch_retain_configs")
        self.n_configs = len(keep)
        self.sizes, self.size_of_band = self.frame_sizes()

    def segments(self, config):
        """config's segments per stream: [[(from, to, avg_ratio, vad_met_sec)]]"""
        offs = (sz * (self.n_streams + 1))()
        st = lib().fvad_vad_batch_config_segments(self.h, config, None, 0, offs)
        n = offs[self.n_streams]
        if st != FVAD_OK and not (st == FVAD_ERR_BUFFER_TOO_SMALL and n > 0):
            check(st, "fvad_vad_batch_config_segments")
        arr = (SpeechSegment * max(n, 1))()
        check(lib().fvad_vad_batch_config_segments(self.h, config, arr, max(n, 1), offs), "fvad_vad_batch_config_segments")
        flat = [(a.sample_from, a.sample_to, a.avg_channel_vol_ratio, a.vad_met_sec) for a in arr[:n]]
        return [flat[offs[s]:offs[s + 1]] for s in range(self.n_streams)]

    def hold_from(self, config=0):
        """fvad_vad_batch_hold_from: per stream the smallest sample_from a segment not yet reported by `config`'s machines can still get --
        the audio a run sliced in time must keep.  Defined after host runs only."""
        out = (C.c_uint64 * self.n_streams)()
        st = lib().fvad_vad_batch_hold_from(self.h, config, out)
        if st == FVAD_ERR_INVALID_ARGUMENT:
            raise FvadError(st, "fvad_vad_batch_hold_from", "a bad config, a part in flight, or the last run was a device run: "
                            "the machines' state is not on the host")
        check(st, "fvad_vad_batch_hold_from")
        return list(out)

    def audit(self, stream, config):
        a = VadAudit()
        check(lib().fvad_vad_batch_config_audit(self.h, stream, config, C.byref(a)), "fvad_vad_batch_config_audit")
        return a.min_rel_threshold_margin, a.min_abs_ratio_margin, a.n_frames

    def lazy_stats(self, stream, config):
        """(exact evaluations of the long-term chain, lazily absorbed pushes) of machine (stream, config) in the last run"""
        e, p = C.c_uint64(), C.c_uint64()
        check(lib().fvad_vad_batch_lazy_stats(self.h, stream, config, C.byref(e), C.byref(p)), "fvad_vad_batch_lazy_stats")
        return e.value, p.value

    def set_references(self, refs, stat_cfgs):
        """fvad_vad_batch_set_references: refs[s] = stream s's labels, [(from_sec, to_sec)] or a float32 [n][2] array;
        stat_cfgs: one StatConfig dict per config (stats_from_segments' keys), or one dict for every config"""
        if isinstance(stat_cfgs, dict):
            stat_cfgs = [stat_cfgs] * self.n_configs
        assert len(refs) == self.n_streams and len(stat_cfgs) == self.n_configs
        arrs = [np.asarray(r, np.float32).reshape(-1, 2) for r in refs]
        flat = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros((0, 2), np.float32))
        offs = (sz * (self.n_streams + 1))(*np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(int).tolist())
        sc = (StatConfig * self.n_configs)(*[StatConfig(c.get("ignore_shorter_than_sec", 0.0), c.get("extrude_start", 0.0),
                                                        c.get("extrude_end", 0.0), c.get("fill_gaps", 0.0)) for c in stat_cfgs])
        check(lib().fvad_vad_batch_set_references(self.h, flat.ctypes.data_as(C.POINTER(SegmentSec)), offs, sc),
              "fvad_vad_batch_set_references")

    def keep_segments(self, keep):
        """fvad_vad_batch_set_keep_segments: keep=False leaves a device run's segments on the device (segments() then raises)"""
        check(lib().fvad_vad_batch_set_keep_segments(self.h, 1 if keep else 0), "fvad_vad_batch_set_keep_segments")

    def score(self, n_threads=16):
        """fvad_vad_batch_score: every machine's segments against its stream's labels on n_threads host threads"""
        check(lib().fvad_vad_batch_score(self.h, n_threads), "fvad_vad_batch_score")

    def config_stats(self, config, out=None):
        """config's SingleStats of every stream from the last scoring (host or device), as float32 [n_streams][11]; out: a
        C-contiguous float32 [n_streams][11] array to fill instead"""
        if out is None:
            out = np.empty((self.n_streams, len(SingleStats._fields_)), np.float32)
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.shape == (self.n_streams, len(SingleStats._fields_))
        check(lib().fvad_vad_batch_config_stats(self.h, config, out.ctypes.data_as(C.POINTER(SingleStats))),
              "fvad_vad_batch_config_stats")
        return out

    def close(self):
        if self.h:
            lib().fvad_vad_batch_destroy(self.h)
            self.h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VadSweepSized(VadSweep):
    """fvad_vad_batch_create_sweep_sized: a sweep whose configs run on frames of their own sizes (fft_sizes[c] for configs[c]),
    several frame clocks in one batch.  Everything but the constructor is VadSweep's; bands() names each band's size, and run,
    run_device and run_device_part are the sample-based calls (run_sized, run_device_sized, run_device_part_sized)."""

    def __init__(self, n_streams, configs, fft_sizes, n_channels=1, sample_rate=48000):
        assert len(fft_sizes) == len(configs)
        sizes = (sz * len(configs))(*[int(f) for f in fft_sizes])
        self.h = vp()
        check(lib().fvad_vad_batch_create_sweep_sized(_config_array(configs), sizes, len(configs), sample_rate, n_channels, n_streams,
                                                      C.byref(self.h)), "fvad_vad_batch_create_sweep_sized")
        self._created(n_streams, n_channels, len(configs))

    def bands(self):
        """-> ([(fft_size, min_bin, max_bin)] of the distinct bands, size-major, band_of [config])"""
        bins, band_of = VadSweep.bands(self)
        return [(self.sizes[self.size_of_band[j]], lo, hi) for j, (lo, hi) in enumerate(bins)], band_of

    run = VadSweep.run_sized
    run_device = VadSweep.run_device_sized
    run_device_part = VadSweep.run_device_part_sized


def finish_bits(config, words, ratios, n_frames, first_sample=0, state=None, sample_rate=48000, fft_size=1024, seg_cap=None):
    """fvad_vad_finish_bits: the finishing walk (csrc/vad_finish.h) of one config (overrides dict) over a part's bits (uint64
    words) and frame ratios (float32) -> (segments as SpeechSegment list, state uint64 [6]); state None = a fresh machine"""
    words = np.ascontiguousarray(words, np.uint64)
    ratios = np.ascontiguousarray(ratios, np.float32)
    st = np.zeros(6, np.uint64) if state is None else np.array(state, np.uint64)
    cap = int(n_frames) // 4 + 1 if seg_cap is None else int(seg_cap)
    segs = (SpeechSegment * max(cap, 1))()
    n = sz()
    check(lib().fvad_vad_finish_bits(_config_array([config]), sample_rate, fft_size, words.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     fptr(ratios), int(n_frames), int(first_sample), st.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     segs, cap, C.byref(n)), "fvad_vad_finish_bits")
    return [segs[i] for i in range(n.value)], st


def avg_chain(x, length, first_frame=0, ring=None):
    """fvad_vad_avg_chain: the average of a rolling average of `length` slots (no initial value) after each of the frames
    first_frame + k, x[k] their inputs (float32) -> float64 [len(x)]; ring: the slots as they were before frame first_frame"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros(len(x), np.float64)
    r = None if ring is None else np.ascontiguousarray(ring, np.float32)
    check(lib().fvad_vad_avg_chain(fptr(x), len(x), int(first_frame), int(length), None if r is None else fptr(r),
                                   out.ctypes.data_as(C.POINTER(C.c_double))), "fvad_vad_avg_chain")
    return out


def vad_run_many(machines, bands, ratios, first_index=None, fft_size=1024, n_threads=1):
    """machines: list[VadMachine]; bands[s]: [n_frames][C] f32; ratios[s]: [n_frames] f32 (NaN=null)"""
    n = len(machines)
    C_ = machines[0].n_channels
    hs = (vp * n)(*[m.h for m in machines])
    bands = [np.ascontiguousarray(b, np.float32).reshape(-1, C_) for b in bands]
    ratios = [np.ascontiguousarray(r, np.float32) for r in ratios]
    bp = (c_float_p * n)(*[fptr(b) for b in bands])
    rp = (c_float_p * n)(*[fptr(r) for r in ratios])
    nf = (sz * n)(*[b.shape[0] for b in bands])
    fi = (C.c_uint64 * n)(*(first_index or [0] * n))
    check(lib().fvad_vad_run_many(hs, n, bp, rp, nf, C_, fi, fft_size, n_threads),
          "fvad_vad_run_many")


def _clip_rows(clips):
    return np.ascontiguousarray(np.asarray(clips, np.uint64).reshape(-1, CLIP_FIELDS))


def _clip_split_rows(clips):
    return np.ascontiguousarray(np.asarray(clips, np.uint64).reshape(-1, CLIP_SPLIT_FIELDS))


def clips_split_check(a, b, src_pcm16, clips, out_pcm16=False, out=1 << 20, out_capacity=None, device_out=True, src_format=None,
                      out_format=None):
    """fvad_clips_split_check (host only; a, b as for Context.clips_export_split, `out` an address) -> (status, offsets, total)"""
    clips = _clip_split_rows(clips)
    n = clips.shape[0]
    offsets, total = np.zeros(n, np.uint64), C.c_uint64(0)
    st = lib().fvad_clips_split_check(vp(a[0]), a[1], a[2], a[3], vp(b[0]), b[1], b[2], b[3],
                                      (CLIP_PCM16 if src_pcm16 else CLIP_F32) if src_format is None else src_format,
                                      clips.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                      (CLIP_PCM16 if out_pcm16 else CLIP_F32) if out_format is None else out_format, vp(out),
                                      (1 << 62) if out_capacity is None else out_capacity, int(device_out),
                                      offsets.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(total))
    return st, offsets, total.value


def clips_plan(clips, out_pcm16=False):
    """fvad_clips_plan: (offsets [n] uint64, total), in samples of the output format"""
    clips = _clip_rows(clips)
    offsets = np.zeros(clips.shape[0], np.uint64)
    total = C.c_uint64(0)
    check(lib().fvad_clips_plan(clips.ctypes.data_as(C.POINTER(C.c_uint64)), clips.shape[0], CLIP_PCM16 if out_pcm16 else CLIP_F32,
                                offsets.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(total)), "fvad_clips_plan")
    return offsets, total.value


def clips_phase_skips(sample_from, step, phase):
    """fvad_clips_phase_skips: per clip the first kept sample, so that the kept samples are the lane indices = phase (mod step)"""
    sample_from = np.ascontiguousarray(np.asarray(sample_from, np.uint64).reshape(-1))
    skips = np.zeros(sample_from.shape[0], np.uint32)
    check(lib().fvad_clips_phase_skips(sample_from.ctypes.data_as(C.POINTER(C.c_uint64)), sample_from.shape[0], step, phase,
                                       skips.ctypes.data_as(C.POINTER(C.c_uint32))), "fvad_clips_phase_skips")
    return skips


def clips_fir_design(step, half=0, cutoff=0.0, beta=0.0):
    """fvad_clips_fir_design: the 2 half + 1 float32 taps of a Kaiser-windowed sinc of unit sum (half 0: 16 step, cutoff 0:
    0.45 / step cycles per input sample, beta 0: 6)"""
    taps = np.zeros(CLIP_FIR_TAPS_MAX, np.float32)
    check(lib().fvad_clips_fir_design(step, half, cutoff, beta, fptr(taps)), "fvad_clips_fir_design")
    return taps[:2 * (half if half else 16 * step) + 1].copy()


def clips_fir_check(taps):
    """fvad_clips_fir_check -> status (0: the taps are an odd number of finite values, at most CLIP_FIR_TAPS_MAX)"""
    if taps is None:
        return lib().fvad_clips_fir_check(None, 0)
    taps = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
    return lib().fvad_clips_fir_check(fptr(taps), taps.shape[0])


def clips_plan_strided(lens, skips, step, out_pcm16=False):
    """fvad_clips_plan_strided: (out_lens [n] uint64, offsets [n] uint64, total), in samples of the output format; skips None: 0"""
    lens = np.ascontiguousarray(np.asarray(lens, np.uint64).reshape(-1))
    n = lens.shape[0]
    skips = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32).reshape(n))
    out_lens, offsets, total = np.zeros(n, np.uint64), np.zeros(n, np.uint64), C.c_uint64(0)
    check(lib().fvad_clips_plan_strided(lens.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        None if skips is None else skips.ctypes.data_as(C.POINTER(C.c_uint32)), n, step,
                                        CLIP_PCM16 if out_pcm16 else CLIP_F32, out_lens.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        offsets.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(total)), "fvad_clips_plan_strided")
    return out_lens, offsets, int(total.value)


def clips_plan_resampled(lens, up, down, out_pcm16=False):
    """fvad_clips_plan_resampled: (out_lens [n] uint64 = ceil(len * up / down), offsets [n] uint64, total), in samples of the
    output format"""
    lens = np.ascontiguousarray(np.asarray(lens, np.uint64).reshape(-1))
    n = lens.shape[0]
    out_lens, offsets, total = np.zeros(n, np.uint64), np.zeros(n, np.uint64), C.c_uint64(0)
    check(lib().fvad_clips_plan_resampled(lens.ctypes.data_as(C.POINTER(C.c_uint64)), n, int(up), int(down), CLIP_PCM16 if out_pcm16 else CLIP_F32,
                                          out_lens.ctypes.data_as(C.POINTER(C.c_uint64)), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          C.byref(total)), "fvad_clips_plan_resampled")
    return out_lens, offsets, int(total.value)


def mel_design(sample_rate, n_fft, n_mels, fmin, fmax):
    """fvad_mel_design: Slaney's mel filter bank [n_mels][n_fft / 2 + 1] float32 (librosa.filters.mel's formula)"""
    matrix = np.zeros((max(int(n_mels), 1), max(int(n_fft), 0) // 2 + 1), np.float32)
    check(lib().fvad_mel_design(sample_rate, int(n_fft), int(n_mels), fmin, fmax, fptr(matrix)), "fvad_mel_design")
    return matrix


def _clips_plan_features(name, lens, skips, step, taps, hop, n_mels):
    """fvad_clips_plan_mel / fvad_clips_plan_fbank (`name`; taps is n_fft or win_length)"""
    lens = np.ascontiguousarray(np.asarray(lens, np.uint64).reshape(-1))
    n = lens.shape[0]
    skips = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32).reshape(n))
    n_frames, offsets, total = np.zeros(n, np.uint64), np.zeros(n, np.uint64), C.c_uint64(0)
    check(getattr(lib(), name)(lens.ctypes.data_as(C.POINTER(C.c_uint64)),
                               None if skips is None else skips.ctypes.data_as(C.POINTER(C.c_uint32)), n, int(step), int(taps),
                               int(hop), int(n_mels), n_frames.ctypes.data_as(C.POINTER(C.c_uint64)),
                               offsets.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(total)), name)
    return n_frames, offsets, int(total.value)


def _clips_features_check(name, d_src, src_format, n_lanes, lane_stride, n_samples, clips, out, out_capacity, device_out, step, skips,
                          out_format, params, split=None):
    """fvad_clips_mel_check / fvad_clips_fbank_check (`name`).  params(p) is the family's arguments between skips and n_frames, p
    turning a float32 array or None into a pointer or NULL.  split (a, b): fvad_clips_split_mel_check / _split_fbank_check over
    split rows; d_src, n_lanes, lane_stride and n_samples are then not used"""
    clips = None if clips is None else (_clip_split_rows if split else _clip_rows)(clips)
    n = 0 if clips is None else clips.shape[0]
    skips = None if skips is None else np.ascontiguousarray(np.asarray(skips, np.uint32).reshape(-1))
    keep = []

    def p(a):
        if a is None:
            return None
        keep.append(np.ascontiguousarray(np.asarray(a, np.float32)))
        return fptr(keep[-1])
    n_frames, offsets, total = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), C.c_uint64(0)
    a, b = split if split else (None, None)
    src_args = (vp(a[0]), a[1], a[2], a[3], vp(b[0]), b[1], b[2], b[3], src_format) if split else (vp(d_src), src_format, n_lanes, lane_stride, n_samples)
    st = getattr(lib(), name)(*src_args,
                              None if clips is None else clips.ctypes.data_as(C.POINTER(C.c_uint64)), n, out_format, vp(out),
                              out_capacity, int(device_out), int(step),
                              None if skips is None else skips.ctypes.data_as(C.POINTER(C.c_uint32)), *params(p),
                              n_frames.ctypes.data_as(C.POINTER(C.c_uint64)), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                              C.byref(total))
    return st, n_frames[:n], offsets[:n], int(total.value)


def clips_plan_mel(lens, skips, step, n_fft, hop, n_mels):
    """fvad_clips_plan_mel: (n_frames [n] uint64, offsets [n] uint64, total), offsets and total in floats; skips None: 0"""
    return _clips_plan_features("fvad_clips_plan_mel", lens, skips, step, n_fft, hop, n_mels)


def clips_mel_check(d_src, src_format, n_lanes, lane_stride, n_samples, clips, out, out_capacity, device_out, step, skips, n_fft, hop,
                    window, n_mels, matrix, floor, norm, out_format=CLIP_F32):
    """fvad_clips_mel_check (host only; d_src and out are addresses) -> (status, n_frames, offsets, total).  window, matrix and
    norm are float32 arrays or None (NULL), passed as they are"""
    return _clips_features_check("fvad_clips_mel_check", d_src, src_format, n_lanes, lane_stride, n_samples, clips, out, out_capacity,
                                 device_out, step, skips, out_format,
                                 lambda p: (int(n_fft), int(hop), p(window), int(n_mels), p(matrix), floor, p(norm)))


def mel_design_kaldi(sample_rate, n_fft, n_mels, low_freq, high_freq):
    """fvad_mel_design_kaldi: Kaldi's mel bank [n_mels][n_fft / 2 + 1] float32 (HTK mel, triangles in the mel domain, no
    normalisation, a zero Nyquist column); high_freq <= 0 counts from Nyquist"""
    matrix = np.zeros((max(int(n_mels), 1), max(int(n_fft), 0) // 2 + 1), np.float32)
    check(lib().fvad_mel_design_kaldi(sample_rate, int(n_fft), int(n_mels), low_freq, high_freq, fptr(matrix)), "fvad_mel_design_kaldi")
    return matrix


def clips_plan_fbank(lens, skips, step, win_length, hop, n_mels):
    """fvad_clips_plan_fbank: (n_frames [n] uint64, offsets [n] uint64, total), offsets and total in floats; skips None: 0"""
    return _clips_plan_features("fvad_clips_plan_fbank", lens, skips, step, win_length, hop, n_mels)


def clips_fbank_check(d_src, src_format, n_lanes, lane_stride, n_samples, clips, out, out_capacity, device_out, step, skips, win_length,
                      n_fft, hop, window, n_mels, matrix, scale, preemph, remove_dc, floor, cmn, out_format=CLIP_F32):
    """fvad_clips_fbank_check (host only; d_src and out are addresses) -> (status, n_frames, offsets, total).  window and matrix
    are float32 arrays or None (NULL), passed as they are"""
    return _clips_features_check("fvad_clips_fbank_check", d_src, src_format, n_lanes, lane_stride, n_samples, clips, out, out_capacity,
                                 device_out, step, skips, out_format,
                                 lambda p: (int(win_length), int(n_fft), int(hop), p(window), int(n_mels), p(matrix), scale, preemph,
                                            int(remove_dc), floor, int(cmn)))


def clips_split_mel_check(a, b, src_format, clips, out, out_capacity, device_out, step, skips, n_fft, hop, window, n_mels, matrix, floor,
                          norm, out_format=CLIP_F32):
    """fvad_clips_split_mel_check (host only; a, b as for Context.clips_export_split, `out` an address) -> (status, n_frames,
    offsets, total), as clips_mel_check"""
    return _clips_features_check("fvad_clips_split_mel_check", None, src_format, 0, 0, 0, clips, out, out_capacity, device_out, step, skips,
                                 out_format, lambda p: (int(n_fft), int(hop), p(window), int(n_mels), p(matrix), floor, p(norm)), split=(a, b))


def clips_split_fbank_check(a, b, src_format, clips, out, out_capacity, device_out, step, skips, win_length, n_fft, hop, window, n_mels,
                            matrix, scale, preemph, remove_dc, floor, cmn, out_format=CLIP_F32):
    """fvad_clips_split_fbank_check (host only) -> (status, n_frames, offsets, total), as clips_fbank_check"""
    return _clips_features_check("fvad_clips_split_fbank_check", None, src_format, 0, 0, 0, clips, out, out_capacity, device_out, step, skips,
                                 out_format,
                                 lambda p: (int(win_length), int(n_fft), int(hop), p(window), int(n_mels), p(matrix), scale, preemph,
                                            int(remove_dc), floor, int(cmn)), split=(a, b))


def clips_resample_check(up, down, taps):
    """fvad_clips_resample_check -> status (0: up / down is a ratio, the taps are an odd number of finite values, at most
    RESAMPLE_TAPS_MAX, and the window of 8 outputs fits a tile of the gather)"""
    if taps is None:
        return lib().fvad_clips_resample_check(int(up), int(down), None, 0)
    taps = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
    return lib().fvad_clips_resample_check(int(up), int(down), fptr(taps), taps.shape[0])


def clips_resample_tile(up, down, n_taps):
    """fvad_clips_resample_tile: outputs per workgroup of the resampling clip gather (0: the window of 8 outputs does not fit, or
    the ratio or the tap count is none)"""
    return int(lib().fvad_clips_resample_tile(int(up), int(down), int(n_taps)))


def clips_from_segments(segs, first_lane, n_channels, n_available, cap=None):
    """fvad_clips_from_segments: segs = [(sample_from, sample_to, ...)] -> (clips [n][CLIP_FIELDS] uint64, n_skipped)"""
    arr = (SpeechSegment * max(len(segs), 1))()
    for i, s in enumerate(segs):
        arr[i].sample_from, arr[i].sample_to = int(s[0]), int(s[1])
    cap = len(segs) if cap is None else cap
    clips = np.zeros((max(cap, 1), CLIP_FIELDS), np.uint64)
    n, skipped = sz(), sz()
    check(lib().fvad_clips_from_segments(arr, len(segs), first_lane, n_channels, n_available,
                                         clips.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(n), C.byref(skipped)),
          "fvad_clips_from_segments")
    return clips[:n.value].copy(), skipped.value


def _ingest_rows(sources):
    return np.ascontiguousarray(np.asarray(sources, np.uint64).reshape(-1, INGEST_FIELDS))


def ingest_tile_frames(n_channels, fmt):
    """frames of a source per workgroup of the ingest kernel: INGEST_TILE_BYTES rounded down to whole frames, in fours"""
    return INGEST_TILE_BYTES // (n_channels * INGEST_SAMPLE_BYTES[fmt]) // 4 * 4


def _host_buffers(call, noun, verb, rows, bufs, writable, where=None):
    """The per-row host buffers of a host-form call (`call`: the method's name; `where`: the C call in an FvadError, fvad_<call>
    unless given) -> the pointer array the library takes.  A row without frames gets None: no byte of it is read or written,
    whatever its byte_offset says.  Every other buffer is a C-contiguous uint8 array (`writable` for the calls that write) that
    holds what the row `verb`s -- the library cannot know where a host buffer ends."""
    n = rows.shape[0]
    if len(bufs) != n:
        raise ValueError(f"{call}: {n} {noun}s, {len(bufs)} buffers")
    ptrs = (vp * max(n, 1))()
    for i, b in enumerate(bufs):
        if b is None or b.size == 0 or int(rows[i, 1]) == 0:
            ptrs[i] = None
            continue
        if b.dtype != np.uint8 or not b.flags["C_CONTIGUOUS"] or (writable and not b.flags["WRITEABLE"]):
            raise ValueError(f"{call}: a {noun}'s bytes are a {'writable ' if writable else ''}C-contiguous uint8 array")
        need = int(rows[i, 0]) + int(rows[i, 1]) * int(rows[i, 2]) * INGEST_SAMPLE_BYTES.get(int(rows[i, 3]), 4)
        if need > b.size:
            raise FvadError(FVAD_ERR_OUT_OF_RANGE, where or "fvad_" + call, f"{noun} {i} {verb} {need} bytes of a buffer of {b.size}")
        ptrs[i] = b.ctypes.data
    return ptrs


def ingest_check(sources, raw_bytes, out_pcm16, n_lanes, lane_stride, n_samples):
    """fvad_ingest_check: the status (FVAD_OK or the error the device calls would return), without a device"""
    sources = _ingest_rows(sources)
    return lib().fvad_ingest_check(sources.ctypes.data_as(C.POINTER(C.c_uint64)), sources.shape[0], int(raw_bytes),
                                   INGEST_PCM16 if out_pcm16 else INGEST_F32, n_lanes, lane_stride, n_samples)


def _egress_rows(sinks):
    return np.ascontiguousarray(np.asarray(sinks, np.uint64).reshape(-1, EGRESS_FIELDS))


def egress_check(sinks, out_bytes, src_pcm16, n_lanes, lane_stride, n_samples):
    """fvad_egress_check: the status (FVAD_OK or the error the device calls would return), without a device"""
    sinks = _egress_rows(sinks)
    return lib().fvad_egress_check(sinks.ctypes.data_as(C.POINTER(C.c_uint64)), sinks.shape[0], int(out_bytes),
                                   INGEST_PCM16 if src_pcm16 else INGEST_F32, n_lanes, lane_stride, n_samples)


def _egress_mix_rows(sinks):
    return np.ascontiguousarray(np.asarray(sinks, np.uint64).reshape(-1, EGRESS_MIX_FIELDS))


def egress_mix_check(sinks, out_bytes, w_orig, w_den, n_lanes, orig_stride, orig_samples, den_stride, den_samples, src_pcm16=False):
    """fvad_egress_mix_check: the status (FVAD_OK or the error the device calls would return), without a device"""
    sinks = _egress_mix_rows(sinks)
    return lib().fvad_egress_mix_check(sinks.ctypes.data_as(C.POINTER(C.c_uint64)), sinks.shape[0], int(out_bytes),
                                       INGEST_PCM16 if src_pcm16 else INGEST_F32, float(w_orig), float(w_den), n_lanes, orig_stride,
                                       orig_samples, den_stride, den_samples)


def nsnet2_delay(sample_rate):
    """fvad_nsnet2_delay: the samples (of sample_rate) by which NSNet2's denoised output lags its input, 482 at 48000"""
    d = C.c_uint64(0)
    check(lib().fvad_nsnet2_delay(int(sample_rate), C.byref(d)), "fvad_nsnet2_delay")
    return int(d.value)


def _egress_resample_rows(sinks):
    return np.ascontiguousarray(np.asarray(sinks, np.uint64).reshape(-1, EGRESS_RESAMPLE_FIELDS))


def egress_resample_tile(up, down, n_taps, n_channels, fmt):
    """fvad_egress_resample_tile: output frames per workgroup of the resampling egress kernel (0: the window of 4 outputs does
    not fit a tile, or arguments that are none)"""
    return int(lib().fvad_egress_resample_tile(up, down, n_taps, n_channels, fmt))


def egress_resample_ready(up, down, n_taps, stream_frames, frames_have):
    """fvad_egress_resample_ready: the leading outputs of a stream of stream_frames lane samples whose whole window lies below
    frames_have (all of them once frames_have >= stream_frames): what a time slice can finish"""
    return int(lib().fvad_egress_resample_ready(up, down, n_taps, int(stream_frames), int(frames_have)))


def egress_resample_check(sinks, out_bytes, up, down, taps, n_lanes, lane_stride, n_samples, src_pcm16=False):
    """fvad_egress_resample_check: the status (FVAD_OK or the error the device calls would return), without a device"""
    sinks = _egress_resample_rows(sinks)
    if taps is None:
        tp, nt = None, 0
    else:
        taps = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
        tp, nt = fptr(taps), taps.shape[0]
    return lib().fvad_egress_resample_check(sinks.ctypes.data_as(C.POINTER(C.c_uint64)), sinks.shape[0], int(out_bytes), up, down, tp, nt,
                                            INGEST_PCM16 if src_pcm16 else INGEST_F32, n_lanes, lane_stride, n_samples)


def egress_resample_strided_check(sinks, out_bytes, up, down, taps, src_step, n_lanes, lane_stride, n_samples, src_pcm16=False):
    """fvad_egress_resample_strided_check: the status (FVAD_OK or the error the device calls would return), without a device"""
    sinks = _egress_resample_rows(sinks)
    if taps is None:
        tp, nt = None, 0
    else:
        taps = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
        tp, nt = fptr(taps), taps.shape[0]
    return lib().fvad_egress_resample_strided_check(sinks.ctypes.data_as(C.POINTER(C.c_uint64)), sinks.shape[0], int(out_bytes), up, down, tp, nt,
                                                    int(src_step), INGEST_PCM16 if src_pcm16 else INGEST_F32, n_lanes, lane_stride, n_samples)


def wav_header(fmt, n_channels, sample_rate, n_frames):
    """fvad_wav_header: the 44 bytes in front of the samples of a canonical WAV file of format fmt (INGEST_F32, INGEST_PCM16 or
    INGEST_PCM24); FvadError for what fvad_wav_write refuses (no or too many channels, a zero rate, more than 4 GB of data)"""
    out, n = np.zeros(WAV_HEADER_BYTES, np.uint8), sz(0)
    check(lib().fvad_wav_header(int(fmt), int(n_channels), int(sample_rate), int(n_frames), out.ctypes.data, out.size, C.byref(n)),
          "fvad_wav_header")
    return out[:n.value].tobytes()


def _resample_rows(sources):
    return np.ascontiguousarray(np.asarray(sources, np.uint64).reshape(-1, RESAMPLE_FIELDS))


def resample_ratio(rate_in, rate_out=48000):
    """fvad_resample_ratio: (up, down) = rate_out / rate_in in lowest terms; FvadError for a zero rate or up > RESAMPLE_UP_MAX"""
    up, down = C.c_uint32(0), C.c_uint32(0)
    check(lib().fvad_resample_ratio(rate_in, rate_out, C.byref(up), C.byref(down)), f"fvad_resample_ratio({rate_in}, {rate_out})")
    return up.value, down.value


def resample_out_frames(file_frames, up, down):
    """fvad_resample_out_frames: ceil(file_frames * up / down)"""
    return int(lib().fvad_resample_out_frames(int(file_frames), up, down))


def resample_design(up, down, half=0, cutoff=0.0, beta=0.0):
    """fvad_resample_design: the 2 half max(up, down) + 1 float32 taps of a Kaiser-windowed sinc that sum to `up` (half 0: 16,
    cutoff 0: 0.45 / max(up, down) cycles per sample of the up-times-oversampled input, beta 0: 6)"""
    taps, n = np.zeros(RESAMPLE_TAPS_MAX, np.float32), C.c_uint32(0)
    check(lib().fvad_resample_design(up, down, half, cutoff, beta, fptr(taps), C.byref(n)), "fvad_resample_design")
    return taps[:n.value].copy()


def resample_window(up, down, n_taps, file_frames, out_from, n_out):
    """fvad_resample_window: (frame_lo, frame_hi), the file's frames that outputs [out_from, out_from + n_out) read"""
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    check(lib().fvad_resample_window(up, down, n_taps, int(file_frames), int(out_from), int(n_out), C.byref(lo), C.byref(hi)),
          "fvad_resample_window")
    return int(lo.value), int(hi.value)


def ingest_resample_tile(up, down, n_taps, n_channels, fmt):
    """fvad_ingest_resample_tile: outputs of one channel per workgroup of the resampling ingest kernel (0: the taps are too long
    for frames this wide)"""
    return int(lib().fvad_ingest_resample_tile(up, down, n_taps, n_channels, fmt))


def ingest_resample_check(sources, raw_bytes, up, down, taps, n_lanes, lane_stride, n_samples, out_pcm16=False):
    """fvad_ingest_resample_check: the status (FVAD_OK or the error the device calls would return), without a device"""
    sources = _resample_rows(sources)
    if taps is None:
        tp, nt = None, 0
    else:
        taps = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
        tp, nt = fptr(taps), taps.shape[0]
    return lib().fvad_ingest_resample_check(sources.ctypes.data_as(C.POINTER(C.c_uint64)), sources.shape[0], int(raw_bytes), up, down,
                                            tp, nt, INGEST_PCM16 if out_pcm16 else INGEST_F32, n_lanes, lane_stride, n_samples)


def wav_probe(path):
    """fvad_wav_probe: a WAV file's header without its samples -> dict(format [INGEST_*], n_channels, sample_rate, data_offset,
    n_frames, bits).  PCM16, PCM24 and 32-bit float; whatever else fvad_wav_read refuses raises FvadError."""
    info = (C.c_uint64 * WAV_INFO_FIELDS)()
    check(lib().fvad_wav_probe(path.encode(), info), f"fvad_wav_probe({path})")
    return dict(zip(("format", "n_channels", "sample_rate", "data_offset", "n_frames", "bits"), (int(x) for x in info)))


def wav_map_raw(path):
    """A WAV file's data chunk as bytes, not read: (raw, info) -- raw a read-only uint8 numpy memmap of the n_frames *
    n_channels * bits / 8 bytes of its whole frames, interleaved as in the file (what Context.ingest takes), info wav_probe's
    dict.  Takes 24-bit PCM too, which wav_map refuses."""
    info = wav_probe(path)
    n = info["n_frames"] * info["n_channels"] * (info["bits"] // 8)
    if n == 0:
        return np.zeros(0, np.uint8), info
    return np.memmap(path, dtype=np.uint8, mode="r", offset=info["data_offset"], shape=(n,)), info


def wav_read(path):
    """-> (pcm [n_channels][n_frames] float32, sample_rate)"""
    pcm = C.POINTER(c_float_p)()
    nc, nf, sr = sz(), sz(), sz()
    check(lib().fvad_wav_read(path.encode(), C.byref(pcm), C.byref(nc), C.byref(nf), C.byref(sr)),
          f"fvad_wav_read({path})")
    try:
        out = np.empty((nc.value, nf.value), np.float32)
        for c in range(nc.value):
            if nf.value:
                out[c] = np.ctypeslib.as_array(pcm[c], shape=(nf.value,))
        return out, sr.value
    finally:
        lib().fvad_wav_free(pcm, nc.value)


def wav_write(path, pcm, sample_rate=48000, pcm16=False):
    """pcm [n_channels][n_frames] float32 -> WAV file (float32 or PCM16)"""
    pcm = np.ascontiguousarray(np.atleast_2d(pcm), dtype=np.float32)
    ptrs = (c_float_p * pcm.shape[0])(*[fptr(pcm[c]) for c in range(pcm.shape[0])])
    check(lib().fvad_wav_write(path.encode(), ptrs, pcm.shape[0], pcm.shape[1], sample_rate, 1 if pcm16 else 0), "fvad_wav_write")


def wav_write_i16(path, pcm, sample_rate=48000):
    """pcm [n_channels][n_frames] int16 -> PCM16 WAV file, the samples as they are (fvad_wav_write_i16)"""
    pcm = np.atleast_2d(pcm)
    assert pcm.dtype == np.int16
    pcm = np.ascontiguousarray(pcm)
    i16p = C.POINTER(C.c_int16)
    ptrs = (i16p * pcm.shape[0])(*[pcm[c].ctypes.data_as(i16p) for c in range(pcm.shape[0])])
    check(lib().fvad_wav_write_i16(path.encode(), ptrs, pcm.shape[0], pcm.shape[1], sample_rate), "fvad_wav_write_i16")


def wav_read_i16(path):
    """PCM16 WAV -> (pcm [n_channels][n_frames] int16, sample_rate) without conversion"""
    pp = C.POINTER(C.POINTER(C.c_int16))()
    nch, nfr, sr = sz(), sz(), sz()
    check(lib().fvad_wav_read_i16(path.encode(), C.byref(pp), C.byref(nch), C.byref(nfr), C.byref(sr)), "fvad_wav_read_i16")
    try:
        out = np.empty((nch.value, nfr.value), np.int16)    # one copy per channel (stacking copies of the channels was three)
        for c in range(nch.value):
            if nfr.value:
                out[c] = np.ctypeslib.as_array(pp[c], shape=(nfr.value,))
    finally:
        lib().fvad_wav_free_i16(pp, nch.value)
    return out, sr.value


def wav_map(path):
    """A WAV file's samples without reading them: (samples, sample_rate), samples a read-only numpy memmap of the data chunk,
    [n_frames][n_channels] int16 (PCM16) or float32 (IEEE float), interleaved as in the file.  The RIFF chunks are walked as
    fvad_wav_read walks them (the first "fmt " and "data" chunks; WAVE_FORMAT_EXTENSIBLE takes its sub-format; a data length
    past the end of the file is cut to the file); whatever fvad_wav_read refuses raises FvadError."""
    import struct
    def bad(why):
        return FvadError(FVAD_ERR_MODEL_FORMAT, f"wav_map({path})", why)

    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise bad("not a RIFF/WAVE file")
        tag = channels = bits = rate = 0
        data_off = data_bytes = None
        pos = 12
        while pos + 8 <= size:
            f.seek(pos)
            ck = f.read(8)
            length = struct.unpack("<I", ck[4:8])[0]
            body = pos + 8
            if ck[:4] == b"fmt " and length >= 16 and body + 16 <= size:
                fmt = f.read(min(length, 26))
                tag, channels, rate = struct.unpack("<HHI", fmt[:8])
                bits = struct.unpack("<H", fmt[14:16])[0]
                if tag == 0xFFFE and length >= 26 and body + 26 <= size:
                    tag = struct.unpack("<H", fmt[24:26])[0]
            elif ck[:4] == b"data":
                data_off = body
                data_bytes = length if body + length <= size else size - body
                break
            pos = body + length + (length & 1)
    if data_off is None or channels <= 0 or rate == 0:
        raise bad("no data chunk or no format")
    if tag == 1 and bits == 16:
        dtype = np.dtype("<i2")
    elif tag == 3 and bits == 32:
        dtype = np.dtype("<f4")
    else:
        raise bad(f"format tag {tag} with {bits} bits (PCM16 or 32-bit float only)")
    frames = data_bytes // (channels * dtype.itemsize)
    if frames == 0:
        return np.zeros((0, channels), dtype), rate
    return np.memmap(path, dtype=dtype, mode="r", offset=data_off, shape=(frames, channels)), rate


def parse_audacity(text):
    raw = text.encode() if isinstance(text, str) else text
    cap = raw.count(b"\n") + 2
    out = (SegmentSec * cap)()
    n = sz()
    check(lib().fvad_parse_audacity(raw, len(raw), out, cap, C.byref(n)), "formats.parseAudacitySegments")
    return [(out[i].from_sec, out[i].to_sec) for i in range(n.value)]


def stats_from_segments(vad, ref, cfg):
    """vad/ref: lists of (from_sec, to_sec); cfg: dict -> SingleStats"""
    v = (SegmentSec * max(len(vad), 1))(*[SegmentSec(a, b) for a, b in vad])
    r = (SegmentSec * max(len(ref), 1))(*[SegmentSec(a, b) for a, b in ref])
    sc = StatConfig(cfg.get("ignore_shorter_than_sec", 0.0), cfg.get("extrude_start", 0.0),
                    cfg.get("extrude_end", 0.0), cfg.get("fill_gaps", 0.0))
    out = SingleStats()
    check(lib().fvad_stats_from_segments(v, len(vad), r, len(ref), C.byref(sc), C.byref(out)),
          "statistics.fromEvaluator")
    return out


COMM_ID_BYTES = 128


def comm_unique_id():
    """rank 0: the 128-byte RCCL bootstrap id (bytes) to hand to the other ranks"""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    check(lib().fvad_comm_unique_id(buf, COMM_ID_BYTES), "fvad_comm_unique_id")
    return bytes(buf)


class Comm:
    """fvad_comm: one rank of the per-stream statistics all-gather (RCCL, bound to the context's device)"""

    def __init__(self, ctx, unique_id, world, rank):
        self.ctx = ctx
        self.h = vp()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        check(lib().fvad_comm_create(ctx.h, buf, COMM_ID_BYTES, world, rank, C.byref(self.h)), "fvad_comm_create", ctx.h)
        self.world, self.rank = world, rank

    def allgather_stats(self, local_ids, local_stats, n_streams):
        """local_stats: list of SingleStats -> list of n_streams SingleStats in plan order"""
        n = len(local_ids)
        ids = (C.c_uint32 * max(n, 1))(*local_ids)
        loc = (SingleStats * max(n, 1))(*local_stats)
        out = (SingleStats * n_streams)()
        check(lib().fvad_stats_allgather(self.h, ids, loc, n, n_streams, out), "fvad_stats_allgather", self.ctx.h)
        return list(out)

    def close(self):
        if self.h:
            lib().fvad_comm_destroy(self.h)
            self.h = vp()


def stats_aggregate(stats):
    arr = (SingleStats * max(len(stats), 1))(*stats)
    out = AggregateStats()
    check(lib().fvad_stats_aggregate(arr, len(stats), C.byref(out)), "statistics.aggregate")
    return out


def stats_aggregate_array(stats):
    """statistics.aggregate over a C-contiguous float32 [n][11] array of SingleStats (VadSweep.config_stats' layout)"""
    assert stats.dtype == np.float32 and stats.flags["C_CONTIGUOUS"] and stats.shape[-1] == len(SingleStats._fields_)
    out = AggregateStats()
    check(lib().fvad_stats_aggregate(stats.ctypes.data_as(C.POINTER(SingleStats)), stats.shape[0], C.byref(out)),
          "statistics.aggregate")
    return out


def single_stats_to_array(s):
    return np.array([getattr(s, n) for n, _ in SingleStats._fields_], np.float32)


def array_to_single_stats(a):
    s = SingleStats()
    for (n, _), v in zip(SingleStats._fields_, a):
        setattr(s, n, float(v))
    return s
