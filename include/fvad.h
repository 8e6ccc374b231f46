/*
 * fvad.h -- C ABI of libfvad_hip.so: the MI355X (gfx950) implementation of Formula-VAD's
 * per-frame spectral front end + NSNet2 denoiser + VAD decision path.
 *
 * The reference (recursiveGecko/Formula-VAD) is Zig; its hot path sits behind three nested Zig
 * seams: B1 AudioPipeline (src/AudioPipeline.zig), B2 NSNet2
 * (src/NSNet2.zig), B3 FFT (src/FFT.zig), which bottom out in two C-ABI dependencies, kissfft
 * and ONNX Runtime.  Every entry point below names the reference interface it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the Zig `extern` block a
 * maintainer adds (bindings/fvad.zig).
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returns an int
 * status (0 = FVAD_OK, negative = the reference's Zig error of the same name) unless it is a
 * pure query; nothing throws or aborts across this boundary.  The caller owns every sample
 * buffer and the callee never keeps a pointer past the call (same contract as the ring-buffer
 * slices the reference hands around, src/structures/MultiRingBuffer.zig:159-161).  Objects are
 * thread-confined like the reference's (one AudioPipeline per OS thread,
 * src/simulator.zig:225-231): one fvad_ctx = one HIP device + one HIP stream.
 *
 * Audio is channel-planar f32 (`[][]f32`, src/AudioPipeline.zig:118); `Complex` is
 * {f32 r; f32 i} (src/FFT.zig:12-14, == kiss_fft_cpx); sample indices are u64
 * (src/AudioPipeline/Segment.zig:22).
 *
 * The functions that need the GPU fail with FVAD_ERR_NO_DEVICE when no gfx950 device is
 * present; there is no CPU fallback.  The VAD state machine / Evaluator entry points are host
 * code by design (src/AudioPipeline/VADMachine.zig is sequential per stream) and work without
 * a device.
 */
#ifndef FVAD_H
#define FVAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FVAD_ABI_VERSION 3

/* ------------------------------------------------------------------ status codes */
enum {
    FVAD_OK = 0,
    FVAD_ERR_INVALID_FFT_SIZE = -1,       /* error.InvalidFFTSize        FFT.zig:42 */
    FVAD_ERR_INVALID_SAMPLES_LENGTH = -2, /* error.InvalidSamplesLength  FFT.zig:92 */
    FVAD_ERR_INVALID_WINDOW_LENGTH = -3,  /* error.InvalidWindowLength   FFT.zig:96 */
    FVAD_ERR_INVALID_RESULT_LENGTH = -4,  /* error.InvalidResultLength   FFT.zig:101,125 */
    FVAD_ERR_INVALID_BINS_LENGTH = -5,    /* error.InvalidBinsLength     FFT.zig:121 */
    FVAD_ERR_OUT_OF_RANGE = -6,           /* error.OutOfRange            FFT.zig:158,174 */
    FVAD_ERR_NEGATIVE_FREQUENCY = -7,     /* error.NegativeFrequency     FFT.zig:162 */
    FVAD_ERR_INVALID_INPUT_LENGTH = -8,   /* error.InvalidInputLength    NSNet2.zig:168 */
    FVAD_ERR_INVALID_SAMPLE_RATE = -9,    /* error.InvalidSampleRate     VADPipeline.zig:57 */
    FVAD_ERR_CHANNEL_COUNT_MISMATCH = -10,/* error.ChannelCountMismatch  SegmentWriter.zig:70 */
    FVAD_ERR_ALLOC_FAILED = -11,          /* error.KissFFTAllocFailed / OutOfMemory FFT.zig:59 */
    /* errors with no reference counterpart */
    FVAD_ERR_INVALID_ARGUMENT = -100,
    FVAD_ERR_NO_DEVICE = -101,            /* no gfx950 device / HIP runtime unavailable */
    FVAD_ERR_HIP = -102,                  /* a HIP call failed; text in fvad_last_error */
    FVAD_ERR_NO_MODEL = -103,             /* NSNet2 weights not loaded */
    FVAD_ERR_MODEL_FORMAT = -104,         /* ONNX file unreadable / not the NSNet2 graph */
    FVAD_ERR_IO = -105,
    FVAD_ERR_BUFFER_TOO_SMALL = -106,
    FVAD_ERR_NOT_AVAILABLE = -107         /* what was asked for does not exist in this state (fvad_ctx_nn_tap) */
};

const char *fvad_status_name(int status);
int fvad_abi_version(void);

/* ------------------------------------------------------------------ context */
typedef struct fvad_ctx fvad_ctx;

/* Binds HIP device `device` (hipSetDevice) and creates the context's stream and constant
 * tables (windows, twiddles).  Replaces the allocator argument every reference init takes. */
int fvad_ctx_create(int device, fvad_ctx **out);
void fvad_ctx_destroy(fvad_ctx *ctx);
/* Text of the last failure on this context ("" if none).  Valid until the next call. */
const char *fvad_last_error(const fvad_ctx *ctx);
/* Blocks until all work queued on the context's stream has finished. */
int fvad_ctx_synchronize(fvad_ctx *ctx);
/* The context's hipStream_t as an opaque pointer, so a caller can time it with HIP events. */
void *fvad_ctx_stream(fvad_ctx *ctx);
/* hipMemcpyAsync(device -> host) on the context's stream: ordered after everything queued so
 * far; the bytes are valid after fvad_ctx_synchronize. */
int fvad_ctx_copy_to_host(fvad_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);
/* Page-locked host memory for audio buffers handed to fvad_engine_run / fvad_pipeline_push_samples.
 * Optional: any host pointer is accepted, but pageable memory has to be staged through pinned rings
 * (the host side of that moves ~25-45 GB/s), while buffers from this allocator are copied by the DMA
 * engine directly (57 GB/s measured).  The allocator replaces the std.mem.Allocator the reference
 * injects for its sample buffers (AudioPipeline.zig:40-44).  Free with fvad_host_free. */
int fvad_host_alloc(fvad_ctx *ctx, size_t bytes, void **out);
void fvad_host_free(fvad_ctx *ctx, void *p);
/* Device (HBM) memory on the context's device, for callers that keep audio resident on the GPU
 * (fvad_engine_enqueue_device, `on_device` lanes) without linking a HIP runtime themselves: a Zig or C
 * host needs nothing but this library.  fvad_ctx_copy_to_device is a hipMemcpyAsync(host -> device)
 * on the context's stream: `src_host` must stay valid until fvad_ctx_synchronize. */
int fvad_device_alloc(fvad_ctx *ctx, size_t bytes, void **out);
void fvad_device_free(fvad_ctx *ctx, void *p);
int fvad_ctx_copy_to_device(fvad_ctx *ctx, void *dst_device, const void *src_host, size_t bytes);

/* ------------------------------------------------------------------ NSNet2 model
 * Replaces onnx.OnnxInstance.init(allocator, .{ .model_path = ... }) (NSNet2.zig:53-61): the
 * model is loaded once per context and shared by every denoiser/pipeline made from it. */

/* Host-side weights in the ONNX operator layout: all matrices [out][in] row-major; GRU tensors
 * W [3H][in], R [3H][H], B [6H] = {Wb_z,Wb_r,Wb_h,Rb_z,Rb_r,Rb_h}, gate order z,r,h,
 * linear_before_reset = 1. */
typedef struct {
    int32_t n_bins;   /* 161 */
    int32_t n_fc1;    /* 400 */
    int32_t n_hidden; /* 400 */
    int32_t n_fc2;    /* 600 */
    int32_t n_fc3;    /* 600 */
    const float *fc1_w, *fc1_b;
    const float *gru1_w, *gru1_r, *gru1_b;
    const float *gru2_w, *gru2_r, *gru2_b;
    const float *fc2_w, *fc2_b;
    const float *fc3_w, *fc3_b;
    const float *fc4_w, *fc4_b;
} fvad_nsnet2_weights;

/* Reads nsnet2-20ms-baseline.onnx (the file NSNet2.zig:56 names) with a built-in protobuf
 * reader; dimensions are taken from the file. */
int fvad_load_nsnet2_onnx(fvad_ctx *ctx, const char *onnx_path);
/* Takes weights from host memory (copied). */
int fvad_load_nsnet2_weights(fvad_ctx *ctx, const fvad_nsnet2_weights *w);
/* Seeded synthetic weights of the NSNet2-baseline architecture (for benchmarks and tests: the
 * real model file is not redistributable here). */
int fvad_load_nsnet2_synth(fvad_ctx *ctx, uint64_t seed);
/* Borrow the host copy of the loaded weights (valid until the next load / ctx destroy). */
int fvad_get_nsnet2_weights(const fvad_ctx *ctx, fvad_nsnet2_weights *out);
/* Host-only helpers (no device needed): */
int fvad_onnx_read_nsnet2(const char *onnx_path, fvad_nsnet2_weights *out, void **owner);
int fvad_synth_nsnet2(uint64_t seed, fvad_nsnet2_weights *out, void **owner);
void fvad_weights_free(void *owner);

/* ------------------------------------------------------------------ B3: FFT  (src/FFT.zig)
 * Replaces FFT.init/fft/invFft/deinit and, underneath, kiss_fftr_alloc / kiss_fftr /
 * kiss_fftri / kiss_fftr_free (FFT.zig:52-57,108-112,129-133,79). */
typedef struct { float r, i; } fvad_complex; /* FFT.zig:12-14 */
typedef struct fvad_fft fvad_fft;

/* FFT.init(allocator, n_fft, sample_rate, mode_inverse)  FFT.zig:35-76.  Any even n_fft from 4 to 16384, forward or inverse,
 * like kiss_fftr_alloc (odd or zero: FVAD_ERR_INVALID_FFT_SIZE, FFT.zig:41-43; so are 2 and sizes past 16384, this library's
 * limits).  The sizes the pipeline runs at have wavefront kernels -- 320 (forward and inverse: NSNet2's STFT), 512 / 1024 /
 * 2048 (forward: the VAD-side transform, VADPipeline.Config.fft_size); every other case runs on a generic mixed-radix kernel
 * (one workgroup per frame, any radix; correct, not tuned). */
int fvad_fft_create(fvad_ctx *ctx, size_t n_fft, size_t sample_rate, int mode_inverse,
                    fvad_fft **out);
void fvad_fft_destroy(fvad_fft *fft);                                   /* FFT.deinit :78-83 */
/* FFT.fft(samples: SplitSlice, window, bins)  FFT.zig:85-113.  Host pointers. */
int fvad_fft_forward(fvad_fft *fft, const float *first, size_t n_first, const float *second,
                     size_t n_second, const float *window, size_t n_window, fvad_complex *bins,
                     size_t n_bins);
/* FFT.invFft(bins, result)  FFT.zig:115-134: unscaled inverse (== n_fft * x). */
int fvad_fft_inverse(fvad_fft *fft, const fvad_complex *bins, size_t n_bins, float *result,
                     size_t n_result);
size_t fvad_fft_bin_count(const fvad_fft *fft);                         /* FFT.zig:137-139 */
float fvad_fft_bin_width(const fvad_fft *fft);                          /* :142-147 */
float fvad_fft_nyquist_freq(const fvad_fft *fft);                       /* :150-153 */
int fvad_fft_freq_to_bin(const fvad_fft *fft, float freq, size_t *bin); /* :156-167 */
int fvad_fft_bin_to_freq(const fvad_fft *fft, size_t bin, float *freq); /* :170-180 */
/* The batched form the GPU wants (BASELINE config 2): n_frames contiguous frames of n_fft
 * samples -> bins [n_frames][n_fft/2+1] and/or magnitudes [n_frames][n_fft/2+1]; either output
 * may be NULL.  `on_device` != 0: all pointers are device pointers and the call only enqueues. */
int fvad_fft_forward_batch(fvad_fft *fft, const float *frames, size_t n_frames,
                           const float *window, fvad_complex *bins, float *magnitudes,
                           int on_device);

/* window_fn.zig:22-41, 8-16 and NSNet2.zig:384-396 (host; same f32 arithmetic as the reference) */
void fvad_hann_window_periodic(float *result, size_t n);
void fvad_hann_window_symmetric(float *result, size_t n);
float fvad_window_norm_factor(const float *window, size_t n);
void fvad_nsnet2_window(float *window320);

/* ------------------------------------------------------------------ B2: NSNet2 (src/NSNet2.zig) */
typedef struct fvad_nsnet2 fvad_nsnet2;
/* NSNet2.init(allocator, sample_rate, model_path)  NSNet2.zig:35-142.  The model comes from the
 * context.  One object per channel, like BufferedDenoiser.zig:38-41.  sample_rate: any multiple of
 * 16000 Hz like the reference (resample.zig:4-7: calcDownsampleRate), FVAD_ERR_INVALID_SAMPLE_RATE
 * otherwise; chunks are fvad_nsnet2_chunk_size(sample_rate) = 8000 * (sample_rate / 16000) samples. */
int fvad_nsnet2_create(fvad_ctx *ctx, size_t sample_rate, fvad_nsnet2 **out);
void fvad_nsnet2_destroy(fvad_nsnet2 *d);                               /* NSNet2.zig:144-155 */
size_t fvad_nsnet2_chunk_size(size_t in_sample_rate);                   /* NSNet2.zig:157-159 */
/* The lag of the denoised samples behind the input's (host only): denoised[n] belongs to input[n - *delay], in samples of
 * in_sample_rate = r * 16000.  Two parts.  NSNet2 keeps the previous chunk's last hop in front of its input
 * (NSNet2.zig:175-197: audio_input[0..n_hop] is the last n_hop samples of the chunk before), so the network's output sample j
 * belongs to its input sample j - 160: 160 samples of 16 kHz, 160 r of the input.  And the up-sampler writes r - 1 interpolated
 * samples IN FRONT of every network sample (resample.zig:44-46: "[interp1, interp2, first, ...]"), so network sample j lies at
 * output index r j + (r - 1), while the down-sampler took it from input index r j (resample.zig:20-21).  Together
 * denoised[r j + r - 1] belongs to input[r (j - 160)]: *delay = 161 r - 1, 482 at 48000 (160 at 16000, 321 at 32000).  The
 * interpolated samples in between are a linear blend of two neighbours and have no single partner; at 48000 the samples that
 * have one are those at 2 modulo 3.  Whoever mixes or subtracts the two without this shift builds a comb filter.
 * FVAD_ERR_INVALID_SAMPLE_RATE for the rates fvad_nsnet2_create refuses, FVAD_ERR_INVALID_ARGUMENT for NULL. */
int fvad_nsnet2_delay(size_t in_sample_rate, uint64_t *delay);
/* NSNet2.denoise(samples: SplitSlice, denoised_result)  NSNet2.zig:161-237.  Host pointers;
 * carries the same cross-chunk state (input hop, overlap-add tail, 4 feature rows,
 * last_sample: NSNet2.zig:27-33). */
int fvad_nsnet2_denoise(fvad_nsnet2 *d, const float *first, size_t n_first, const float *second,
                        size_t n_second, float *denoised_result, size_t n_result);

/* ------------------------------------------------------------------ batched engine
 * What simulator.zig would call with preload_audio = true: whole streams in, per-stream VAD
 * inputs out.  A "lane" is one channel of one stream.  For every lane the engine runs, for all
 * complete 24000-sample chunks at once: chunk RMS (BufferedVolumeAnalyzer.zig:48-69), decimate +
 * sqrt-Hann STFT-320 + log-power features (NSNet2.zig:205-219), NSNet2 (NSNet2.zig:220), gain +
 * inverse STFT overlap-add + x3 upsample (NSNet2.zig:221-236), then the 1024-point periodic-Hann
 * rFFT magnitude and 500-2000 Hz band sum of the denoised audio (BufferedFFT.zig:162-202). */
typedef struct fvad_lane_state fvad_lane_state; /* cross-call carry of one lane (device) */
int fvad_lane_state_create(fvad_ctx *ctx, fvad_lane_state **out);
void fvad_lane_state_reset(fvad_lane_state *s);
void fvad_lane_state_destroy(fvad_lane_state *s);
/* Time-split sharding of ONE long stream over several GPUs (BASELINE config 5).  The ONNX
 * session carries no state across chunks (NSNet2.zig:57-58,71-112), so what crosses a chunk edge is short: the
 * 160-sample input hop, the 4 warm-up feature rows, the overlap-add tail and the upsampler's last sample
 * (NSNet2.zig:27-33,188-203), all functions of the previous chunk and of the 4 last frames of the one before.  A
 * lane that starts TWO chunks early from zero history (this call, sample_index = 24000 * (c0 - 2)) is therefore
 * bit-identical to the unsplit stream from chunk c0 on -- when both runs select the same kernels (see
 * fvad_ctx_set_option: "reproducible"; ~1e-6 apart otherwise) --; the VAD FFT's frame grid stays anchored at sample 0
 * (first_frame_index of the next fvad_engine_run says where the lane's first frame starts).  The caller drops
 * the two warm-up chunks and the frames that start before 24000 * c0.  sample_index: a multiple of 24000. */
int fvad_lane_state_seek(fvad_lane_state *s, uint64_t sample_index, size_t fft_size /* 0 = 1024 */);

typedef struct {
    const float *pcm;        /* n_samples f32 @48 kHz (host or device, see on_device); NULL: use pcm_i16 */
    size_t n_samples;        /* only floor(n/24000) chunks are consumed */
    fvad_lane_state *state;  /* NULL = fresh stream (zero history), state not kept */
    float *denoised;         /* out, optional: n_chunks*24000 f32 (same memory space as pcm) */
    float *band_sum;         /* out: one f32 per completed 1024-sample frame */
    size_t band_sum_capacity;
    float *chunk_rms;        /* out: one f32 per chunk */
    size_t chunk_rms_capacity;
    float *fft_bins;         /* out, optional (parity/debug): [n_fft_frames][513] magnitudes */
    /* 16-bit transport: the reference decodes PCM16 files to f32 on the host (AudioFileStream.zig:56-102 through
     * libsndfile: s / 32768); here the samples can cross PCIe and HBM as PCM16 and are converted by the kernel
     * that reads them, bit-identical to converting first. */
    const int16_t *pcm_i16;  /* used when pcm == NULL: n_samples PCM16 samples (same memory space as pcm would be) */
    int16_t *denoised_i16;   /* out, optional: n_chunks*24000 samples, rint(clamp(y * 32768, -32768, 32767)) */
    float *spectrogram;      /* out, optional (parity/debug, host): [n_chunks][50][161] {r,i} -- NSNet2.calcSpectrogram's
                                bins before the gain (NSNet2.zig:239-264) */
    float *features;         /* out, optional (parity/debug, host): [n_chunks][54][161] -- the ONNX input rows: 4 warm-up
                                rows (previous chunk's last 4, zeros at t = 0) + calcFeatures (NSNet2.zig:188-203,266-287) */
    /* filled by the call: */
    size_t n_chunks;         /* chunks consumed */
    size_t n_fft_frames;     /* band sums written */
    uint64_t first_frame_index; /* absolute sample index of the first FFT frame's window */
} fvad_lane;

typedef struct {
    int32_t on_device;       /* pcm/denoised are device pointers; outputs band_sum/chunk_rms/
                                fft_bins are always host pointers */
    int32_t min_bin;         /* band edges, inclusive; default 11..43 = freqToBin(500/2000) */
    int32_t max_bin;
    int32_t max_chunks_per_launch; /* 0 = default (49152) */
    int32_t fft_size;        /* frame length of the VAD-side FFT (VADPipeline.Config.fft_size, VADPipeline.zig:21): any even
                                size from 4 to 16384 (512, 1024, 2048: wavefront kernels; others: the generic kernel);
                                0 = 1024.  min_bin / max_bin index that transform's bins and fft_bins rows have
                                fft_size / 2 + 1 entries */
    int32_t no_wait;         /* fvad_engine_enqueue_device* only: 1 = return as soon as the work is queued on the
                                context's stream (results valid after fvad_ctx_synchronize or an event the caller
                                records on fvad_ctx_stream); the next call may be made at once -- descriptor and job
                                tables are double-buffered -- so a caller can keep one batch queued behind the running
                                one.  0 (default) = return when the work has completed */
    int32_t use_graph;       /* fvad_engine_enqueue_device* only: 1 = the call's launch sequence (K1, the NSNet2 kernels,
                                K3 per launch, then K4) is captured into a hipGraph the first time and replayed while the
                                arguments, the model and the workspace stay the same -- the "hipGraph-captured steady-state
                                frame loop" of a long corpus processed batch after batch through the same buffers.  Results
                                are bit-identical to direct launches.  The call returns when the work has completed. */
} fvad_engine_opts;
void fvad_engine_opts_default(fvad_engine_opts *o);

int fvad_engine_run(fvad_ctx *ctx, fvad_lane *lanes, size_t n_lanes, const fvad_engine_opts *opts);

/* Device-resident form: `d_pcm` holds n_lanes lanes of n_samples (lane l at d_pcm + l * lane_stride);
 * d_denoised [n_lanes][n_chunks*24000] (NULL: kept in the context's workspace), d_band_sum
 * [n_lanes][n_chunks*24000/1024] and d_chunk_rms [n_lanes][n_chunks] (may be NULL) are device buffers
 * too; nothing is copied to the host.  Every lane starts from zero history.  The call returns once
 * the work has COMPLETED on the context's stream, unless opts->no_wait is set. */
int fvad_engine_enqueue_device(fvad_ctx *ctx, const float *d_pcm, size_t n_lanes,
                               size_t lane_stride, size_t n_samples, float *d_denoised,
                               float *d_band_sum, float *d_chunk_rms,
                               const fvad_engine_opts *opts);
/* The same with PCM16 device buffers in (and optionally out): half the HBM footprint and transport. */
int fvad_engine_enqueue_device_i16(fvad_ctx *ctx, const int16_t *d_pcm16, size_t n_lanes,
                                   size_t lane_stride, size_t n_samples, int16_t *d_denoised16,
                                   float *d_band_sum, float *d_chunk_rms,
                                   const fvad_engine_opts *opts);
/* Band sums of several bands in one pass over device-resident denoised audio: n_bands bands (bins[2j], bins[2j+1]
 * inclusive, a host array) of the fft_size-point periodic-Hann magnitude spectrum of every frame of every lane (lane l
 * at d_denoised + l * lane_stride, frames at k * fft_size, k < n_samples / fft_size); band j of lane l at
 * d_band_sum + (j * n_lanes + l) * band_stride.  Each band's sums have the bits an engine call with min_bin/max_bin =
 * that band gives (FVAD_ERR_OUT_OF_RANGE for bins outside 0..fft_size/2 or max < min).  Frames are read as float pairs:
 * d_denoised must be 8-byte aligned and lane_stride even (FVAD_ERR_INVALID_ARGUMENT otherwise); 16-byte alignment is not
 * needed.  Returns when the work has completed. */
int fvad_engine_band_sums_device(fvad_ctx *ctx, const float *d_denoised, size_t n_lanes, size_t lane_stride,
                                 size_t n_samples, size_t fft_size, const int32_t *bins, size_t n_bands,
                                 float *d_band_sum, size_t band_stride);
/* NSNet2 graph only: features [n_seq][T][161] -> gains [n_seq][T][161] (host pointers).
 * Replaces onnx_instance.run() (NSNet2.zig:220) for n_seq independent sequences. */
int fvad_nsnet2_forward(fvad_ctx *ctx, const float *features, size_t n_seq, size_t T,
                        float *gains);
/* Arithmetic of the NSNet2 matrix products -- a property of the CONTEXT (and of the loaded model), never of a
 * launch's size: every launch of a context, large or small, uses the same one.
 *   FVAD_NN_MATH_F32 (default): v_mfma_f32_16x16x4_f32 throughout (kernels_nn.hip, kernels_ws.hip): f32 operands,
 *     f32 accumulation, each output a k-ordered chain of f32 fmas -- the arithmetic of the reference's ONNX Runtime
 *     CPU kernels (NSNet2.zig:220);
 *   FVAD_NN_MATH_F16X3 (opt-in, an EMULATION that is narrower than f32): every f32 operand as two f16 pieces of a
 *     power-of-two scaled value (22 significand bits, f32 has 24), three f16 MFMAs with f32 accumulation per product
 *     (kernels_h3.hip), batches padded to 128 sequences.  Measured against float64 as close as the f32 kernels on the
 *     models tried (tests), 2.1 x their speed at saturating batches; differs from them by ~1e-6 in the gains.  A
 *     model whose weights are not finite or whose l1 activation bounds exceed 2^17 is not eligible and keeps f32.
 *   FVAD_NN_MATH_BF16X3 (opt-in, an emulation that is NOT narrower than f32): the five dense layers with every f32
 *     operand as three bf16 pieces (x = h + m + l exactly: all 24 significand bits, f32's exponent range, no scales
 *     or bounds) and the six significant cross terms as six bf16 MFMAs with f32 accumulation per product
 *     (kernels_b3.hip); the two GRU recurrences stay on the f32 matrix cores.  Batches padded to 128 sequences.
 *     NSNet2-baseline dimensions only (other models keep f32).
 * fvad_ctx_set_nn_math returns the previous setting or a negative status.  fvad_ctx_nn_math_effective returns what
 * the context actually uses with the model it has loaded (the request, demoted to F32 for an ineligible model or
 * while an f32 kernel variant is forced through fvad_ctx_set_option); fvad_ctx_last_nn_path names the kernels the
 * last NSNet2 pass ran, e.g. "f32: panel_gemm3 (fc1 folded) + gru_rec3<12>". */
enum { FVAD_NN_MATH_F32 = 0, FVAD_NN_MATH_F16X3 = 1, FVAD_NN_MATH_BF16X3 = 2 };
int fvad_ctx_set_nn_math(fvad_ctx *ctx, int mode);
int fvad_ctx_nn_math_effective(const fvad_ctx *ctx);
const char *fvad_ctx_last_nn_path(const fvad_ctx *ctx);
/* A test tap, not needed in production: what the context's LAST NSNet2 pass left in the workspace for its sequences
 * [first_seq, first_seq + n_seq), as out[seq][row][unit] (f32, host pointer, room for n_seq * rows * width floats: at most
 * n_seq * T * 600).  Waits for the context's stream, then copies; launches no kernel and changes none.
 *   layer               rows per sequence   width
 *   FVAD_NN_TAP_H1      T                   400    first GRU's states
 *   FVAD_NN_TAP_H2      T                   400    second GRU's states
 *   FVAD_NN_TAP_F2      T - skip            600    relu(fc2); row r is step skip + r
 *   FVAD_NN_TAP_F3      T - skip            600    relu(fc3)
 *   FVAD_NN_TAP_GAINS   T - skip            161    sigmoid(fc4): what K3 applies
 * T and skip are the pass's: fvad_nsnet2_forward's T and 0; 54 and 4 in the engine, where a sequence is a chunk and row 0..3
 * its warm-up rows.  After an fvad_engine_* or pipeline call the tap describes that call's LAST LAUNCH (a call may be cut into
 * several: max_chunks_per_launch, or the engine's plan), sequences in launch order, lane-contiguous.  *rows_per_seq and *width
 * are written on success.
 * FVAD_ERR_NOT_AVAILABLE (never stale memory) when no pass has run, when a workspace buffer was reallocated or a model loaded
 * since, and for a layer the pass's kernels never write row-major: h1 of the pipelined small-batch recurrence (gru_ws2k /
 * gru_ws2m hand it on through their exchange buffer; also in the rare pass whose fallback launch did write it: the tap does
 * not look at the fallback counter), every layer of the f16x3 / bf16x3 emulations (split fragments) and of a
 * model of other dimensions.  FVAD_ERR_INVALID_ARGUMENT for a NULL pointer, n_seq == 0, an unknown layer, or sequences past the
 * pass's real ones (the batch's padding is not tapped). */
enum { FVAD_NN_TAP_H1 = 0, FVAD_NN_TAP_H2 = 1, FVAD_NN_TAP_F2 = 2, FVAD_NN_TAP_F3 = 3, FVAD_NN_TAP_GAINS = 4 };
int fvad_ctx_nn_tap(fvad_ctx *ctx, int layer, size_t first_seq, size_t n_seq, float *out, size_t *rows_per_seq, size_t *width);
/* Bit-reproducibility.  Two launches that select the same NSNet2 kernels (fvad_ctx_last_nn_path names them) give a
 * chunk the same bits wherever in the batch it sits and however lanes and chunks are split.  With FVAD_NN_MATH_F32
 * the engine selects by launch size: up to 1536 sequences the pipelined two-layer weight-stationary recurrence (it
 * computes layer 2's input projection itself, and for 65..96 sequences layer 1's too, in the accumulation order of the GEMM
 * that otherwise runs in front: one set of bits for the whole range);
 * up to 2047 the narrow-block GEMMs with a weight-stationary or the low-latency recurrence; from 2048 the persistent GEMM
 * with the low-latency or the multi-wavefront recurrence (by a cost model over the CU count).  A call whose launch size
 * is left to the engine (max_chunks_per_launch = 0) is cut into launches that fill the chip: 1537..3400 chunks run as two or
 * three equal launches, larger calls as launches of 4096 / 8192 / 12288 / 16384 / 32768 / 49152 chunks and a remainder where
 * the measured curve says that pays (5120 = 4096 + 1024).  Every selection runs f32 operands and f32 accumulation; they differ in
 * accumulation order and agree to ~1e-6 in the gains, not bit for bit.  The option "reproducible" = "1" makes every
 * launch use one selection (persistent GEMM + multi-wavefront recurrence; small launches are padded to 128 sequences
 * and lose their low-latency kernels), so that a stream pushed in any pieces, split over any number of launches or
 * time-split over ranks gives the same bits.  FVAD_NN_MATH_F16X3 and FVAD_NN_MATH_BF16X3 have one selection each.
 *
 * Testing / tuning aids, none needed in production: name = "reproducible" | "nn_math" ("f32" | "f16x3" | "bf16x3": overrides
 * fvad_ctx_set_nn_math) | "gru_kernel" ("v3w12" | "v3w8" | "v3w4" | "v4w8" | "v5w0" | "v6w0") | "gemm_kernel" ("v1" |
 * "v3" | "v3nofold") | "h3_waves" ("8" | "12") | "max_chunks" | "copy_threads" | "ingest_ring_bytes" (fvad_ingest's raw bytes per batch; same bits) | "no_pipeline" | "run_groups" ("1,3,4,8": the lane groups of
 * fvad_engine_run's host-buffer pipeline in sixteenths of the call, at most seven, instead of the planned ones) | "trace_run" (a timeline of every fvad_engine_run call on stderr) | "trace_kernels" |
 * "ws_spin_ticks" | "ws2_variant" (diagnostic bit mask; the timing-only bits exist in the diagnostics build alone) |
 * "ws2_waits" | "ws2_calibrate" (below) | "nn_trim" ("all" | "tiles" | "rows" | "none": what the persistent f32 kernels skip -- "tiles": the MFMAs of
 * fc2 / fc3's all-padding 39th column tile; "rows": layer 1's input projection of a chunk's four warm-up rows, which the recurrence reads from the
 * previous chunk of the lane instead, in fvad_engine_* launches whose lanes all have the same number of chunks (fvad_ctx_last_nn_path then ends in
 * ", gi1 rows 4..53"); same bits whatever the value) | "k4_plain_loads" (the band FFT's staging path of unaligned frames) | "gru_lat_tiles" ("1" | "2" | "3": row tiles per
 * workgroup of the low-latency recurrence instead of the cost model's choice; same bits) | "vad_trigger" ("config" | "shared") | "vad_trigger_max_bytes" (see fvad_vad_batch_trigger_form) | "vad_avgs" ("ring" | "table") | "vad_avgs_max_bytes" (see fvad_vad_batch_avgs_form) | "vad_chain" ("lane" | "coop": the exact
 * long-term chains of the device VAD machines lane by lane or by the whole wavefront, see fvad_vad_batch_run_device_part; same bits);
 * value NULL or ""
 * restores the default.  The environment variables FVAD_<NAME> are read ONCE, by
 * fvad_ctx_create, as initial values (a bad value fails the creation); the data path never reads the environment. */
int fvad_ctx_set_option(fvad_ctx *ctx, const char *name, const char *value);
/* Network passes in which a weight-stationary small-batch recurrence (gru_ws_kernel, or the pipelined gru_ws2k / gru_ws2m /
 * gru_ws2) gave up waiting for a peer workgroup -- the chip was shared with another process, or with a long kernel of another
 * context of this process -- and the low-latency kernel redid the GRU layers.  A spin gives up after max(2 ms, 20 x the
 * launch's own expected duration) (option "ws_spin_ticks" overrides).  Bits: gru_ws and its fallback accumulate in the same
 * order (same bits); the pipelined kernels compute layer 2's input projection in the kernel and their fallback does not, so
 * a pass that fell back differs from one that did not by round-off (<= 2e-6 in the gains): default-mode results of small
 * launches are load-dependent within that bound.  "reproducible" = "1" never runs these kernels.  Waits for the context's
 * stream. */
int fvad_ctx_ws_fallbacks(fvad_ctx *ctx, uint64_t *n);
/* The pipelined recurrence of launches up to 96 sequences (gru_ws2k) waits a fixed interval before a step's first poll of
 * its peers' flags -- a poll made too early is a wasted round trip and traffic on the flag lines.  The intervals are a
 * built-in table per group shape (wait_class 1: groups of 25 + 25 workgroups, 1..80 sequences; 2 and 3: groups of 13 + 25,
 * without / with layer 1's input projection in the kernel), swept on one MI355X.  fvad_ctx_set_option(ctx, "ws2_calibrate",
 * "1") measures them on THIS device (about 0.2 s, the model must be loaded; the table's entry stays unless a candidate is
 * more than 1.5 % faster); "ws2_waits" = layer 1's wait | layer 2's << 16, in 10 ns ticks, sets them by hand for every class.
 * Timing only: results do not depend on them.  Returns the waits in effect for a class, packed like "ws2_waits"; 0 for an
 * unknown class. */
uint32_t fvad_ctx_ws2_waits(const fvad_ctx *ctx, int wait_class);
/* Per-kernel device time of the last fvad_engine_* call (HIP events on the context's stream):
 * names[i]/ms[i] for i < *n.  Enabled by fvad_ctx_enable_timing(ctx, 1). */
int fvad_ctx_enable_timing(fvad_ctx *ctx, int on);
int fvad_ctx_kernel_times(fvad_ctx *ctx, const char **names, float *ms, size_t cap, size_t *n);

/* ------------------------------------------------------------------ VAD state machine (host)
 * src/AudioPipeline/VADMachine.zig + src/structures/RollingAverage.zig, exact f64 order. */
typedef struct {
    float speech_min_freq;             /* 500   VADMachine.zig:32 */
    float speech_max_freq;             /* 2000  :33 */
    float long_term_speech_avg_sec;    /* 180   :35 */
    int32_t has_initial_long_term_avg; /* 1     :36 (?f64) */
    double initial_long_term_avg;      /* 0.005 */
    float short_term_speech_avg_sec;   /* 0.2   :38 */
    float speech_threshold_factor;     /* 10    :41 */
    float channel_vol_ratio_avg_sec;   /* 0.5   :43 */
    float channel_vol_ratio_threshold; /* 0.5   :44 */
    float min_consecutive_sec_to_open; /* 0.2   :46 */
    float max_speech_gap_sec;          /* 2     :48 */
    float min_vad_duration_sec;        /* 0.7   :50 */
} fvad_vad_config;
void fvad_vad_config_default(fvad_vad_config *c);

typedef struct {
    uint64_t sample_from, sample_to;
    float avg_channel_vol_ratio, vad_met_sec;
} fvad_speech_segment; /* VADPipeline.SpeechSegment, VADPipeline.zig:28-33 */

enum { FVAD_REC_NONE = 0, FVAD_REC_STARTED = 1, FVAD_REC_COMPLETED = 2, FVAD_REC_ABORTED = 3 };
typedef struct { int32_t recording_state; uint64_t sample_number; } fvad_vad_result; /* :18-28 */

/* smallest decision margins seen so far (the "margin audit" of SURVEY.md section 7): how close
 * any frame came to flipping `short_term > threshold` or `ratio > 0.5` */
typedef struct {
    double min_rel_threshold_margin; /* min |short_term - threshold| / threshold */
    double min_abs_ratio_margin;     /* min |channel_vol_ratio - ratio_threshold| */
    uint64_t n_frames;
} fvad_vad_audit;

typedef struct fvad_vad fvad_vad;
int fvad_vad_create(const fvad_vad_config *cfg, size_t sample_rate, size_t n_channels,
                    size_t fft_size, fvad_vad **out);                  /* VADMachine.init :75-128 */
void fvad_vad_destroy(fvad_vad *v);
/* VADMachine.run(fft_result)  VADMachine.zig:138-239 with the band volumes already summed. */
int fvad_vad_run(fvad_vad *v, uint64_t index, const float *channel_volumes, int has_ratio,
                 float volume_ratio, fvad_vad_result *out);
size_t fvad_vad_segment_count(const fvad_vad *v);
int fvad_vad_segments(const fvad_vad *v, fvad_speech_segment *out, size_t cap, size_t *n);
int fvad_vad_audit_get(const fvad_vad *v, fvad_vad_audit *out);
/* How often the long-term average's full chain (RollingAverage.zig:45-56) had to be run: this build
 * evaluates it lazily, only when a bound on the incrementally carried value cannot settle the threshold
 * comparison (results are identical either way; see host_vad.cpp). */
int fvad_vad_lazy_stats(const fvad_vad *v, uint64_t *exact_evaluations, uint64_t *lazy_pushes);
/* Many independent streams at once, bit-identical to fvad_vad_run per stream: the streams are dealt to
 * n_threads host threads (stream s -> thread s % n_threads; one thread per file is the reference's own
 * parallelism, simulator.zig:221-232) and each thread runs its streams one after the other.
 * band[s] points at [n_frames[s]][n_channels] f32, ratio[s] at [n_frames[s]].
 * first_index[s] + fft_size*k is frame k's index. */
int fvad_vad_run_many(fvad_vad *const *vads, size_t n_streams, const float *const *band,
                      const float *const *ratio, const size_t *n_frames, size_t n_channels,
                      const uint64_t *first_index, size_t fft_size, int n_threads);

/* The host stage of a whole batch in one call, straight from the engine's lane-major outputs (lane = stream *
 * n_channels + channel): per-chunk volume ratio (BufferedVolumeAnalyzer.zig:48-69), the metadata hand-overs
 * (BufferedVolumeAnalyzer.zig:33-45, BufferedDenoiser.zig:83-86,115), the sample-weighted ratio of every FFT
 * frame (BufferedFFT.zig:137-140,153), then VADMachine.run per frame on fresh machines (VADMachine.zig:138-239),
 * streams dealt to n_threads host threads.  band: lane l's n_frames sums at band + l * band_stride; chunk_rms:
 * lane l's n_chunks values at chunk_rms + l * rms_stride; chunk_size = 24000 at 48 kHz (NSNet2.zig:157-159).
 * Bit-identical to fvad_pipeline_* / fvad_vad_run on the same numbers. */
typedef struct fvad_vad_batch fvad_vad_batch;
int fvad_vad_batch_create(const fvad_vad_config *cfg, size_t sample_rate, size_t n_channels,
                          size_t fft_size, size_t n_streams, fvad_vad_batch **out);
void fvad_vad_batch_destroy(fvad_vad_batch *b);
int fvad_vad_batch_run(fvad_vad_batch *b, const float *band, size_t band_stride, size_t n_frames,
                       const float *chunk_rms, size_t rms_stride, size_t n_chunks, size_t chunk_size,
                       int n_threads);
/* The same in parts: frames [first_frame, first_frame + n_frames) of every stream, the streams' machines living on between
 * the calls, so that a host can run the VAD of the part it has while the GPU produces the next one.  first_frame = 0 starts
 * from fresh machines (fvad_vad_batch_run is this with first_frame = 0); a later part must start where the previous one
 * ended, on a chunk boundary (first_frame * fft_size a multiple of chunk_size: at 48 kHz and fft_size 1024 every 375 frames
 * = 16 chunks), and band / chunk_rms point at the part's first frame / first chunk.  Segments and audits (below) cover
 * everything run so far.  Bit-identical to one fvad_vad_batch_run over all the frames. */
int fvad_vad_batch_run_part(fvad_vad_batch *b, const float *band, size_t band_stride, size_t n_frames,
                            const float *chunk_rms, size_t rms_stride, size_t n_chunks, size_t chunk_size,
                            uint64_t first_frame, int n_threads);
size_t fvad_vad_batch_total_segments(const fvad_vad_batch *b);
/* all segments, stream after stream; offsets[s] .. offsets[s + 1] are stream s's (offsets has n_streams + 1 entries) */
int fvad_vad_batch_segments(const fvad_vad_batch *b, fvad_speech_segment *out, size_t cap,
                            size_t *offsets);
int fvad_vad_batch_audit(const fvad_vad_batch *b, size_t stream, fvad_vad_audit *out);

/* Parameter sweeps: a batch of n_configs VADMachine.Configs over the same streams, one machine per (stream, config) --
 * the reference's alt_vad_machine_configs (VADPipeline.zig:110-122,231-236) with every machine on its own speech band
 * (VADMachine.zig:146-151).  Each config is checked like fvad_vad_create / fvad_pipeline_create do it (speech band above
 * Nyquist: FVAD_ERR_OUT_OF_RANGE; a negative edge: FVAD_ERR_NEGATIVE_FREQUENCY; max bin < min bin or a channel-ratio ring
 * of length 0: FVAD_ERR_INVALID_ARGUMENT).  fvad_vad_batch_run / _run_part take a sweep batch too: `band` then holds
 * n_bands consecutive [n_lanes][band_stride] blocks (fvad_vad_batch_bands' order), config c reading block band_of[c].
 * fvad_vad_batch_segments / _total_segments / _audit give config 0's results. */
int fvad_vad_batch_create_sweep(const fvad_vad_config *cfgs, size_t n_configs, size_t sample_rate, size_t n_channels,
                                size_t fft_size, size_t n_streams, fvad_vad_batch **out);
size_t fvad_vad_batch_n_configs(const fvad_vad_batch *b); /* 1 for fvad_vad_batch_create */
/* distinct speech bands of the configs (FFT.freqToBin of speech_min/max_freq, as fvad_pipeline_create computes them),
 * bins[2j], bins[2j+1], in first-seen config order; band_of[c] = the band of config c (may be NULL) */
int fvad_vad_batch_bands(const fvad_vad_batch *b, int32_t *bins, size_t cap, size_t *n_bands, uint32_t *band_of);
/* config `config`'s segments, stream after stream, like fvad_vad_batch_segments */
int fvad_vad_batch_config_segments(const fvad_vad_batch *b, size_t config, fvad_speech_segment *out, size_t cap,
                                   size_t *offsets);
int fvad_vad_batch_config_audit(const fvad_vad_batch *b, size_t stream, size_t config, fvad_vad_audit *out);
/* fvad_vad_lazy_stats of machine (stream, config) in the last run, host or device */
int fvad_vad_batch_lazy_stats(const fvad_vad_batch *b, size_t stream, size_t config, uint64_t *exact_evaluations,
                              uint64_t *lazy_pushes);
/* Every (stream, config) machine of b on the GPU (csrc/kernels_vad.hip); d_band as fvad_engine_band_sums_device writes it
 * (band j of lane l at d_band + (j * n_lanes + l) * band_stride, lane = stream * n_channels + channel); stream s has
 * n_frames[s] frames and n_chunks[s] chunks (host arrays; chunk_rms on the host: lane l's values at
 * chunk_rms + l * rms_stride).  Returns when the segments and audits are in b; bit-identical to fvad_vad_batch_run. */
int fvad_vad_batch_run_device(fvad_ctx *ctx, fvad_vad_batch *b, const float *d_band, size_t band_stride,
                              const size_t *n_frames, const float *chunk_rms, size_t rms_stride,
                              const size_t *n_chunks, size_t chunk_size);
/* The same in parts, for streams longer than device memory holds: frames [first_frame, first_frame + n_frames[s]) of stream
 * s, d_band and chunk_rms pointing at the part's first frame and first chunk (as fvad_vad_batch_run_part takes them); the
 * machines' state stays in device memory between the parts (csrc/kernels_vad.hip's resume form).  first_frame = 0 starts
 * fresh machines and drops any earlier part state.  A later part must start where the previous device part ended, on a chunk
 * boundary (first_frame * fft_size a multiple of chunk_size), on the same context; a stream given fewer frames than the
 * part's longest has ended, and every later part must give it 0 frames and 0 chunks.  Host and device parts do not mix: a
 * device part with first_frame > 0 after a host run, a one-shot device run or a failed part, and a host fvad_vad_batch_run_part
 * with first_frame > 0 after a device part, return FVAD_ERR_INVALID_ARGUMENT (as does every other broken rule).  After each
 * part the segments, audits and lazy statistics in b cover everything run so far, bit-identical to one
 * fvad_vad_batch_run_device (and fvad_vad_batch_run) over all the frames, for every partition.  With keep_segments 1 each part's
 * new segments are appended to b's; with 0 they stay in device memory (only counts, audits and statistics come back) for
 * fvad_vad_batch_score_device.  A part never scores.  Segments are never truncated: a machine that fills its room (context
 * option vad_seg_cap, as for the one-shot run) pauses, the room grows and the part goes on.
 * fvad_vad_batch_score_device: the statistics of the device-held segments of the parts run so far (read them with
 * fvad_vad_batch_config_stats), bit-identical to fvad_vad_batch_score on the same segments; FVAD_ERR_INVALID_ARGUMENT without
 * references, without device part state, or when a part kept its segments on the host (score those with fvad_vad_batch_score).
 * fvad_vad_batch_device_bytes: the device memory b holds between parts (0 without part state).
 * A batch holding part state owns device memory of its context: destroy the batch before the context.
 * Context option vad_chain ("lane", the default, or "coop"; FVAD_VAD_CHAIN): how the machines' kernel runs an exact long-term
 * chain (csrc/kernels_vad.hip).  "lane": each lane runs its own machine's chain, the other lanes of its wavefront idling through
 * it.  "coop": the 64 lanes of the wavefront load the ring of the machine that needs the chain together and the additions run
 * over it in the reference's order.  Every result (segments, audits, lazy statistics, scores, the state between parts) has the
 * same bits with either, so the option is read at every launch of _run_device(_sized), _run_device_part(_sized), _part_async
 * and of a part's relaunch after its segment room grew, and may change between the parts of a run.
 * fvad_vad_batch_chain_form: *form = 0 before the batch's first device launch, 1 when its last device launch ran the lane form,
 * 2 when it ran the cooperative form (a launch is counted when it is queued: after _part_async already).  The engine never
 * refuses "coop": its LDS (two chain tiles of 8 KB on top of the short rings' at most 48 KB) fits every batch, so 1 is only
 * ever reported with vad_chain "lane". */
int fvad_vad_batch_run_device_part(fvad_ctx *ctx, fvad_vad_batch *b, const float *d_band, size_t band_stride,
                                   const size_t *n_frames, const float *chunk_rms, size_t rms_stride,
                                   const size_t *n_chunks, size_t chunk_size, uint64_t first_frame);
int fvad_vad_batch_score_device(fvad_ctx *ctx, fvad_vad_batch *b);
size_t fvad_vad_batch_device_bytes(const fvad_vad_batch *b);
int fvad_vad_batch_chain_form(const fvad_vad_batch *b, int *form);
/* Keep configs keep[0] < keep[1] < ... < keep[n_keep - 1] of b and drop the rest, between runs or between the parts of a run
 * (successive halving: drop the configs that lose on a prefix, run the survivors on).  Afterwards b is in every observable way
 * the batch fvad_vad_batch_create_sweep (or _create_sweep_sized) would make from cfgs[keep[0..n_keep)] (and their sizes) after
 * the same runs or parts; new config c is old config keep[c].
 * - n_configs, the bands and band_of, the frame sizes and size_of_band are the kept configs', recomputed in first-seen order (a
 *   band or a size no kept config uses disappears); segments (host or device), audits, lazy statistics, held scores, stat configs
 *   and segment counts are restricted to the kept configs; references stay as set.
 * - Allowed on a batch that has not run, after host runs and parts, after a one-shot device run (its results in b are compacted)
 *   and between device parts: every later part, host or device, sized or not, gives the bits a fresh batch of the kept configs
 *   would give over all the parts.
 * - Between device parts the machines' state is gathered on the device (csrc/kernels_vadretain.hip) into new buffers of the kept
 *   machines' size -- the rings as long as the longest kept config needs, in LDS or global memory as the kept configs allow --
 *   and then the old state is freed: for the call, device memory peaks at the old plus the new fvad_vad_batch_device_bytes.
 * - ctx may be NULL unless b holds device part state; then it must be the parts' context.
 * FVAD_ERR_INVALID_ARGUMENT for n_keep == 0, a list not strictly increasing, an index >= n_configs, NULL arguments or the wrong
 * context.  On any error (allocation failures included) b is unchanged and still usable. */
int fvad_vad_batch_retain_configs(fvad_ctx *ctx, fvad_vad_batch *b, const uint32_t *keep, size_t n_keep);

/* Sweeps over the FFT size (VADPipeline.Config.fft_size): config c's machines run on frames of fft_sizes[c] samples (each even,
 * 4 .. 16384, else FVAD_ERR_INVALID_ARGUMENT; each config checked as fvad_vad_batch_create_sweep checks it, at its own size).
 * - A band is the triple (size, min bin, max bin): the same Hz edges at two sizes are two bands, their bins from FFT.freqToBin
 *   at each size.  fvad_vad_batch_bands lists them size-major -- every band of size 0, then of size 1, ... -- in first-seen
 *   config order within a size, so that each size's bands are one run of blocks (one fvad_engine_band_sums_device call per
 *   size on the same denoised audio fills them).  With one size the order is fvad_vad_batch_create_sweep's.
 * - `band` / `d_band` hold the blocks with one band_stride for every size, at least the largest frame count of any size.
 * - The distinct sizes are in first-seen config order (size g); fvad_vad_batch_frame_sizes lists them and size_of_band[j],
 *   the size of band j (may be NULL).  Every batch has frame sizes: one for fvad_vad_batch_create / _create_sweep.
 * - fvad_vad_batch_run_sized: the host machines (the yardstick), every stream the same length as in fvad_vad_batch_run_part;
 *   n_frames[g] frames of size g from sample first_sample on.  fvad_vad_batch_run_device_sized: the device, one shot, as
 *   fvad_vad_batch_run_device (segment room and device scoring alike), with n_frames[g * n_streams + s] frames of size g of
 *   stream s.  fvad_vad_batch_run_device_part_sized: the same in parts, as fvad_vad_batch_run_device_part.  Frame k of a
 *   machine of size F in a part is at sample first_sample + k * F.
 * - Parts: first_sample = 0 starts fresh machines; a later part starts where the previous one ended, and must be a multiple of
 *   chunk_size and of every size (FVAD_ERR_INVALID_ARGUMENT otherwise, as for every other broken part rule).  A part after
 *   which the sizes' frames end at different samples is the last.  A stream given fewer frames of some size than the part's
 *   longest of that size has ended.
 * - The other run calls (_run, _run_part, _run_device, _run_device_part) take a sized batch of exactly one size and then behave
 *   as for a fvad_vad_batch_create_sweep batch; with several sizes they return FVAD_ERR_INVALID_ARGUMENT.  The sized run calls
 *   take every batch.  Segments, audits, lazy statistics, references, keep_segments, scoring (host and device), config_stats
 *   and device_bytes work on sized batches unchanged: segments are in samples, so scoring does not depend on the size.
 * - Context option vad_size_order (vad_lane_map "stream", several sizes): a stream's lanes take its configs "size"-major (the
 *   default: a wavefront mostly runs one frame clock) or in the "caller"'s order; the results are the same bits. */
int fvad_vad_batch_create_sweep_sized(const fvad_vad_config *cfgs, const size_t *fft_sizes, size_t n_configs,
                                      size_t sample_rate, size_t n_channels, size_t n_streams, fvad_vad_batch **out);
int fvad_vad_batch_frame_sizes(const fvad_vad_batch *b, size_t *sizes, size_t cap, size_t *n_sizes,
                               uint32_t *size_of_band);
int fvad_vad_batch_run_sized(fvad_vad_batch *b, const float *band, size_t band_stride, const size_t *n_frames,
                             const float *chunk_rms, size_t rms_stride, size_t n_chunks, size_t chunk_size,
                             uint64_t first_sample, int n_threads);
int fvad_vad_batch_run_device_sized(fvad_ctx *ctx, fvad_vad_batch *b, const float *d_band, size_t band_stride,
                                    const size_t *n_frames, const float *chunk_rms, size_t rms_stride,
                                    const size_t *n_chunks, size_t chunk_size);
int fvad_vad_batch_run_device_part_sized(fvad_ctx *ctx, fvad_vad_batch *b, const float *d_band, size_t band_stride,
                                         const size_t *n_frames, const float *chunk_rms, size_t rms_stride,
                                         const size_t *n_chunks, size_t chunk_size, uint64_t first_sample);

/* Device parts that do not wait: a part's machines beside the next slice's denoising on the same context.
 * - fvad_vad_batch_run_device_part_async: fvad_vad_batch_run_device_part_sized (it takes every batch, n_frames[g * n_streams + s],
 *   the same part rules and the same checks) with the chunk RMS on the DEVICE, as fvad_engine_enqueue_device leaves it
 *   (lane l's chunks at d_chunk_rms + l * rms_stride, from the part's first chunk).  The frame ratios are computed on the device
 *   (csrc/kernels_vadratio.hip, the host's arithmetic from the same header: the same bits), the machines are launched, and the
 *   call returns without waiting.  b's results are those of the previous part until fvad_vad_batch_part_wait has returned.
 * - fvad_vad_batch_part_wait: finishes the part -- waits, grows the segment room and relaunches machines that paused, brings
 *   back counts, audits and lazy statistics, appends the part's segments with keep_segments 1.  Afterwards b is what the blocking
 *   part call would have left, bit for bit.  With nothing in flight it returns FVAD_OK.  A part that fails (in either call)
 *   leaves what a failed blocking part leaves: the run starts again at sample 0.
 * - The part runs on a second stream of the context (created on first use), behind everything queued on the main stream at the
 *   time of the call (the band sums and RMS it reads); nothing on the main stream waits for the part, so engine calls made
 *   between the two calls run beside it.  The kernel-time table (fvad_ctx_set_timing) is the main stream's: it does not list
 *   the part's kernels.  The caller leaves d_band and d_chunk_rms untouched until fvad_vad_batch_part_wait returns.
 * - While a part is in flight every other call that runs, scores, retains, reads results of (segments, audits, statistics) or
 *   sets something on b returns FVAD_ERR_INVALID_ARGUMENT (fvad_vad_batch_total_segments: SIZE_MAX), as do a second _async and a
 *   _part_wait on another context; b stays usable.  fvad_vad_batch_destroy waits for the part; fvad_ctx_synchronize waits for
 *   what the part has queued as well (a paused part's relaunch is still fvad_vad_batch_part_wait's).
 * - fvad_vad_batch_frame_ratios_device: only the frame ratios, row (size g, stream s) at d_ratio + (g * n_streams + s) *
 *   ratio_stride, n_frames[g * n_streams + s] values each (the rest of a row up to the longest row's length is set to 0), on the
 *   context's stream; returns when done.  fvad_vad_batch_frame_ratios: the same rows on the host from host RMS -- what the
 *   blocking device calls hand their machines. */
int fvad_vad_batch_run_device_part_async(fvad_ctx *ctx, fvad_vad_batch *b, const float *d_band, size_t band_stride,
                                         const size_t *n_frames, const float *d_chunk_rms, size_t rms_stride,
                                         const size_t *n_chunks, size_t chunk_size, uint64_t first_sample);
int fvad_vad_batch_part_wait(fvad_ctx *ctx, fvad_vad_batch *b);
int fvad_vad_batch_frame_ratios_device(fvad_ctx *ctx, const fvad_vad_batch *b, const float *d_chunk_rms, size_t rms_stride,
                                       const size_t *n_frames, const size_t *n_chunks, size_t chunk_size,
                                       uint64_t first_sample, float *d_ratio, size_t ratio_stride);
int fvad_vad_batch_frame_ratios(const fvad_vad_batch *b, const float *chunk_rms, size_t rms_stride, const size_t *n_frames,
                                const size_t *n_chunks, size_t chunk_size, uint64_t first_sample, float *ratio,
                                size_t ratio_stride);

/* The short-term and channel-ratio averages from tables (context option vad_avgs: "ring", the default, or "table";
 * FVAD_VAD_AVGS).  VADMachine.run pushes min_volume and the frame's volume ratio into its two short rings whatever it decides, so
 * the two averages of a frame depend on the stream, the frame, the band and the ring length alone: every config with the same
 * short key (band, short-term ring length) has the same short-term average, every config with the same ratio key (size index,
 * channel-ratio ring length) the same ratio average.
 * - "table": before a part's (or a one-shot run's) first launch two kernels (csrc/kernels_vadavgs.hip) fill the min_volume row of
 *   every (band, stream) and, one lane per (key, stream, frame), the two averages -- the reference's chain over the ring's slots
 *   in slot order, with its bits (csrc/vad_avgs.h) -- and the machines read two f64 per frame instead of pushing two rings.  A
 *   launch uses the tables when vad_avgs is "table", vad_chain is "coop" and the part's tables plus min_volume rows fit in
 *   vad_avgs_max_bytes (context option, default 16 GiB); otherwise it pushes the rings.  Either way every result and the state
 *   between parts have the same bits: a table launch leaves the rings and their cursors as the ring form would have, so the
 *   forms may alternate between the parts of a run, and fvad_vad_batch_retain_configs works unchanged.  A relaunch of a part
 *   (after its segment room grew, or the one-shot run's second launch) reads the tables filled before the first.
 * - The tables belong to the batch's device part state: they only grow, are freed with it and count in
 *   fvad_vad_batch_device_bytes.
 * - fvad_vad_batch_avgs_form: *form = 0 before the batch's first device launch, 1 when its last device launch pushed the rings, 2
 *   when it read the tables (counted when the launch is queued, as fvad_vad_batch_chain_form).  fvad_vad_batch_avgs_bytes: the
 *   bytes of the tables and min_volume rows of that launch's part (0 with the rings).
 * - fvad_vad_batch_avg_keys: the keys in first-seen config order, as pairs -- st_keys[2 j], st_keys[2 j + 1] = band and ring
 *   length of short key j, cr_keys likewise size index and ring length -- and each config's keys st_key[c], cr_key[c] (any of
 *   the four may be NULL to get the counts only; cap: pairs each list has room for, FVAD_ERR_BUFFER_TOO_SMALL below either count).
 *   Recomputed by fvad_vad_batch_retain_configs for the kept configs.  Needs no device.
 * - fvad_vad_batch_averages_device (a test tap): only the two table kernels, on the context's stream, for the frames a part call
 *   with the same d_band, n_frames [n_sizes][n_streams], host chunk_rms, n_chunks, chunk_size and first_sample would run; returns
 *   when done.  st_avg[(j * n_streams + s) * row_stride + k] = short key j's average after frame k of the part of stream s,
 *   cr_avg likewise per ratio key (entries past a stream's frames are left alone).  With first_sample > 0 the earlier frames are
 *   read from b's device part state, which must end at first_sample on this context (FVAD_ERR_INVALID_ARGUMENT otherwise).
 *   Changes nothing in b.
 * - fvad_vad_avg_chain: csrc/vad_avgs.h on the host -- out[k] = the average of a ring of `len` slots after frame first_frame + k,
 *   x[k] that frame's input; with first_frame > 0, ring[i] = slot i as the ring was before frame first_frame (else unused). */
int fvad_vad_batch_avgs_form(const fvad_vad_batch *b, int *form);
size_t fvad_vad_batch_avgs_bytes(const fvad_vad_batch *b);
int fvad_vad_batch_avg_keys(const fvad_vad_batch *b, uint32_t *st_keys, uint32_t *cr_keys, size_t cap, size_t *n_st_keys,
                            size_t *n_cr_keys, uint32_t *st_key, uint32_t *cr_key);
int fvad_vad_batch_averages_device(fvad_ctx *ctx, const fvad_vad_batch *b, const float *d_band, size_t band_stride,
                                   const size_t *n_frames, const float *chunk_rms, size_t rms_stride,
                                   const size_t *n_chunks, size_t chunk_size, uint64_t first_sample, double *st_avg,
                                   double *cr_avg, size_t row_stride);
int fvad_vad_avg_chain(const float *x, size_t n_frames, size_t first_frame, uint32_t len, const float *ring, double *out);

/* Shared triggers (context option vad_trigger: "config", the default, or "shared"; FVAD_VAD_TRIGGER read at context creation).
 * The expensive part of a VAD machine is its trigger: the three rolling averages, the lazily exact long-term chain and the
 * decision.  It does not read min_consecutive_sec_to_open, max_speech_gap_sec or min_vad_duration_sec, and nothing flows back
 * into it from the state machine (VADMachine.zig:166-178 against :186-309).  Configs whose derived trigger quantities are all
 * equal -- size index, band block, the three ring lengths (slot counts), has_init and initial, factor and ratio_threshold, the
 * floating-point members compared as bit patterns -- share a trigger key.
 * - "shared": a device sweep runs one trigger machine per (stream, key) -- the cooperative kernel of csrc/kernels_vad.hip in a
 *   form that emits each frame's threshold_met as one bit, ring or table averages, sized or not -- and then one lane per
 *   (stream, config) of csrc/kernels_vadfinish.hip, which walks those bits through the state machine, the segment statistics and
 *   the closing of segments (csrc/vad_finish.h; while a machine is closed it jumps from set bit to set bit).  Segments, counts,
 *   audits, lazy statistics and device scores have the bits of the per-config machines.  When segment room overflows only the
 *   finishing kernel runs again, over the same bits; the one-shot calls run as one such part.
 * - A run takes the shared form at its first launch when vad_trigger is "shared", vad_chain is "coop" and the part's bits fit in
 *   vad_trigger_max_bytes (context option, default 4 GiB: a guard computed from shapes -- S streams x keys x frames / 8 bytes);
 *   otherwise the per-config machines run.  The form is fixed for the run: a run that began in one form continues in it, and
 *   changing the option takes effect at the next run's first part.  Part state is not converted between the forms.
 * - The bits and the finishing state belong to the batch's device part state: they only grow, are freed with it and count in
 *   fvad_vad_batch_device_bytes.  After a one-shot call, which no part can follow, only the bits are still held (for
 *   fvad_vad_batch_trigger_bits) until the next run or the batch's end, and device_bytes reports them.
 *   fvad_vad_batch_retain_configs in a shared run retains the trigger machines to the surviving
 *   keys and then compacts the per-config state; the keys reported afterwards are first-seen over the survivors.
 * - fvad_vad_batch_trigger_keys: key_of[c] = config c's key (first-seen config order), rep[k] = key k's first config; either may
 *   be NULL (counts only); cap: keys rep has room for, FVAD_ERR_BUFFER_TOO_SMALL below *n_keys.  Needs no device; recomputed by
 *   fvad_vad_batch_retain_configs.
 * - fvad_vad_batch_trigger_form: 0 before a device launch, 1 per-config machines, 2 shared.  fvad_vad_batch_trigger_bytes: the
 *   bits of the last shared part.  fvad_vad_batch_trigger_launches: cumulative launches of the emitting machines and of the
 *   finishing kernel in the shared form (either may be NULL).
 * - fvad_vad_batch_trigger_bits (a test tap): the last shared part's bits, out[(k * n_streams + s) * row_stride + w] = word w of
 *   key k, stream s: bit f % 64 of word f / 64 is frame f of the part; bits and words past a stream's frames are zero.
 * - fvad_vad_finish_bits: the walk of csrc/vad_finish.h on the host, for one config at one frame size over one part's words and
 *   frame ratios (frame k at sample first_sample + k * fft_size; bits past n_frames are not read).  state: 6 words, in/out, all
 *   zero = a fresh machine (state, speech_start, speech_end, ratio_count, ratio_sum | met_cum << 32 as f32 bits, segments closed
 *   so far).  Segments closed in this call go to segs (room seg_cap), *n_segs counts them; FVAD_ERR_BUFFER_TOO_SMALL when they
 *   did not all fit (the state has moved on all the same). */
int fvad_vad_batch_trigger_keys(const fvad_vad_batch *b, uint32_t *key_of, size_t cap, size_t *n_keys, uint32_t *rep);
int fvad_vad_batch_trigger_form(const fvad_vad_batch *b, int *form);
size_t fvad_vad_batch_trigger_bytes(const fvad_vad_batch *b);
int fvad_vad_batch_trigger_launches(const fvad_vad_batch *b, uint64_t *machines, uint64_t *finish);
int fvad_vad_batch_trigger_bits(fvad_ctx *ctx, const fvad_vad_batch *b, uint64_t *out, size_t row_stride);
int fvad_vad_finish_bits(const fvad_vad_config *cfg, size_t sample_rate, size_t fft_size, const uint64_t *words,
                         const float *ratios, size_t n_frames, uint64_t first_sample, uint64_t *state,
                         fvad_speech_segment *segs, size_t seg_cap, size_t *n_segs);

/* RollingAverage.zig:11-56 exposed for parity tests */
typedef struct fvad_rolling_average fvad_rolling_average;
int fvad_ra_create(size_t count, int has_initial, double initial_val, fvad_rolling_average **out);
void fvad_ra_destroy(fvad_rolling_average *ra);
double fvad_ra_push(fvad_rolling_average *ra, float sample);
int fvad_ra_last_avg(const fvad_rolling_average *ra, double *out);

/* ------------------------------------------------------------------ B1: AudioPipeline
 * (src/AudioPipeline.zig) -- what simulator.zig / main.zig hold. */
/* Recording payload == AudioBuffer (src/audio_utils/AudioBuffer.zig:16-24) as Recorder.finalize
 * builds it (Recorder.zig:131-164): ONE channel -- the quietest of the stream's channels over the
 * clip (findBestChannel, :113-129) -- covering samples [global_start_frame_number, + length).
 * Unlike the reference (callee frees, MRBRecorder.zig:9-11) the buffer belongs to the library and
 * is valid only during the callback. */
typedef struct fvad_audio_buffer {
    const float *const *channel_pcm;
    size_t n_channels, length, sample_rate;
    float duration_seconds;
    uint64_t global_start_frame_number;
} fvad_audio_buffer;
/* AudioPipeline.Callbacks (AudioPipeline.zig:14-18).  When callbacks are given, every segment the
 * state machine completes (VADPipeline.zig:215-229) schedules one original-audio clip and one
 * denoised-audio clip (AudioPipeline.zig:187-191); each is delivered as soon as its buffer holds the
 * samples up to the clip's end -- at once, or during a later push -- and a recording that restarts
 * before then replaces it, exactly like MRBRecorder.zig:76-118,160-192 on the reference's write schedule
 * (pushes written in steps of buffer_length / 2, denoised audio in 0.5 s chunks).  The denoised audio is
 * then also copied back from the GPU (1920 B per frame). */
typedef void (*fvad_recording_cb)(void *ctx, const fvad_audio_buffer *recording);
typedef struct {                              /* AudioPipeline.Callbacks, AudioPipeline.zig:14-18 */
    void *ctx;
    fvad_recording_cb on_original_recording;
    fvad_recording_cb on_denoised_recording;
} fvad_callbacks;

typedef struct {
    size_t sample_rate;                       /* AudioPipeline.Config, AudioPipeline.zig:20-26 */
    size_t n_channels;
    size_t buffer_length;                     /* 0 = sample_rate * 10 (:46); otherwise >= one 24000-sample chunk */
    int32_t skip_processing;
    size_t fft_size;                          /* VADPipeline.Config.fft_size = 1024 (:21); any even size from 4 to 16384 */
    fvad_vad_config vad_machine_config;       /* :22 */
    const fvad_vad_config *alt_vad_machine_configs; /* :24 */
    size_t n_alt_vad_machine_configs;
} fvad_pipeline_config;
void fvad_pipeline_config_default(fvad_pipeline_config *c);

typedef struct fvad_pipeline fvad_pipeline;
/* AudioPipeline.init(allocator, config, callbacks)  AudioPipeline.zig:40-102 */
int fvad_pipeline_create(fvad_ctx *ctx, const fvad_pipeline_config *cfg,
                         const fvad_callbacks *callbacks, fvad_pipeline **out);
void fvad_pipeline_destroy(fvad_pipeline *p);                          /* deinit :104-112 */
/* pushSamples(channel_pcm) -> index of the first pushed sample  AudioPipeline.zig:118-143 */
int fvad_pipeline_push_samples(fvad_pipeline *p, const float *const *channel_pcm,
                               size_t n_samples, uint64_t *first_sample_index);
uint64_t fvad_pipeline_total_write_count(const fvad_pipeline *p);      /* :114-116 */
/* pipeline.vad.vad_machine.vad_segments  (SimulationInstance.zig:221) */
size_t fvad_pipeline_segment_count(const fvad_pipeline *p);
int fvad_pipeline_segments(const fvad_pipeline *p, fvad_speech_segment *out, size_t cap,
                           size_t *n);
int fvad_pipeline_alt_segments(const fvad_pipeline *p, size_t alt_index,
                               fvad_speech_segment *out, size_t cap, size_t *n);
int fvad_pipeline_audit(const fvad_pipeline *p, fvad_vad_audit *out);
/* traces for parity tests: per-FFT-frame band sums [n][n_channels] and volume ratios [n], kept for the frames
 * processed while tracing is enabled (off by default: a live pipeline does not grow with the stream) */
int fvad_pipeline_enable_trace(fvad_pipeline *p, int on);
size_t fvad_pipeline_n_fft_frames(const fvad_pipeline *p);
int fvad_pipeline_trace(const fvad_pipeline *p, float *band_volumes, float *vol_ratio,
                        size_t cap_frames);

/* ------------------------------------------------------------------ batch Recorder: speech clips of device-resident lanes
 * What Recorder.finalize hands to AudioPipeline.Callbacks (Recorder.zig:74-164, AudioPipeline.zig:187-191), for the batch
 * paths (fvad_engine_run, fvad_engine_enqueue_device*): given clip ranges over lanes that are already on the device, every
 * channel's RMS over every clip, the quietest channel as Recorder.findBestChannel picks it (Recorder.zig:113-129), and that
 * channel's samples packed into one buffer -- so that only the clips cross PCIe, not the corpus (csrc/kernels_clips.hip).
 * - A clip is a row of FVAD_CLIP_FIELDS uint64: first_lane, n_channels, sample_from, sample_to.  Its channels are lanes
 *   first_lane .. first_lane + n_channels - 1, its samples [sample_from, sample_to).  Clips may overlap and repeat.
 * - Sample formats: FVAD_CLIP_F32 or FVAD_CLIP_PCM16, for the source lanes and for the packed output independently.  Equal
 *   formats copy bits; PCM16 -> f32 is s / 32768; f32 -> PCM16 is rint(clamp(y * 32768, -32768, 32767)), as for
 *   fvad_lane.denoised_i16.
 * - Per clip the calls report (each array has n_clips entries, host memory, any may be NULL): best_channel, relative to
 *   first_lane; best_rms, that channel's (float)sqrt(sum of squares / n), the sum in f64; runner_up_rms, the smallest RMS among
 *   the other channels (best_rms for a mono clip) -- how close the pick was, in the spirit of fvad_vad_audit; out_offsets, the
 *   clip's slot in the output in samples.  The pick is strict `<` in channel order: the lowest index wins a tie.  The reference
 *   sums the squares sequentially in f32 (audio_utils.zig:14-24); channels whose RMS differ by less than that sum's round-off
 *   can be picked differently, and runner_up_rms shows which clips those are.
 * - INVARIANT: a clip's info and samples are the same bits whatever else is in the call and in whatever order, run after run
 *   (no atomics; each clip's sums have a fixed order).  A caller short of memory can export in batches.
 * - Deviation from the live pipeline: the batch form gives a clip to every segment whose end the data reaches.  It does not
 *   replay MRBRecorder's drop of a pending clip when a recording restarts before the ring has delivered it
 *   (MRBRecorder.zig:76-118), an artefact of the 10 s ring on the write schedule that fvad_pipeline_* keeps.  With
 *   max_speech_gap_sec >= 2 (the default) the two agree except at a stream's end.
 *
 * fvad_clips_plan (host only): offsets[i] = clip i's slot and *total = the output's size, in samples of out_format; every slot
 * starts on a 16-byte boundary.  FVAD_ERR_INVALID_ARGUMENT for sample_to <= sample_from, n_channels == 0, a bad format or NULLs.
 * fvad_clips_from_segments (host only): one clip (first_lane, n_channels, the segment's range) per segment whose sample_to <=
 * n_available, in order; the others are counted in *n_skipped -- the reference never finalises a recording whose end the stream
 * does not reach.  n_available is the lane's n_samples for the original audio and n_chunks * 24000 for the denoised audio.
 * *n_out = the clips the segments give; FVAD_ERR_BUFFER_TOO_SMALL when cap is below it (the first cap are written; clips may be
 * NULL with cap 0 to count).  FVAD_ERR_INVALID_ARGUMENT for n_channels == 0, NULL counts or a segment with sample_to <= sample_from.
 * fvad_clips_export_device: d_src holds n_lanes lanes of n_samples (lane l at d_src + l * lane_stride samples), as
 * fvad_engine_enqueue_device* lays them out; d_out (device, 16-byte aligned) has room for out_capacity samples.  Every error
 * comes back before any launch: FVAD_ERR_OUT_OF_RANGE for sample_to > n_samples or lanes past n_lanes,
 * FVAD_ERR_BUFFER_TOO_SMALL when out_capacity is below the plan's total, FVAD_ERR_INVALID_ARGUMENT for NULLs, bad formats, a
 * misaligned d_out and what fvad_clips_plan refuses.  n_clips == 0 does nothing and succeeds.  The kernels read nothing outside
 * the clips' ranges and write nothing outside the clips' samples (the padding between slots is left alone).  Returns when the
 * clips are in d_out.  fvad_ctx_kernel_times names clip_rms, clip_pick, clip_gather.  Original and denoised audio are two
 * calls: the reference has two independent recorders, each picking from its own audio.
 * fvad_clips_export: the same into host memory `out` -- a device staging buffer of the plan's size, one copy back, then freed;
 * the padding between slots comes back as zeros. */
enum { FVAD_CLIP_F32 = 0, FVAD_CLIP_PCM16 = 1 };
#define FVAD_CLIP_FIELDS 4
int fvad_clips_plan(const uint64_t *clips, size_t n_clips, int out_format, uint64_t *offsets, uint64_t *total);
int fvad_clips_from_segments(const fvad_speech_segment *segs, size_t n_segs, uint32_t first_lane, uint32_t n_channels,
                             uint64_t n_available, uint64_t *clips, size_t cap, size_t *n_out, size_t *n_skipped);
int fvad_clips_export_device(fvad_ctx *ctx, const void *d_src, int src_format, size_t n_lanes, size_t lane_stride,
                             size_t n_samples, const uint64_t *clips, size_t n_clips, int out_format, void *d_out,
                             size_t out_capacity, int32_t *best_channel, float *best_rms, float *runner_up_rms,
                             uint64_t *out_offsets);
int fvad_clips_export(fvad_ctx *ctx, const void *d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                      const uint64_t *clips, size_t n_clips, int out_format, void *out, size_t out_capacity,
                      int32_t *best_channel, float *best_rms, float *runner_up_rms, uint64_t *out_offsets);

/* ------------------------------------------------------------------ batch Recorder over a split source
 * For runs sliced in time: a clip may begin in audio of earlier slices and end in the current one, so its samples are a head
 * piece in one device buffer (A: the held tail of earlier slices) followed by a body piece in another (B: the current slice's
 * lanes) -- the SplitSlice MRBRecorder reads a recording from its ring as (MRBRecorder.zig:160-192), and what fvad_fft_forward
 * takes as (first, n1, second, n2).  The kernels read the two pieces as one run (csrc/clip_source_device.h).
 * - A split clip is a row of FVAD_CLIP_SPLIT_FIELDS uint64: n_channels, a_lane, a_from, a_len, b_lane, b_from, b_len.  Its
 *   channel c is A[a_lane + c][a_from, a_from + a_len) followed by B[b_lane + c][b_from, b_from + b_len).  Either length may be
 *   0, not both; a piece of no samples has no other rule.  d_a (d_b) may be NULL when no row takes samples from it.
 * - A and B have one sample format, src_format; each has its own lane count, stride and sample count.
 * - Slots, formats, conversions and the per-clip reports are fvad_clips_export's: the slots are those fvad_clips_plan gives
 *   clips of lengths a_len + b_len in the same order.
 * - INVARIANT: a split clip's samples, best_channel, best_rms and runner_up_rms are the bits fvad_clips_export_device gives
 *   for the same samples laid out contiguously, wherever the seam is (tiles and sums are counted from the clip's first sample).
 *   Equal formats move the bits (NaN payloads, -0, denormals), so a mono clip per lane with equal formats carries a tail from
 *   one held buffer to the other; out_offsets are then the lanes' new bases.
 *
 * fvad_clips_split_check (host only; pointers are addresses, nothing is read through d_a, d_b or out): every argument rule of
 * the two exports, in the one order both report them in -- FVAD_ERR_INVALID_ARGUMENT for NULL clips / out, a bad format or a
 * NULL source that a row takes samples from; for a source not aligned to its samples or (device_out) an out not 16-byte
 * aligned; for a stride below its sample count (of a buffer of more than one lane); for a row with both lengths 0 or no
 * channels; FVAD_ERR_OUT_OF_RANGE for a piece past its buffer's samples or lanes; FVAD_ERR_BUFFER_TOO_SMALL when out_capacity
 * is below the total; FVAD_ERR_INVALID_ARGUMENT when the total's bytes at `out` overlap A's or B's address range, and for more
 * than 2^31 - 1 (clip, channel, tile) units of 8192 samples.  Fills offsets (may be NULL) and *total (may be NULL; 0 until the
 * rows' own rules have passed).  n_clips == 0 succeeds.
 * fvad_clips_export_split_device / fvad_clips_export_split: as fvad_clips_export_device / fvad_clips_export; every error comes
 * back before any launch.  fvad_ctx_kernel_times names clip_rms_split, clip_pick, clip_gather_split. */
#define FVAD_CLIP_SPLIT_FIELDS 7
int fvad_clips_split_check(const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void *d_b, size_t b_lanes,
                           size_t b_stride, size_t b_samples, int src_format, const uint64_t *clips, size_t n_clips,
                           int out_format, const void *out, size_t out_capacity, int device_out, uint64_t *offsets,
                           uint64_t *total);
int fvad_clips_export_split_device(fvad_ctx *ctx, const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                   const void *d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                   const uint64_t *clips, size_t n_clips, int out_format, void *d_out, size_t out_capacity,
                                   int32_t *best_channel, float *best_rms, float *runner_up_rms, uint64_t *out_offsets);
int fvad_clips_export_split(fvad_ctx *ctx, const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void *d_b,
                            size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t *clips,
                            size_t n_clips, int out_format, void *out, size_t out_capacity, int32_t *best_channel,
                            float *best_rms, float *runner_up_rms, uint64_t *out_offsets);
/* fvad_vad_batch_hold_from (host only): per stream, the smallest sample_from that a segment not yet reported by machine
 * (stream, config) can still get -- what a caller that slices a run in time must keep of the audio behind it.  A closed machine:
 * next - min(start_buffer, next), next the first sample of the next frame to run; an opening, open or closing one: its pending
 * segment's sample_from.  A batch that has run nothing: 0.  Defined after host runs (fvad_vad_batch_run, _run_part,
 * _run_sized); after a device run the machines' state is not on the host: FVAD_ERR_INVALID_ARGUMENT. */
int fvad_vad_batch_hold_from(const fvad_vad_batch *b, size_t config, uint64_t *hold_from);

/* ------------------------------------------------------------------ batch Recorder with a stride: clips at the denoiser's rate
 * NSNet2 works at 16 kHz; its output comes back to 48 kHz as [lerp, lerp, sample] per 16 kHz sample (resample.zig:32-79), so in
 * a denoised lane the samples at index = 2 (mod 3) are the network's own output, bit for bit, and the others a fused lerp of
 * their neighbours.  A recogniser takes 16 kHz: these calls export every step-th sample of a clip and nothing else crosses PCIe
 * (csrc/kernels_clips_strided.hip).
 * - Per clip a skip < step: the output is samples skip, skip + step, skip + 2 step, ... of the clip's picked channel,
 *   out_len = ceil((len - skip) / step) of them, converted by fvad_clips_export's rules (equal formats move the bits).
 * - The channel is picked exactly as fvad_clips_export picks it, over EVERY sample of the clip.
 * - INVARIANT: for the same clip best_channel, best_rms and runner_up_rms are the bits the full-rate export gives, and the
 *   samples are that export's samples[skip::step] -- for the split form wherever the seam is (the stride runs through it).
 * - Slots: 16-byte aligned, in clip order, sized by out_len (fvad_clips_plan_strided).  step == 1 (every skip 0) gives the
 *   full-rate exports' bits and offsets.
 * - Step 3 with the skips of phase 2 is lossless with respect to the denoiser.  With phase 0 on the original audio it is the
 *   reference's downsampleAudio (resample.zig:9-29: lane index = 0 mod 3, NO anti-alias filter) -- sample for sample what
 *   NSNet2 was fed, aliasing included.  The filtered decimator is fvad_clips_export_fir* (the next block).
 *
 * fvad_clips_phase_skips (host only): skips[i] = (phase + step - sample_from[i] mod step) mod step, so that the kept samples
 * are the lane indices = phase (mod step).  FVAD_ERR_INVALID_ARGUMENT for step == 0, step > FVAD_CLIP_STEP_MAX, phase >= step
 * or NULLs with n_clips > 0.
 * fvad_clips_plan_strided (host only): out_lens[i], offsets[i] and *total for clips of lens[i] samples, in samples of
 * out_format; skips NULL means all zero.  FVAD_ERR_INVALID_ARGUMENT for step == 0, step > FVAD_CLIP_STEP_MAX, a skip >= step,
 * a clip with len <= skip (no sample kept), a bad format, NULLs, or a total that does not fit 64 bits.
 * fvad_clips_export_strided_device / fvad_clips_export_strided / fvad_clips_export_split_strided_device /
 * fvad_clips_export_split_strided: the full-rate call's arguments, then step and skips (host memory, n_clips entries, or NULL:
 * all zero).  Every error comes back before any launch, in the full-rate call's order with the rules above (step, then per clip
 * its skip) directly after the rows' own rules; out_capacity is checked against the strided total and out_offsets are the
 * strided slots.  fvad_ctx_kernel_times names clip_rms, clip_pick, clip_gather_strided (split: clip_rms_split, clip_pick,
 * clip_gather_strided_split); with step == 1 the gather is the full-rate one under its own name.
 * Deviation from a plain "argument list plus two": none in the lists; fvad_clips_phase_skips also refuses phase >= step. */
#define FVAD_CLIP_STEP_MAX 16
int fvad_clips_phase_skips(const uint64_t *sample_from, size_t n_clips, uint32_t step, uint32_t phase, uint32_t *skips);
int fvad_clips_plan_strided(const uint64_t *lens, const uint32_t *skips, size_t n_clips, uint32_t step, int out_format,
                            uint64_t *out_lens, uint64_t *offsets, uint64_t *total);
int fvad_clips_export_strided_device(fvad_ctx *ctx, const void *d_src, int src_format, size_t n_lanes, size_t lane_stride,
                                     size_t n_samples, const uint64_t *clips, size_t n_clips, int out_format, void *d_out,
                                     size_t out_capacity, int32_t *best_channel, float *best_rms, float *runner_up_rms,
                                     uint64_t *out_offsets, uint32_t step, const uint32_t *skips);
int fvad_clips_export_strided(fvad_ctx *ctx, const void *d_src, int src_format, size_t n_lanes, size_t lane_stride,
                              size_t n_samples, const uint64_t *clips, size_t n_clips, int out_format, void *out,
                              size_t out_capacity, int32_t *best_channel, float *best_rms, float *runner_up_rms,
                              uint64_t *out_offsets, uint32_t step, const uint32_t *skips);
int fvad_clips_export_split_strided_device(fvad_ctx *ctx, const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                           const void *d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                           const uint64_t *clips, size_t n_clips, int out_format, void *d_out,
                                           size_t out_capacity, int32_t *best_channel, float *best_rms, float *runner_up_rms,
                                           uint64_t *out_offsets, uint32_t step, const uint32_t *skips);
int fvad_clips_export_split_strided(fvad_ctx *ctx, const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                    const void *d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                    const uint64_t *clips, size_t n_clips, int out_format, void *out, size_t out_capacity,
                                    int32_t *best_channel, float *best_rms, float *runner_up_rms, uint64_t *out_offsets,
                                    uint32_t step, const uint32_t *skips);

/* ------------------------------------------------------------------ batch Recorder with a filter: anti-aliased clips
 * The strided export keeps every step-th sample and nothing else, so whatever the lane holds above the new Nyquist frequency
 * folds into the exported band (a 10 kHz tone in a 48 kHz lane leaves a step-3 export as a 6 kHz tone at full level).  A
 * filtered export is a strided export plus `const float *taps, uint32_t n_taps` in host memory: a FIR filter applied while the
 * clip is decimated (csrc/kernels_clips_fir.hip), so that only the kept, band-limited samples leave the device.
 * - n_taps is odd, 1 <= n_taps <= FVAD_CLIP_FIR_TAPS_MAX; H = (n_taps - 1) / 2; the taps need not be symmetric.
 * - Clip, pick, step, skip, out_len = ceil((len - skip) / step), slots and out_offsets are exactly the strided export's
 *   (fvad_clips_plan_strided plans it).  step == 1 is a plain FIR without decimation, n_taps == 1 a scaled strided export.
 * - Output q of a clip is centred on clip sample c = skip + q * step of the picked channel:
 *       y[q] = sum over k = 0 .. n_taps - 1 of taps[k] * x[c + k - H]
 *   x[i] is the clip's sample i as f32 (PCM16: s / 32768, exact) and 0 for i < 0 or i >= len; the sum is accumulated in f32 and
 *   converted by fvad_clips_export's rule for an f32 source (f32: as it is; PCM16: rint(clamp(y * 32768, -32768, 32767))).
 * - The clip is filtered as a finite signal, zero-extended: nothing outside [sample_from, sample_to) is read.  So a filtered
 *   clip is what decimating the full-rate exported clip on the host with the same taps gives, and a sliced run needs no more
 *   held audio than fvad_vad_batch_hold_from keeps.
 * - RMS and pick run over every sample of the UNFILTERED clip: best_channel, best_rms and runner_up_rms are the full-rate
 *   export's bits.
 * - INVARIANTS.  An output's bits do not depend on the call form (contiguous or split, device or host output), on where the
 *   seam of a split clip is, on which tile of the gather the output falls in, or on the other clips of the call.  The PCM16
 *   output is the f32 output of the same call converted by the rule above, bit for bit.  A PCM16 source gives the bits of an
 *   f32 source that holds s / 32768.  (Every output is one f32 fma chain from +0 in an order that depends on step and n_taps
 *   alone; the order itself is not part of the contract.)
 *
 * fvad_clips_fir_design (host only): taps[0 .. 2 half] of a Kaiser-windowed sinc, computed in float64:
 *   h[k] = 2 cutoff sinc(2 cutoff (k - half)) * kaiser(2 half + 1, beta)[k], normalised to unit sum, then rounded to f32;
 *   cutoff in cycles per input sample, I0 by its power series.  half == 0 selects half = 16 step, cutoff == 0 selects
 *   cutoff = 0.45 / step, beta == 0 selects beta = 6.  FVAD_ERR_INVALID_ARGUMENT for a step outside 1..FVAD_CLIP_STEP_MAX,
 *   half > 256, a cutoff not in (0, 0.5] (0 apart), a negative or non-finite beta, or NULL.
 * fvad_clips_fir_check (host only): the tap rules without a device -- FVAD_ERR_INVALID_ARGUMENT for NULL taps, n_taps of 0,
 *   an even n_taps, n_taps above FVAD_CLIP_FIR_TAPS_MAX or a non-finite tap.
 * fvad_clips_export_fir_device / fvad_clips_export_fir / fvad_clips_export_split_fir_device / fvad_clips_export_split_fir:
 *   the matching strided call's arguments, then taps and n_taps.  Every error comes back before any launch; the tap rules are
 *   reported directly after the strided rules for step and skips, before ranges and lanes.  fvad_ctx_kernel_times names
 *   clip_rms, clip_pick, clip_gather_fir (split: clip_rms_split, clip_pick, clip_gather_fir_split), at every step. */
#define FVAD_CLIP_FIR_TAPS_MAX 513
int fvad_clips_fir_design(uint32_t step, uint32_t half, double cutoff, double beta, float *taps);
int fvad_clips_fir_check(const float *taps, uint32_t n_taps);
int fvad_clips_export_fir_device(fvad_ctx *ctx, const void *d_src, int src_format, size_t n_lanes, size_t lane_stride,
                                 size_t n_samples, const uint64_t *clips, size_t n_clips, int out_format, void *d_out,
                                 size_t out_capacity, int32_t *best_channel, float *best_rms, float *runner_up_rms,
                                 uint64_t *out_offsets, uint32_t step, const uint32_t *skips, const float *taps,
                                 uint32_t n_taps);
int fvad_clips_export_fir(fvad_ctx *ctx, const void *d_src, int src_format, size_t n_lanes, size_t lane_stride,
                          size_t n_samples, const uint64_t *clips, size_t n_clips, int out_format, void *out,
                          size_t out_capacity, int32_t *best_channel, float *best_rms, float *runner_up_rms,
                          uint64_t *out_offsets, uint32_t step, const uint32_t *skips, const float *taps, uint32_t n_taps);
int fvad_clips_export_split_fir_device(fvad_ctx *ctx, const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                       const void *d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                       const uint64_t *clips, size_t n_clips, int out_format, void *d_out,
                                       size_t out_capacity, int32_t *best_channel, float *best_rms, float *runner_up_rms,
                                       uint64_t *out_offsets, uint32_t step, const uint32_t *skips, const float *taps,
                                       uint32_t n_taps);
int fvad_clips_export_split_fir(fvad_ctx *ctx, const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                const void *d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                const uint64_t *clips, size_t n_clips, int out_format, void *out, size_t out_capacity,
                                int32_t *best_channel, float *best_rms, float *runner_up_rms, uint64_t *out_offsets,
                                uint32_t step, const uint32_t *skips, const float *taps, uint32_t n_taps);

/* ------------------------------------------------------------------ batch Recorder with a resampler: clips at any rate
 * The strided and filtered exports leave at whole fractions of the lanes' 48 kHz.  A resampled export is a full-rate export
 * plus `uint32_t up, uint32_t down, const float *taps, uint32_t n_taps` (taps in host memory): a rational up/down polyphase
 * resampler applied while the clip is gathered (csrc/kernels_clips_resample.hip), the resampling ingest's arithmetic (below) on
 * the way out.
 * THE DEFINITION
 * - up/down = rate_out/48000 in lowest terms, as fvad_resample_ratio(48000, rate_out, ...) gives it: 44100 is 147/160, 32000
 *   2/3, 22050 147/320, 11025 147/640, 16000 1/3, 96000 2/1.  1 <= up <= FVAD_RESAMPLE_UP_MAX, down >= 1.
 * - n_taps is odd and <= FVAD_RESAMPLE_TAPS_MAX, the centre K = (n_taps - 1) / 2; the taps need not be symmetric.  One ratio and
 *   one set of taps per call.
 * - Clip, pick and the per-clip reports are exactly the full-rate export's: RMS and pick run over every sample of the
 *   UNRESAMPLED clip, and best_channel, best_rms and runner_up_rms are the full-rate export's bits.
 * - For a clip of len samples of its picked channel, x[0 .. len) is the clip as f32 (PCM16: s / 32768, exact) and x is 0 outside
 *   [0, len).  out_len = ceil(len * up / down) = fvad_resample_out_frames(len, up, down), and
 *       y[o] = sum over n of x[n] * taps[K + o * down - n * up],   over every n whose tap index lies in [0, 2 K],
 *   accumulated in f32 and converted by fvad_clips_export's rule for an f32 source (f32: as it is; PCM16:
 *   rint(clamp(y * 32768, -32768, 32767))).  Output o sits o / rate_out seconds after the clip's first sample: the phase is
 *   counted from the CLIP's start, never from the lane index or the seam of a split clip.
 * - The clip is filtered as a finite signal: nothing outside [sample_from, sample_to) is read.  So a file is what resampling
 *   the exported 48 kHz clip on the host with the same taps gives, and a sliced run holds no more audio than
 *   fvad_vad_batch_hold_from keeps.
 * - Index arithmetic is 64-bit (o * down passes 2^32 in a 29 M-sample clip at down = 640); len * up must stay below 2^62.
 * - Slots are 16-byte aligned, in clip order, sized by out_len (fvad_clips_plan_resampled plans them).
 * - INVARIANTS, all bit for bit.  An output's bits do not depend on the call form (contiguous or split, device or host output),
 *   on where the seam of a split clip lies, on which tile of the gather the output falls in, or on the other clips of the call
 *   and their order.  The PCM16 output is the f32 output of the same call converted by the rule above.  A PCM16 source gives the
 *   bits of an f32 source that holds s / 32768.  (Every output is one f32 fma chain from +0 in an order that depends on up,
 *   down, n_taps and o mod up alone; the order itself is not part of the contract, and bit equality with the filtered export
 *   at up == 1 is not promised.  up == down == 1 with the single tap 1.0 gives the full-rate export's bits, a -0.0 sample
 *   apart, which leaves as +0.0.)
 * - The default taps are fvad_resample_design(up, down, 0, 0, 0, ...): with m = max(up, down), K = 16 m, cutoff 0.45 / m,
 *   beta 6, sum up; 5121 taps at 147/160 and FVAD_RESAMPLE_TAPS_MAX at 147/640.  Computed from these taps in float64
 *   (tools/resample_response.py; the prototype's shape depends on m alone, so ripple and stop band are the ingest's at the
 *   mirrored ratio; the phases are others):
 *     ratio 147/160 (44100): pass-band ripple up to 0.40/m 0.11 dB, stop band from 0.60/m -69.9 dB,  35 taps a phase, the phases'
 *                            DC gains within 3.4e-4 of each other
 *     ratio 147/320 (22050): 0.11 dB, -69.8 dB,  70 taps a phase, 1.4e-4
 *     ratio 147/640 (11025): 0.11 dB, -69.8 dB, 140 taps a phase, 6.5e-5
 *     ratio 2/3 (32000):     0.11 dB, -72.1 dB,  49 taps a phase, 1.7e-4
 *     ratio 1/3 (16000):     0.11 dB, -72.1 dB,  97 taps, one phase
 *
 * Host only (csrc/host_clips_resample.cpp):
 * fvad_clips_resample_check: FVAD_ERR_INVALID_ARGUMENT for a ratio that is none (up == 0, up > FVAD_RESAMPLE_UP_MAX,
 *   down == 0); then for taps that fail fvad_ingest_resample_check's tap rules (NULL, a zero or even count, more than
 *   FVAD_RESAMPLE_TAPS_MAX, a non-finite tap); then for a tile of 0.
 * fvad_clips_resample_tile: the gather's outputs per tile, the most (a multiple of 8, at most 8192) whose window
 *   floor(((n - 1) down + 2 K) / up) + 1 fits the 8192 clip samples a tile stages; 0 when not even 8 outputs' window fits (such
 *   a call is refused), for a ratio that is none or a tap count that is none.
 * fvad_clips_plan_resampled: out_lens[i] = ceil(lens[i] * up / down), the slots' offsets and their total in samples of
 *   out_format, as fvad_clips_plan_strided plans its own.  FVAD_ERR_INVALID_ARGUMENT for a ratio that is none, a clip of length
 *   0, a bad format, NULL, or a total (an out_len that saturates at UINT64_MAX included) that does not fit 64 bits.
 * fvad_clips_export_resampled_device / fvad_clips_export_resampled / fvad_clips_export_split_resampled_device /
 * fvad_clips_export_split_resampled: the matching full-rate call's arguments, then up, down, taps and n_taps.  Every error
 *   comes back before any launch, in the full-rate call's order; fvad_clips_resample_check's rules, then a clip with
 *   len * up >= 2^62 or a total past 64 bits, are reported directly after the rows' own rules, before ranges and lanes.
 *   out_capacity is checked against the resampled total and out_offsets are the resampled slots; more than 2^31 - 1 (clip, tile)
 *   units in one call is FVAD_ERR_INVALID_ARGUMENT.  fvad_ctx_kernel_times names clip_rms, clip_pick, clip_gather_resampled
 *   (split: clip_rms_split, clip_pick, clip_gather_resampled_split). */
int fvad_clips_resample_check(uint32_t up, uint32_t down, const float *taps, uint32_t n_taps);
uint64_t fvad_clips_resample_tile(uint32_t up, uint32_t down, uint32_t n_taps);
int fvad_clips_plan_resampled(const uint64_t *lens, size_t n_clips, uint32_t up, uint32_t down, int out_format,
                              uint64_t *out_lens, uint64_t *offsets, uint64_t *total);
int fvad_clips_export_resampled_device(fvad_ctx *ctx, const void *d_src, int src_format, size_t n_lanes, size_t lane_stride,
                                       size_t n_samples, const uint64_t *clips, size_t n_clips, int out_format, void *d_out,
                                       size_t out_capacity, int32_t *best_channel, float *best_rms, float *runner_up_rms,
                                       uint64_t *out_offsets, uint32_t up, uint32_t down, const float *taps, uint32_t n_taps);
int fvad_clips_export_resampled(fvad_ctx *ctx, const void *d_src, int src_format, size_t n_lanes, size_t lane_stride,
                                size_t n_samples, const uint64_t *clips, size_t n_clips, int out_format, void *out,
                                size_t out_capacity, int32_t *best_channel, float *best_rms, float *runner_up_rms,
                                uint64_t *out_offsets, uint32_t up, uint32_t down, const float *taps, uint32_t n_taps);
int fvad_clips_export_split_resampled_device(fvad_ctx *ctx, const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                             const void *d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                             const uint64_t *clips, size_t n_clips, int out_format, void *d_out,
                                             size_t out_capacity, int32_t *best_channel, float *best_rms, float *runner_up_rms,
                                             uint64_t *out_offsets, uint32_t up, uint32_t down, const float *taps,
                                             uint32_t n_taps);
int fvad_clips_export_split_resampled(fvad_ctx *ctx, const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                      const void *d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                      const uint64_t *clips, size_t n_clips, int out_format, void *out, size_t out_capacity,
                                      int32_t *best_channel, float *best_rms, float *runner_up_rms, uint64_t *out_offsets,
                                      uint32_t up, uint32_t down, const float *taps, uint32_t n_taps);

/* ------------------------------------------------------------------ batch Recorder with a front end: log-mel features of clips
 * A recogniser does not take 16 kHz audio, it takes a log-mel spectrogram of it (Whisper: 400-point periodic-Hann STFT, hop 160,
 * frames centred with reflection, power spectrum, 80 Slaney mel bands, log10(max(., 1e-10))).  These calls compute it from the
 * device-resident lanes; per clip only [T][n_mels] floats cross PCIe (csrc/kernels_clips_mel.hip).  For a clip row:
 * - Channel: picked exactly as fvad_clips_export picks it, over EVERY sample of the clip; best_channel, best_rms and
 *   runner_up_rms are that call's bits.
 * - Feature stream: s[i] = f32(clip sample skip + i * step) of the picked channel, i < L = ceil((len - skip) / step); step in
 *   1..FVAD_CLIP_STEP_MAX and skip < step as in fvad_clips_plan_strided, skips as fvad_clips_phase_skips gives them (step 3 with
 *   phase 2 on the denoised lanes: NSNet2's own 16 kHz samples).  PCM16 lanes give s / 32768.
 * - Frames: n_fft even in 4..FVAD_CLIP_MEL_NFFT_MAX, hop in 1..n_fft, pad = n_fft / 2, T = floor(L / hop) frames -- torch.stft
 *   with center = True and its last frame dropped, Whisper's convention.  Frame t, tap i reads s[rho(t * hop + i - pad)] with
 *   rho(j) = -j for j < 0 and 2 (L - 1) - j for j >= L (reflection that does not repeat the edge).  A clip with L < pad + 1 or
 *   T == 0 is refused.  Nothing outside the clip's samples is read, and no sample off the stride.
 * - Spectrum: X = rfft(frame * window), window[n_fft] f32 from the caller; P[k] = re^2 + im^2 in f32, k = 0 .. n_fft / 2;
 *   mel[m] = sum_k M[m][k] * P[k] with M[n_mels][n_fft / 2 + 1] f32 row-major from the caller, n_mels in
 *   1..FVAD_CLIP_MEL_BANDS_MAX, one rounded product and one rounded sum per k in ascending k, no atomics;
 *   feat = log10f(fmaxf(mel, floor)), floor a finite positive f32.  log10f(floor) itself is evaluated once per call on the host
 *   (log10 in double, rounded to f32) and is what every mel <= floor gives: digital silence is exactly that value in every band.
 * - Output: per clip [T][n_mels] f32, frame-major, in slots that are 16-byte aligned and in clip order (fvad_clips_plan_mel);
 *   out_format must be FVAD_CLIP_F32, out_capacity and the offsets count floats.  The device form never writes the padding
 *   between slots; the host form zeroes it, as fvad_clips_export does.
 * - Per-clip reports: the four of fvad_clips_export, n_frames (T) and feat_max, the clip's largest feature before any
 *   normalisation (a maximum has no rounding: a fixed tree per tile, then the tiles in order).
 * - Normalisation, norm = (range, offset, scale), three finite f32, or NULL for none:
 *   feat' = (fmaxf(feat, feat_max - range) + offset) * scale -- one rounded subtraction, one rounded sum, one rounded product,
 *   never contracted (numpy float32 is the exact model).  (8, 4, 0.25) is Whisper's.  DEVIATION: the maximum is taken per CLIP;
 *   Whisper takes it over its 30 s window, so a clip cut from a longer window can come out with another clamp.
 * - INVARIANTS, bit for bit: a frame's features depend on that frame's samples and the call's parameters alone -- not on the
 *   other clips, their order, the tile or wavefront slot the frame lands in, the alignment of either side or the call form --
 *   and are the same run after run.  Which transform runs depends on n_fft and the context option clip_mel_fft alone ("auto":
 *   n_fft == 400 on the eight-frames-per-wavefront transform, every other size on the generic mixed-radix one; "generic": every
 *   size on the generic one; environment twin FVAD_CLIP_MEL_FFT), never on the size of the call.  The two transforms agree to
 *   rounding, not bit for bit.
 *
 * fvad_mel_design (host only): matrix[n_mels][n_fft / 2 + 1] of Slaney's filter bank, evaluated in double and rounded once.
 *   mel(f) = 3 f / 200 below 1 kHz and 15 + ln(f / 1000) / (ln 6.4 / 27) above; n_mels + 2 points equally spaced in mel from
 *   fmin to fmax give the edges f_0 .. f_{n_mels + 1}; filter m is the triangle over the bin frequencies k * sample_rate / n_fft
 *   that rises from f_m to f_{m+1} and falls to f_{m+2}, times 2 / (f_{m+2} - f_m).  FVAD_ERR_INVALID_ARGUMENT for fmin < 0,
 *   fmax > sample_rate / 2, fmin >= fmax, a sample rate that is not positive and finite, NULL, or n_fft / n_mels outside the
 *   exports' ranges.  This is librosa.filters.mel's formula (htk = False, norm = "slaney"); librosa was not at hand, so the
 *   designer is checked against the formula written out independently, not against librosa's output.
 * fvad_clips_plan_mel (host only): n_frames[i], offsets[i] and *total (floats) for clips of lens[i] samples; skips NULL means all
 *   zero.  FVAD_ERR_INVALID_ARGUMENT for a bad step, n_fft, hop or n_mels, a skip >= step, a clip with len <= skip, L < pad + 1
 *   or no frame, NULLs, or a total that does not fit 64 bits.
 * fvad_clips_mel_check (host only; d_src and out are addresses, nothing is read through them): every argument rule of the two
 *   exports in the one order both report them in -- NULLs, formats, alignment (device_out: out 16-byte aligned), lane_stride,
 *   the rows' own rules, then step, n_fft, hop, n_mels, per clip its skip and frames (fvad_clips_plan_mel's rules), a window,
 *   matrix, floor or norm value that is not finite (floor also: not positive), then FVAD_ERR_OUT_OF_RANGE for a clip past
 *   n_samples or n_lanes, FVAD_ERR_BUFFER_TOO_SMALL for out_capacity below the total, and more than 2^31 - 1 units or tiles of
 *   frames in one call.  Fills n_frames, offsets and *total (each may be NULL) as far as the rules held.
 * fvad_clips_export_mel_device / fvad_clips_export_mel: the full-rate call's arguments, then step, skips, n_fft, hop, window,
 *   n_mels, matrix, floor, norm (window, matrix, norm: host memory) and the two new reports (each may be NULL).  Every error
 *   comes back before any launch.  fvad_ctx_kernel_times names clip_rms, clip_pick, clip_mel400 or clip_mel, clip_mel_max and,
 *   with norm, clip_mel_norm.  The split-source form (sliced runs) is fvad_clips_export_split_mel* below. */
#define FVAD_CLIP_MEL_NFFT_MAX 2048
#define FVAD_CLIP_MEL_BANDS_MAX 128
int fvad_mel_design(double sample_rate, uint32_t n_fft, uint32_t n_mels, double fmin, double fmax, float *matrix);
int fvad_clips_plan_mel(const uint64_t *lens, const uint32_t *skips, size_t n_clips, uint32_t step, uint32_t n_fft, uint32_t hop,
                        uint32_t n_mels, uint64_t *n_frames, uint64_t *offsets, uint64_t *total);
int fvad_clips_mel_check(const void *d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                         const uint64_t *clips, size_t n_clips, int out_format, const void *out, size_t out_capacity,
                         int device_out, uint32_t step, const uint32_t *skips, uint32_t n_fft, uint32_t hop, const float *window,
                         uint32_t n_mels, const float *matrix, float floor, const float *norm, uint64_t *n_frames,
                         uint64_t *offsets, uint64_t *total);
int fvad_clips_export_mel_device(fvad_ctx *ctx, const void *d_src, int src_format, size_t n_lanes, size_t lane_stride,
                                 size_t n_samples, const uint64_t *clips, size_t n_clips, int out_format, void *d_out,
                                 size_t out_capacity, int32_t *best_channel, float *best_rms, float *runner_up_rms,
                                 uint64_t *out_offsets, uint32_t step, const uint32_t *skips, uint32_t n_fft, uint32_t hop,
                                 const float *window, uint32_t n_mels, const float *matrix, float floor, const float *norm,
                                 uint64_t *n_frames, float *feat_max);
int fvad_clips_export_mel(fvad_ctx *ctx, const void *d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                          const uint64_t *clips, size_t n_clips, int out_format, void *out, size_t out_capacity,
                          int32_t *best_channel, float *best_rms, float *runner_up_rms, uint64_t *out_offsets, uint32_t step,
                          const uint32_t *skips, uint32_t n_fft, uint32_t hop, const float *window, uint32_t n_mels,
                          const float *matrix, float floor, const float *norm, uint64_t *n_frames, float *feat_max);

/* ------------------------------------------------------------------ batch Recorder with a front end: Kaldi-style filter-bank features
 * The other input open recognisers take (k2 / icefall, WeNet, ESPnet, SpeechBrain, FunASR) is Kaldi's fbank, as
 * compute-fbank-feats or torchaudio.compliance.kaldi.fbank make it: frames that are not centred, each with its DC removed and
 * pre-emphasised before the window, zero-padded into a longer transform, HTK-mel triangles without area normalisation, the
 * natural logarithm.  It cannot be made from the log-mel output above.  These calls compute it from the device-resident lanes
 * (csrc/kernels_clips_mel.hip: the mel export's kernel with the conditioned form on).  For a clip row:
 * - Channel, best_rms, runner_up_rms: fvad_clips_export's bits over every sample, as in the mel export.
 * - Feature stream: s[i] = f32(clip sample skip + i * step) * scale, i < L = ceil((len - skip) / step); step, skips and PCM16
 *   follow the mel export's rules; scale is a finite non-zero f32 and the product is rounded once (Kaldi's own convention is
 *   32768, which only moves the exponent).
 * - Parameters: win_length in 2..n_fft; n_fft even in 4..FVAD_CLIP_MEL_NFFT_MAX; hop in 1..win_length; n_mels in
 *   1..FVAD_CLIP_MEL_BANDS_MAX; preemph a finite f32 in [0, 1]; remove_dc 0 or 1; the caller's window[win_length] and
 *   matrix[n_mels][n_fft / 2 + 1]; floor finite and positive.
 * - Frames (Kaldi's snip_edges = true): T = 1 + (L - win_length) / hop for L >= win_length; a clip with L < win_length is
 *   refused, as the mel export refuses one too short to reflect.  Frame t is x[i] = s[t * hop + i], i < win_length.  Nothing
 *   outside the clip is read, no sample off the stride, and there is no reflection.
 * - Conditioning of a frame, in f32, every operation rounded on its own (fp contraction is off for the library), in this order:
 *   1. with remove_dc, d[i] = x[i] - mean, mean = (sum of x[i]) / f32(win_length); without, d = x.  The order of the sum is
 *      fixed for a given win_length and the same for every frame, tile and wavefront slot (the kernel's header states it).
 *   2. y[0] = d[0] - preemph * d[0] and y[i] = d[i] - preemph * d[i - 1] (Kaldi's replicated first sample): one rounded
 *      product and one rounded difference each.
 *   3. z[i] = y[i] * window[i], zero for win_length <= i < n_fft.
 * - Then as the mel export: P[k] = |rfft(z)[k]|^2; mel[m] = sum_k M[m][k] * P[k] over ascending k, one rounded product and one
 *   rounded sum each; feat = logf(fmaxf(mel, floor)), the natural logarithm.  logf(floor) is evaluated on the host in double and
 *   rounded once and is what every mel <= floor gives: digital silence is exactly that value in every band.
 * - Output: per clip [T][n_mels] f32 in 16-byte-aligned slots in clip order (fvad_clips_plan_fbank); the padding is never
 *   written by the device form and zeroed by the host form -- the mel export's rules.
 * - Cepstral mean subtraction, cmn 0 or 1 (torchaudio's subtract_mean), in THIS order, so that numpy float32 evaluated in it is
 *   the exact model: within a tile of min(32, (8192 - win_length) / hop + 1) consecutive frames the features of a band are
 *   added over ascending t onto 0.0f by one lane; the tiles' sums are then added in tile order onto 0.0f by one lane per (clip,
 *   band); mean_m = that sum / f32(T), one rounded division; with cmn, feat' = feat - mean_m, one rounded subtraction.
 * - Reports: the four of fvad_clips_export, n_frames, and means[n_clips][n_mels] (may be NULL), filled whether or not cmn is set.
 * - INVARIANTS, bit for bit: a frame's features before cmn depend on that frame's samples and the call's parameters alone -- not
 *   on the other clips, their order, the tile or slot, the alignment of either side or the call form -- and repeat run after
 *   run.  Every size runs on the generic mixed-radix transform.
 *
 * fvad_mel_design_kaldi (host only): matrix[n_mels][n_fft / 2 + 1] of Kaldi's bank, evaluated in double and rounded once.
 *   mel(f) = 1127 ln(1 + f / 700); high_freq <= 0 means Nyquist + high_freq; n_mels + 2 points equally spaced in mel from
 *   low_freq to high_freq; filter m over the bins k * sample_rate / n_fft, k < n_fft / 2, is max(0, min((mel_k - l) / (c - l),
 *   (r - mel_k) / (r - c))) with l, c, r its three points: the triangle in the mel domain, no normalisation.  The Nyquist column
 *   is zero.  Refusals as fvad_mel_design's (low_freq < 0, high_freq above Nyquist, low_freq >= high_freq, ...).  torchaudio was
 *   not at hand, so the designer is checked against the formula written out independently, not against torchaudio's output.
 * fvad_clips_plan_fbank (host only): n_frames[i], offsets[i] and *total (floats) for clips of lens[i] samples; skips NULL means
 *   all zero.  FVAD_ERR_INVALID_ARGUMENT for a bad step, win_length (2..FVAD_CLIP_MEL_NFFT_MAX), hop or n_mels, a skip >= step,
 *   a clip with len <= skip or L < win_length, NULLs, or a total that does not fit 64 bits.
 * fvad_clips_fbank_check (host only; d_src and out are addresses, nothing is read through them): every argument rule of the two
 *   exports in the one order both report them in -- the mel check's up to the rows' own rules, then step, n_fft, win_length, hop,
 *   n_mels, per clip its skip and frames, a window or matrix value that is not finite, scale, preemph, remove_dc, floor, cmn,
 *   then FVAD_ERR_OUT_OF_RANGE, FVAD_ERR_BUFFER_TOO_SMALL and the grids as in the mel check.
 * fvad_clips_export_fbank_device / fvad_clips_export_fbank: the full-rate call's arguments, then step, skips, win_length, n_fft,
 *   hop, window, n_mels, matrix, scale, preemph, remove_dc, floor, cmn (window, matrix: host memory) and the two reports.  Every
 *   error comes back before any launch.  fvad_ctx_kernel_times names clip_rms, clip_pick, clip_fbank, clip_fbank_mean (always)
 *   and, with cmn, clip_fbank_sub.  The split-source form (sliced runs) is fvad_clips_export_split_fbank* below. */
int fvad_mel_design_kaldi(double sample_rate, uint32_t n_fft, uint32_t n_mels, double low_freq, double high_freq, float *matrix);
int fvad_clips_plan_fbank(const uint64_t *lens, const uint32_t *skips, size_t n_clips, uint32_t step, uint32_t win_length,
                          uint32_t hop, uint32_t n_mels, uint64_t *n_frames, uint64_t *offsets, uint64_t *total);
int fvad_clips_fbank_check(const void *d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                           const uint64_t *clips, size_t n_clips, int out_format, const void *out, size_t out_capacity,
                           int device_out, uint32_t step, const uint32_t *skips, uint32_t win_length, uint32_t n_fft, uint32_t hop,
                           const float *window, uint32_t n_mels, const float *matrix, float scale, float preemph, int remove_dc,
                           float floor, int cmn, uint64_t *n_frames, uint64_t *offsets, uint64_t *total);
int fvad_clips_export_fbank_device(fvad_ctx *ctx, const void *d_src, int src_format, size_t n_lanes, size_t lane_stride,
                                   size_t n_samples, const uint64_t *clips, size_t n_clips, int out_format, void *d_out,
                                   size_t out_capacity, int32_t *best_channel, float *best_rms, float *runner_up_rms,
                                   uint64_t *out_offsets, uint32_t step, const uint32_t *skips, uint32_t win_length, uint32_t n_fft,
                                   uint32_t hop, const float *window, uint32_t n_mels, const float *matrix, float scale,
                                   float preemph, int remove_dc, float floor, int cmn, uint64_t *n_frames, float *means);
int fvad_clips_export_fbank(fvad_ctx *ctx, const void *d_src, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                            const uint64_t *clips, size_t n_clips, int out_format, void *out, size_t out_capacity,
                            int32_t *best_channel, float *best_rms, float *runner_up_rms, uint64_t *out_offsets, uint32_t step,
                            const uint32_t *skips, uint32_t win_length, uint32_t n_fft, uint32_t hop, const float *window,
                            uint32_t n_mels, const float *matrix, float scale, float preemph, int remove_dc, float floor, int cmn,
                            uint64_t *n_frames, float *means);

/* ------------------------------------------------------------------ batch Recorder with a front end: features of split clips
 * The feature exports over the split source of fvad_clips_export_split: the features of a run sliced in time, whose clips have
 * their head in the held tail of earlier slices (buffer A) and their body in the current slice (buffer B).  Rows are
 * FVAD_CLIP_SPLIT_FIELDS rows and the buffers are passed as there; everything behind the rows is the contiguous call's argument
 * list, unchanged, and so are the reports.  fvad_clips_plan_mel and fvad_clips_plan_fbank plan them with lens[i] = a_len + b_len.
 * - The mapping: stream sample i of a clip is clip sample e = skip + i * step, read from piece A at a_from + e when e < a_len,
 *   else from piece B at b_from + (e - a_len).  The stride is counted from the clip's first sample and runs through the seam;
 *   frames and tiles are counted from the clip's first kept sample, never from the seam.  Nothing outside either piece is read,
 *   and at a step above 1 no sample off the stride.
 * - INVARIANTS, bit for bit: every result -- n_frames, offsets, best_channel, both RMS values, feat_max or means, every feature,
 *   with or without norm / cmn -- is the contiguous call's over the same samples laid out contiguously, wherever the seam is; a
 *   clip's results do not depend on the other rows, their order, either piece's alignment or the call form; a refused call
 *   launches nothing and writes nothing.
 * - The rules, in the one order all six entry points report them in:
 *   1. fvad_clips_split_check's down to the rows' own rule (a clip with both lengths 0 or no channels); directly behind its
 *      format rule: window or matrix NULL ("NULL argument"), then out_format other than FVAD_CLIP_F32 ("features are f32: ...");
 *   2. the family's rules as fvad_clips_mel_check / fvad_clips_fbank_check state them from the frame parameters on: step, n_fft,
 *      (win_length,) hop, n_mels, every clip's skip, length and slot with len = a_len + b_len, a window or matrix value that is
 *      not finite, the family's own conditions;
 *   3. FVAD_ERR_OUT_OF_RANGE for a piece past its buffer's samples or lanes;
 *   4. FVAD_ERR_BUFFER_TOO_SMALL for out_capacity below the plan's total;
 *   5. the output overlapping a source;
 *   6. more than 2^31 - 1 RMS units or tiles of frames in one call.
 * fvad_clips_split_mel_check / fvad_clips_split_fbank_check (host only; pointers are addresses): these rules; n_frames, offsets and
 *   *total (each may be NULL) are filled as far as the rules held.
 * fvad_clips_export_split_mel(_device) / fvad_clips_export_split_fbank(_device): every error comes back before any launch.
 *   fvad_ctx_kernel_times names clip_rms_split, clip_pick and the contiguous call's feature labels. */
int fvad_clips_split_mel_check(const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void *d_b, size_t b_lanes,
                               size_t b_stride, size_t b_samples, int src_format, const uint64_t *clips, size_t n_clips,
                               int out_format, const void *out, size_t out_capacity, int device_out, uint32_t step,
                               const uint32_t *skips, uint32_t n_fft, uint32_t hop, const float *window, uint32_t n_mels,
                               const float *matrix, float floor, const float *norm, uint64_t *n_frames, uint64_t *offsets,
                               uint64_t *total);
int fvad_clips_export_split_mel_device(fvad_ctx *ctx, const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                       const void *d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                       const uint64_t *clips, size_t n_clips, int out_format, void *d_out, size_t out_capacity,
                                       int32_t *best_channel, float *best_rms, float *runner_up_rms, uint64_t *out_offsets,
                                       uint32_t step, const uint32_t *skips, uint32_t n_fft, uint32_t hop, const float *window,
                                       uint32_t n_mels, const float *matrix, float floor, const float *norm, uint64_t *n_frames,
                                       float *feat_max);
int fvad_clips_export_split_mel(fvad_ctx *ctx, const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void *d_b,
                                size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t *clips,
                                size_t n_clips, int out_format, void *out, size_t out_capacity, int32_t *best_channel,
                                float *best_rms, float *runner_up_rms, uint64_t *out_offsets, uint32_t step, const uint32_t *skips,
                                uint32_t n_fft, uint32_t hop, const float *window, uint32_t n_mels, const float *matrix,
                                float floor, const float *norm, uint64_t *n_frames, float *feat_max);
int fvad_clips_split_fbank_check(const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void *d_b, size_t b_lanes,
                                 size_t b_stride, size_t b_samples, int src_format, const uint64_t *clips, size_t n_clips,
                                 int out_format, const void *out, size_t out_capacity, int device_out, uint32_t step,
                                 const uint32_t *skips, uint32_t win_length, uint32_t n_fft, uint32_t hop, const float *window,
                                 uint32_t n_mels, const float *matrix, float scale, float preemph, int remove_dc, float floor,
                                 int cmn, uint64_t *n_frames, uint64_t *offsets, uint64_t *total);
int fvad_clips_export_split_fbank_device(fvad_ctx *ctx, const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples,
                                         const void *d_b, size_t b_lanes, size_t b_stride, size_t b_samples, int src_format,
                                         const uint64_t *clips, size_t n_clips, int out_format, void *d_out, size_t out_capacity,
                                         int32_t *best_channel, float *best_rms, float *runner_up_rms, uint64_t *out_offsets,
                                         uint32_t step, const uint32_t *skips, uint32_t win_length, uint32_t n_fft, uint32_t hop,
                                         const float *window, uint32_t n_mels, const float *matrix, float scale, float preemph,
                                         int remove_dc, float floor, int cmn, uint64_t *n_frames, float *means);
int fvad_clips_export_split_fbank(fvad_ctx *ctx, const void *d_a, size_t a_lanes, size_t a_stride, size_t a_samples, const void *d_b,
                                  size_t b_lanes, size_t b_stride, size_t b_samples, int src_format, const uint64_t *clips,
                                  size_t n_clips, int out_format, void *out, size_t out_capacity, int32_t *best_channel,
                                  float *best_rms, float *runner_up_rms, uint64_t *out_offsets, uint32_t step, const uint32_t *skips,
                                  uint32_t win_length, uint32_t n_fft, uint32_t hop, const float *window, uint32_t n_mels,
                                  const float *matrix, float scale, float preemph, int remove_dc, float floor, int cmn,
                                  uint64_t *n_frames, float *means);

/* ------------------------------------------------------------------ device-side ingest: a corpus's bytes into planar lanes
 * The way in for the batch paths, as fvad_clips_* is the way out: the bytes of WAV data chunks go to the device as the files
 * hold them -- interleaved frames at the file's sample width -- and ONE kernel (csrc/kernels_ingest.hip) de-interleaves,
 * decodes and zero-pads them into the planar lanes fvad_engine_enqueue_device* and fvad_clips_export* take.  The host does no
 * per-sample work, a PCM16 corpus crosses PCIe at 2 bytes per sample, and 24-bit PCM -- which fvad_wav_read refuses -- is usable.
 * - Format pairs (source -> lanes), all exact: PCM16 -> f32 is (float)s * (1.0f / 32768.0f), fvad_lane.pcm_i16's rule; PCM16 ->
 *   PCM16 the bits; PCM24 (3 bytes little-endian, sign-extended) -> f32 is (float)s * (1.0f / 8388608.0f), exact because
 *   |s| <= 2^23 fits the f32 significand and the scale is a power of two (libsndfile's normalised float read of 24-bit PCM
 *   [external: libsndfile is not part of this build, not verifiable here]); f32 -> f32 the bits, NaN payloads and -0 included.
 *   PCM24 -> PCM16 and f32 -> PCM16 are conversions, not ingest: FVAD_ERR_INVALID_ARGUMENT.
 * - A source (a file, or a slice of one) is a row of FVAD_INGEST_FIELDS uint64: byte_offset (where its frame 0 starts in the
 *   raw bytes: any value, a data chunk usually starts at byte 44), n_frames, n_channels (1 .. 64), format (FVAD_INGEST_*),
 *   first_lane (channel c goes to lane first_lane + c), dst_offset (the lane sample frame 0 is written to), fill_to (>=
 *   dst_offset + n_frames: the lane samples [dst_offset + n_frames, fill_to) of the source's lanes are written as zeros -- the
 *   padding of a ragged batch without a memset).  Lanes are laid out as for fvad_engine_enqueue_device*: lane l at d_lanes +
 *   l * lane_stride samples of out_format, n_samples each; lane_stride and dst_offset need no alignment.
 * - Nothing outside a source's bytes [byte_offset, byte_offset + n_frames * n_channels * bytes per sample) is read and nothing
 *   outside [dst_offset, fill_to) of its lanes is written.  INVARIANT: the lanes get the same bits whatever the order of the
 *   sources, however they are split over calls, and run after run (no atomics; a source's output depends on its bytes alone).
 *
 * fvad_wav_probe (host only): walks the RIFF chunks as fvad_wav_read does (the first "fmt " and "data" chunks,
 * WAVE_FORMAT_EXTENSIBLE's sub-format, a data length past the end of the file cut to the file, a partial last frame dropped)
 * WITHOUT reading the samples: info[FVAD_WAV_INFO_FIELDS] = format (FVAD_INGEST_*), n_channels, sample_rate, data_offset (bytes
 * from the start of the file), n_frames, bits.  PCM16, PCM24 and 32-bit float are accepted; everything fvad_wav_read refuses
 * except 24-bit PCM is refused the same way (FVAD_ERR_MODEL_FORMAT; FVAD_ERR_IO for a file that cannot be opened).
 * fvad_ingest_check (host only): every argument rule of the two calls below, in this order: FVAD_ERR_INVALID_ARGUMENT for a bad
 * out_format, NULL sources, lane_stride < n_samples with several lanes; then per source FVAD_ERR_INVALID_ARGUMENT for a bad
 * format or pair, n_channels outside 1 .. 64, fill_to < dst_offset + n_frames; then per source FVAD_ERR_OUT_OF_RANGE for lanes
 * past n_lanes, fill_to > n_samples, byte_offset + bytes > raw_bytes; then FVAD_ERR_INVALID_ARGUMENT when two sources'
 * destination ranges [dst_offset, fill_to) overlap on a common lane (the order of the writes would decide the result; equal
 * ranges on different lanes, and adjacent ranges on one lane, are fine).  n_sources == 0 succeeds; a source with n_frames == 0
 * only fills.
 * fvad_ingest_device: d_raw holds raw_bytes bytes on the device.  Runs fvad_ingest_check (and refuses NULL pointers and lanes
 * that are not aligned to their samples) before any launch, returns when the lanes are written, and names `ingest` in
 * fvad_ctx_kernel_times (one launch per source format present).  A launch takes fewer than 2^24 tiles (16 KB of source bytes or
 * 8192 zeros of a lane each): a call with more -- some 270 GB of source -- is FVAD_ERR_INVALID_ARGUMENT; ingest in batches.
 * fvad_ingest: the same for bytes in host memory (mapped files, pageable or page-locked): source i's byte_offset is relative to
 * src_host[i] (which may be NULL when n_frames == 0).  The bytes are copied, as they are, into a two-slot page-locked ring the
 * context keeps (context option ingest_ring_bytes / FVAD_INGEST_RING_BYTES at creation: the raw bytes per batch, default 32 MB,
 * 1 KB .. 1 GB in multiples of 16) and uploaded batch by batch, the kernel running on one batch while the next is copied; a
 * source larger than what is left of a batch is cut at a multiple of 4 frames.  The result has the same bits however the ring
 * cuts the sources, and the same as fvad_ingest_device's. */
enum { FVAD_INGEST_F32 = 0, FVAD_INGEST_PCM16 = 1, FVAD_INGEST_PCM24 = 2 };
#define FVAD_INGEST_FIELDS 7
#define FVAD_WAV_INFO_FIELDS 6
int fvad_wav_probe(const char *path, uint64_t *info);
int fvad_ingest_check(const uint64_t *sources, size_t n_sources, uint64_t raw_bytes, int out_format, size_t n_lanes,
                      size_t lane_stride, size_t n_samples);
int fvad_ingest_device(fvad_ctx *ctx, const void *d_raw, uint64_t raw_bytes, const uint64_t *sources, size_t n_sources,
                       int out_format, void *d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples);
int fvad_ingest(fvad_ctx *ctx, const void *const *src_host, const uint64_t *sources, size_t n_sources, int out_format,
                void *d_lanes, size_t n_lanes, size_t lane_stride, size_t n_samples);

/* ------------------------------------------------------------------ resampling ingest: corpora at other rates into 48 kHz lanes
 * The batch paths run at 48 kHz.  A file at another rate (44.1 kHz, 32 kHz, 16 kHz ...) goes to the device as its own bytes, as
 * with fvad_ingest, and ONE kernel (csrc/kernels_ingest_resample.hip) decodes, de-interleaves, filters and re-times it: a
 * rational up/down polyphase resampler inside the ingest.  The lanes are ordinary 48 kHz f32 lanes.
 * THE DEFINITION
 * - A ratio is up/down = rate_out/rate_in in lowest terms (fvad_resample_ratio): 44100 -> 48000 is 160/147, 32000 3/2,
 *   22050 320/147, 16000 3/1, 24000 2/1, 8000 6/1, 96000 1/2, 11025 640/147.  1 <= up <= FVAD_RESAMPLE_UP_MAX, down >= 1.
 * - The prototype is taps[0 .. 2 K], an odd count n_taps <= FVAD_RESAMPLE_TAPS_MAX with centre K; it need not be symmetric.
 * - A file of file_frames frames has out_frames = ceil(file_frames * up / down) outputs (fvad_resample_out_frames).
 * - Output o of a channel is
 *       y[o] = sum over n of x[n] * taps[K + o * down - n * up],   over every n whose tap index lies in [0, 2 K],
 *   x[n] the decoded sample of frame n (fvad_ingest's rules: PCM16 s / 32768, PCM24 s / 8388608, f32 the value) and 0 outside
 *   [0, file_frames).  The filter is centred (zero phase): output o sits at time o / rate_out of the file, so segments, labels
 *   and clip indices need no delay correction.  A file is filtered as a finite signal; nothing outside it is read.
 * - Index arithmetic is 64-bit throughout (o * down passes 2^32 after 10.1 minutes of 44.1 kHz audio); file_frames * up must
 *   stay below 2^62.
 * - The lanes are f32.  PCM16 lanes would be a conversion: FVAD_ERR_INVALID_ARGUMENT, as fvad_ingest says for PCM24 -> PCM16.
 * - INVARIANTS, all bit for bit.  A file's lane bits do not depend on how the file is cut into sources or calls (time slices),
 *   on the order of the sources, on the other sources of the call, on which tile of the kernel an output falls in, on the call
 *   form (device bytes or host bytes), on ingest_ring_bytes or on the destination's alignment.  A PCM16 source gives the bits of
 *   an f32 source holding s / 32768, PCM24 likewise with s / 8388608.  No atomics; nothing outside [dst_offset, fill_to) of a
 *   source's lanes is written.  (Every output is one f32 fma chain from +0 in an order that depends on up, down, n_taps and
 *   o mod up alone; the order itself is not part of the contract.)
 * - A source is a row of FVAD_RESAMPLE_FIELDS uint64: byte_offset (where frame `frame_base` lies in the raw bytes), n_frames
 *   (the frames given), n_channels, format, first_lane, dst_offset (the lane sample output out_from is written to), fill_to (>=
 *   dst_offset + n_out; zeros behind the outputs), frame_base, file_frames, out_from, n_out.  The row asks for outputs
 *   [out_from, out_from + n_out) of the file and gives frames [frame_base, frame_base + n_frames) of it: a slice of a file is a
 *   row whose given frames cover the window of its outputs, and is then the whole file's result by construction.  One ratio and
 *   one set of taps per call.
 *
 * Host only (csrc/host_resample.cpp):
 * fvad_resample_ratio: up/down = rate_out/rate_in reduced by their gcd; FVAD_ERR_INVALID_ARGUMENT for a zero rate, NULL or
 *   up > FVAD_RESAMPLE_UP_MAX.
 * fvad_resample_out_frames: ceil(file_frames * up / down), saturated at UINT64_MAX; 0 for a ratio that is none.
 * fvad_resample_design: fvad_clips_fir_design's rule with m = max(up, down): K = half * m, taps[0 .. 2 K] with
 *   h[k] = 2 cutoff sinc(2 cutoff (k - K)) * kaiser(2 K + 1, beta)[k] in float64, normalised to sum `up` (unit DC gain), then
 *   rounded to f32; *n_taps = 2 K + 1.  cutoff is in cycles per sample of the up-times-oversampled input.  half == 0 selects
 *   16, cutoff == 0 selects 0.45 / m, beta == 0 selects 6.  FVAD_ERR_INVALID_ARGUMENT for a ratio that is none, 2 half m + 1 >
 *   FVAD_RESAMPLE_TAPS_MAX (= 2 * 16 * 640 + 1, the default design at the largest up), a cutoff not in (0, 0.5] (0 apart), a
 *   negative or non-finite beta, or NULL.  The default design, computed from these taps in float64 (tools/resample_response.py):
 *     ratios 160/147, 320/147, 640/147: pass-band ripple up to 0.40/m 0.11 dB, stop band from 0.60/m -69.8 dB (160/147: -69.9),
 *                                       33 taps a phase, the phases' DC gains within 2.8e-4 of each other
 *     ratios 3/1, 3/2:                  0.11 dB, -72.1 dB, 33 taps a phase, 2.3e-4
 *     ratio 6/1:                        0.11 dB, -70.8 dB, 33 taps a phase, 2.6e-4
 *     ratios 2/1, 1/2:                  0.11 dB, -74.1 dB, 33 taps a phase (1/2: 65, one phase), 2.1e-4
 * fvad_resample_window: the input frames [*frame_lo, *frame_hi) that outputs [out_from, out_from + n_out) read, clipped to the
 *   file; an empty window (n_out == 0, a phase without taps) has *frame_lo == *frame_hi.
 * fvad_ingest_resample_tile: the kernel's outputs of one channel per tile for frames of n_channels samples of `format`; 0 when
 *   the window of 4 outputs does not fit the 64 KB of LDS a tile stages (such a source is refused).
 * fvad_ingest_resample_check: every argument rule of the two calls below, in this order: FVAD_ERR_INVALID_ARGUMENT for an
 *   out_format other than FVAD_INGEST_F32, a ratio that is none, taps that fail (NULL, an even or zero count, more than
 *   FVAD_RESAMPLE_TAPS_MAX, a non-finite tap); n_sources == 0 succeeds here; NULL sources, lane_stride < n_samples with several
 *   lanes; then per source FVAD_ERR_INVALID_ARGUMENT for a bad format, n_channels outside 1 .. 64, file_frames * up >= 2^62,
 *   out_from + n_out > out_frames(file_frames), fill_to < dst_offset + n_out, given frames that leave the file, given frames
 *   that do not cover fvad_resample_window of the row, a tile of 0; then per source FVAD_ERR_OUT_OF_RANGE for lanes past
 *   n_lanes, fill_to > n_samples, byte_offset + bytes > raw_bytes; then FVAD_ERR_INVALID_ARGUMENT for overlapping destinations
 *   (fvad_ingest_check's rule).  A source with n_out == 0 only fills.
 * fvad_ingest_resample_device / fvad_ingest_resample: fvad_ingest_device's and fvad_ingest's forms.  Both run the check (and
 *   refuse NULL pointers and lanes not aligned to 4 bytes) before any launch, return when the lanes are written and name
 *   `ingest_resample` in fvad_ctx_kernel_times.  The host form cuts a source into batches of the context's ring in OUTPUT
 *   coordinates and copies each batch's window (batches overlap by the filter's reach); a ring smaller than the window of 4
 *   outputs is enlarged for the call. */
#define FVAD_RESAMPLE_FIELDS 11
#define FVAD_RESAMPLE_UP_MAX 640
#define FVAD_RESAMPLE_TAPS_MAX 20481
int fvad_resample_ratio(uint32_t rate_in, uint32_t rate_out, uint32_t *up, uint32_t *down);
uint64_t fvad_resample_out_frames(uint64_t file_frames, uint32_t up, uint32_t down);
int fvad_resample_design(uint32_t up, uint32_t down, uint32_t half, double cutoff, double beta, float *taps, uint32_t *n_taps);
int fvad_resample_window(uint32_t up, uint32_t down, uint32_t n_taps, uint64_t file_frames, uint64_t out_from, uint64_t n_out,
                         uint64_t *frame_lo, uint64_t *frame_hi);
uint64_t fvad_ingest_resample_tile(uint32_t up, uint32_t down, uint32_t n_taps, uint32_t n_channels, uint32_t format);
int fvad_ingest_resample_check(const uint64_t *sources, size_t n_sources, uint64_t raw_bytes, uint32_t up, uint32_t down,
                               const float *taps, uint32_t n_taps, int out_format, size_t n_lanes, size_t lane_stride,
                               size_t n_samples);
int fvad_ingest_resample_device(fvad_ctx *ctx, const void *d_raw, uint64_t raw_bytes, const uint64_t *sources, size_t n_sources,
                                uint32_t up, uint32_t down, const float *taps, uint32_t n_taps, void *d_lanes, size_t n_lanes,
                                size_t lane_stride, size_t n_samples);
int fvad_ingest_resample(fvad_ctx *ctx, const void *const *src_host, const uint64_t *sources, size_t n_sources, uint32_t up,
                         uint32_t down, const float *taps, uint32_t n_taps, void *d_lanes, size_t n_lanes, size_t lane_stride,
                         size_t n_samples);

/* ------------------------------------------------------------------ device-side egress: planar lanes into a file's bytes
 * The ingest's inverse, the way out for whole recordings: ONE kernel (csrc/kernels_egress.hip) converts planar device lanes --
 * the denoised lanes of fvad_engine_enqueue_device*, or any others -- to the sample format of a WAV file and interleaves them
 * into the bytes of its data chunk.  The host does no per-sample work, a PCM16 file crosses PCIe at 2 bytes per sample, and
 * 24-bit PCM files, which fvad_wav_write cannot write, can be written.
 * - A sink (a file, or a time slice of one) is a row of FVAD_EGRESS_FIELDS uint64: byte_offset (where its frame 0 goes in the
 *   output bytes: any value, a data chunk usually starts at byte 44, which is 12 modulo 16), n_frames, n_channels (1 .. 64),
 *   format (the FILE's sample format, FVAD_INGEST_*), first_lane (channel c is lane first_lane + c), src_offset (the lane
 *   sample frame 0 is taken from).  Lanes are laid out as for fvad_ingest: lane l at d_lanes + l * lane_stride samples of
 *   src_format (FVAD_INGEST_F32 or FVAD_INGEST_PCM16), n_samples each; nothing needs alignment beyond the sample's size.
 *   Sample (f, c) of a sink goes to byte_offset + (f * n_channels + c) * bytes per sample, little-endian.
 * - Format pairs (lanes -> file): f32 -> f32 the bits (moved as 32-bit integers: NaN payloads and -0 survive); f32 -> PCM16 is
 *   rint(fminf(fmaxf(y * 32768.0f, -32768.0f), 32767.0f)), ties to even, NaN gives -32768 (as fmaxf gives there): the rule of
 *   fvad_lane.denoised_i16 and of PCM16 clips (csrc/clip_device.h) -- NOT fvad_wav_write's libsndfile rule
 *   lrintf(clip(x, -1, 1) * 32767), so a PCM16 file written here and one fvad_wav_write(as_pcm16) wrote differ; f32 -> PCM24 is
 *   rint(fminf(fmaxf(y * 8388608.0f, -8388608.0f), 8388607.0f)) written as its low three bytes (the scale is a power of two and
 *   both bounds are exact in f32: the inverse of fvad_ingest's s / 8388608 for every value that came from a 24-bit file, as
 *   the PCM16 rule is of s / 32768); PCM16 -> PCM16 the bits.  PCM16 lanes -> f32 or PCM24 files are conversions, not egress:
 *   FVAD_ERR_INVALID_ARGUMENT.
 * - INVARIANTS, all bit for bit.  No byte outside [byte_offset, byte_offset + n_frames * n_channels * bytes per sample) of a
 *   sink is written; no sample outside [src_offset, src_offset + n_frames) of its lanes is read.  The output does not depend on
 *   the order of the sinks, on how a file is cut into sinks or calls, on ingest_ring_bytes, on the call form (device bytes or
 *   host bytes), or on the alignment of either side.  No atomics; a sink's bytes depend on its lanes' samples alone.
 *
 * fvad_wav_header (host only): the FVAD_WAV_HEADER_BYTES (44) bytes of the canonical header -- RIFF, "fmt " of length 16, no
 *   "fact" chunk, "data" -- into out[0 .. cap), *n_bytes = 44.  For f32 (tag 3, 32 bits) and PCM16 (tag 1, 16 bits) byte for
 *   byte what fvad_wav_write / fvad_wav_write_i16 put in front of their samples; for PCM24 tag 1, 24 bits, block align 3 *
 *   n_channels.  FVAD_ERR_INVALID_ARGUMENT for a bad format, zero or more than 65535 channels, a zero rate, data bytes above
 *   0xFFFFFF00 (their refusals) or NULL; FVAD_ERR_BUFFER_TOO_SMALL for cap < 44 (with *n_bytes set).  fvad_wav_probe on header
 *   + data returns the arguments back.
 * fvad_egress_check (host only): every argument rule of the two calls below, in this order: FVAD_ERR_INVALID_ARGUMENT for a bad
 *   src_format, NULL sinks, lane_stride < n_samples with several lanes; then per sink FVAD_ERR_INVALID_ARGUMENT for a bad format
 *   or pair, n_channels outside 1 .. 64; then per sink FVAD_ERR_OUT_OF_RANGE for lanes past n_lanes, src_offset + n_frames >
 *   n_samples, byte_offset + bytes > out_bytes (all sums checked for 64-bit overflow); then FVAD_ERR_INVALID_ARGUMENT when two
 *   sinks' byte ranges overlap (the order of the writes would decide the result; ranges that touch are fine).  n_sinks == 0
 *   succeeds; a sink with n_frames == 0 writes nothing.
 * fvad_egress_device: d_out holds out_bytes bytes on the device.  Runs fvad_egress_check (and refuses NULL pointers and lanes
 *   that are not aligned to their samples) before any launch, returns when the bytes are written, and names `egress` in
 *   fvad_ctx_kernel_times (one launch per file format present).  A launch takes fewer than 2^24 tiles (16 KB of output bytes
 *   each): a call with more is FVAD_ERR_INVALID_ARGUMENT; write in batches.
 * fvad_egress: the same for bytes in host memory (a mapped output file, pageable or page-locked memory): sink i's byte_offset
 *   is relative to dst_host[i] (which may be NULL when n_frames == 0), and the overlap rule applies to the absolute host ranges.
 *   The kernel writes batch after batch into the two-slot page-locked ring fvad_ingest uses (ingest_ring_bytes: the output bytes
 *   per batch); each batch is copied back and moved into place with memcpy while the kernel fills the other slot.  A sink larger
 *   than what is left of a batch is cut at a multiple of 4 frames.  The bytes are the same however the ring cuts the sinks, and
 *   the same as fvad_egress_device's. */
#define FVAD_EGRESS_FIELDS 6
#define FVAD_WAV_HEADER_BYTES 44
int fvad_wav_header(int format, uint32_t n_channels, uint32_t sample_rate, uint64_t n_frames, uint8_t *out, size_t cap,
                    size_t *n_bytes);
int fvad_egress_check(const uint64_t *sinks, size_t n_sinks, uint64_t out_bytes, int src_format, size_t n_lanes,
                      size_t lane_stride, size_t n_samples);
int fvad_egress_device(fvad_ctx *ctx, const void *d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                       const uint64_t *sinks, size_t n_sinks, void *d_out, uint64_t out_bytes);
int fvad_egress(fvad_ctx *ctx, const void *d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                const uint64_t *sinks, size_t n_sinks, void *const *dst_host);

/* ------------------------------------------------------------------ resampling egress: denoised recordings at another rate
 * fvad_egress writes a recording at the lanes' 48 kHz.  A corpus at 44.1 kHz (32 kHz, 16 kHz ...) wants its denoised recordings
 * back at its own rate: ONE kernel (csrc/kernels_egress_resample.hip) is the egress kernel with the rational polyphase resampler
 * of the clip export in front of its conversion.  The lanes never leave the device as f32, the host does no per-sample work.
 * THE DEFINITION
 * - Source lanes are planar f32 at 48 kHz (FVAD_INGEST_F32, laid out as for fvad_egress).  PCM16 lanes are refused with
 *   FVAD_ERR_INVALID_ARGUMENT, as the resampling ingest refuses PCM16 lanes.
 * - up/down = rate_out/48000 in lowest terms, as fvad_resample_ratio(48000, rate_out, ...) gives it: 44100 is 147/160, 32000
 *   2/3, 16000 1/3.  1 <= up <= FVAD_RESAMPLE_UP_MAX, down >= 1.  The taps are an odd count n_taps <= FVAD_RESAMPLE_TAPS_MAX in
 *   host memory with centre K = (n_taps - 1) / 2; they need not be symmetric.  One ratio and one set of taps per call.
 * - A stream of stream_frames lane samples per channel has out_frames = ceil(stream_frames * up / down) output frames
 *   (fvad_resample_out_frames).  Output o of channel c is
 *       y[o] = sum over n of x_c[n] * taps[K + o * down - n * up],   over every n whose tap index lies in [0, 2 K],
 *   x_c the stream's samples of lane first_lane + c and 0 outside [0, stream_frames), accumulated in f32 as one fma chain from
 *   +0 (the chain's order is kernels_clips_resample.hip's and, as there, not part of the contract).  The filter is centred: output
 *   o sits at time o / rate_out of the stream.  y is converted to the file's format by fvad_egress's rules for f32 lanes: f32
 *   keeps the value, PCM16 is rint(fminf(fmaxf(y * 32768.0f, -32768.0f), 32767.0f)), PCM24 the same with 8388608 / 8388607, its
 *   low three bytes.  Sample (o, c) is written little-endian at byte_offset + ((o - out_from) * n_channels + c) * bytes per
 *   sample.
 * - A sink row is FVAD_EGRESS_RESAMPLE_FIELDS uint64: byte_offset (where output out_from goes), n_out, n_channels (1 .. 64),
 *   format (the FILE's, FVAD_INGEST_*), first_lane, src_offset (the lane sample that holds stream sample frame_base),
 *   frame_base, n_frames (the lanes hold the stream samples [frame_base, frame_base + n_frames) for this row), stream_frames,
 *   out_from.  A recording is a stream, not a finite clip: a time slice cannot finish the outputs whose window reaches into the
 *   next slice, so a row names its outputs [out_from, out_from + n_out) and the frames it is given apart, as the resampling
 *   ingest's row does.  The given frames must cover fvad_resample_window(up, down, n_taps, stream_frames, out_from, n_out); a
 *   superset is fine.  Nothing outside [src_offset, src_offset + n_frames) of a lane is read, nothing outside the given frames
 *   and [0, stream_frames) enters a sum.  Index arithmetic is 64-bit (o * down passes 2^32 after 11 minutes at 147/160);
 *   stream_frames * up must stay below 2^62.
 * - INVARIANTS, all bit for bit.  A stream's bytes do not depend on how it is cut into rows or calls (time slices, any out_from,
 *   any superset of the window), on the order of the rows or the other rows of the call, on which tile of the kernel an output
 *   falls in, on the call form (device bytes or host bytes), on ingest_ring_bytes or on the alignment of either side.  The PCM16
 *   and PCM24 bytes of an output are the conversion of the f32 value the same row gives as an f32 file.  No byte outside a row's
 *   range is written, also where another row touches it.  No atomics.  up == down == 1 with the single tap 1.0 gives
 *   fvad_egress's bytes, a -0.0 sample apart (fma(1, -0, +0) is +0).
 *
 * Host only (csrc/host_egress_resample.cpp, the rules in csrc/egress_resample.h):
 * fvad_egress_resample_tile: the kernel's output frames per tile for frames of n_channels samples of `format`: the most, a
 *   multiple of 4, whose bytes fit the egress's 16 KB tile and whose window of one channel fits the 8192 lane samples a tile
 *   stages; 0 when not even 4 outputs' window fits (such a row is refused) or for arguments that are none.
 * fvad_egress_resample_ready: the number of leading outputs of a stream whose whole window lies below frames_have: out_frames
 *   when frames_have >= stream_frames, otherwise ceil((frames_have * up - K) / down) clamped to [0, out_frames] (128-bit
 *   intermediates); 0 for a ratio or a tap count that is none.  What a sliced caller can finish with the frames it has.
 * fvad_egress_resample_check: every argument rule of the two calls below, in this order: FVAD_ERR_INVALID_ARGUMENT for a
 *   src_format other than FVAD_INGEST_F32, a ratio that is none, taps that fail (NULL, an even or zero count, more than
 *   FVAD_RESAMPLE_TAPS_MAX, a non-finite tap); n_sinks == 0 succeeds here; NULL sinks, lane_stride < n_samples with several
 *   lanes; then per row FVAD_ERR_INVALID_ARGUMENT for a bad format, n_channels outside 1 .. 64, stream_frames * up >= 2^62,
 *   out_from + n_out > out_frames(stream_frames), given frames that leave the stream, given frames that do not cover
 *   fvad_resample_window of the row, a tile of 0; then per row FVAD_ERR_OUT_OF_RANGE for lanes past n_lanes, src_offset +
 *   n_frames > n_samples, byte_offset + bytes > out_bytes (all sums checked for 64-bit overflow); then
 *   FVAD_ERR_INVALID_ARGUMENT when two rows' byte ranges overlap (ranges that touch are fine).  A row with n_out == 0 writes
 *   nothing.
 * fvad_egress_resample_device / fvad_egress_resample: fvad_egress_device's and fvad_egress's forms.  Both run the check (and
 *   refuse NULL pointers and lanes not aligned to 4 bytes) before any launch, return when the bytes are written and name
 *   `egress_resample` in fvad_ctx_kernel_times (one launch per file format present, fewer than 2^24 tiles each).  The tap table
 *   is uploaded once per call.  The host form goes through the ring fvad_ingest and fvad_egress use and cuts a row into pieces
 *   in OUTPUT frames at multiples of 4: a piece is the row with out_from advanced and the same given frames (the lanes are on
 *   the device already: no window is copied), so the bytes cannot depend on the cut. */
#define FVAD_EGRESS_RESAMPLE_FIELDS 10
uint64_t fvad_egress_resample_tile(uint32_t up, uint32_t down, uint32_t n_taps, uint32_t n_channels, uint32_t format);
uint64_t fvad_egress_resample_ready(uint32_t up, uint32_t down, uint32_t n_taps, uint64_t stream_frames, uint64_t frames_have);
int fvad_egress_resample_check(const uint64_t *sinks, size_t n_sinks, uint64_t out_bytes, uint32_t up, uint32_t down,
                               const float *taps, uint32_t n_taps, int src_format, size_t n_lanes, size_t lane_stride,
                               size_t n_samples);
int fvad_egress_resample_device(fvad_ctx *ctx, const void *d_lanes, int src_format, size_t n_lanes, size_t lane_stride,
                                size_t n_samples, const uint64_t *sinks, size_t n_sinks, uint32_t up, uint32_t down,
                                const float *taps, uint32_t n_taps, void *d_out, uint64_t out_bytes);
int fvad_egress_resample(fvad_ctx *ctx, const void *d_lanes, int src_format, size_t n_lanes, size_t lane_stride, size_t n_samples,
                         const uint64_t *sinks, size_t n_sinks, uint32_t up, uint32_t down, const float *taps, uint32_t n_taps,
                         void *const *dst_host);

/* ------------------------------------------------------------------ strided resampling egress: recordings from the network's samples
 * NSNet2 works at 16 kHz.  The 48 kHz lanes the engine keeps are the reference's x3 LINEAR interpolation of the network's
 * output: network sample j lands unchanged at lane index 3 j + 2 and the two samples in front of it are lerps.  A lerp is a
 * triangular filter: a network tone at 6 kHz stands in the lanes at -3.8 dB with images at 10 kHz (-11.8 dB, both against the
 * network's tone) and 22 kHz (-20 dB); a 7.5 kHz tone at -6.1 dB, its image at 8.5 kHz at -8.1 dB.  The VAD wants exactly these
 * lanes; a listener does not.  The stream lane[3 j + 2] is the network's output bit for bit, and ONE kernel (csrc/kernels_egress_resample.hip), the
 * resampling egress over a stream that lies src_step apart in its lanes, writes recordings from it: at 16 kHz (1/1 with the
 * tap 1.0) lossless at a third of the bytes, at 48 kHz (3/1) a band-limited interpolation in place of the lerp, at 44.1 kHz one
 * filter (441/160) in place of two.
 * THE DEFINITION is fvad_egress_resample's with one more argument, src_step in 1 .. FVAD_EGRESS_STEP_MAX, and another meaning
 * of the word "stream":
 * - Stream sample n of channel c is lane sample src_offset + (n - frame_base) * src_step of lane first_lane + c, for
 *   frame_base <= n < frame_base + n_frames.  The row keeps its FVAD_EGRESS_RESAMPLE_FIELDS fields and their order;
 *   stream_frames, out_from, frame_base and n_frames count STRIDED samples.  fvad_resample_window, fvad_egress_resample_ready
 *   and fvad_egress_resample_tile are used as they are (the tile's window is 8192 staged samples whatever the step).
 * - The sum, its ascending f32 fma chain from +0 with the zeros outside [0, stream_frames) skipped, the conversion and the
 *   interleaving are fvad_egress_resample's.  So the bytes equal fvad_egress_resample's over a compacted copy of the lanes, and
 *   with src_step == 1 over the same lanes, bit for bit; every invariant of fvad_egress_resample holds.
 * - Nothing outside [src_offset, src_offset + (n_frames - 1) * src_step] of a lane is read, and no sample off the stride
 *   enters a sum (they may be NaN).
 * - The default 3/1 design (fvad_resample_design(3, 1, 0, 0, 0): 97 taps), from tools/resample_response.py: a pass-band ripple
 *   of 0.108 dB up to 6.4 kHz of the 16 kHz stream (-0.10 .. +0.01 dB) and a stop band of -72.1 dB from 9.6 kHz on; in between
 *   the transition band falls through -66.6 dB at 8.5 kHz.  Every image of a network tone up to 6.4 kHz lies at 9.6 kHz or above.
 *
 * fvad_egress_resample_strided_check (host only, csrc/host_egress_strided.cpp, the rules in csrc/egress_strided.h):
 *   fvad_egress_resample_check's rules in its order, with two changes: FVAD_ERR_INVALID_ARGUMENT for a src_step outside
 *   1 .. FVAD_EGRESS_STEP_MAX directly after the ratio's rule, and the lane range rule is n_frames == 0 || src_offset +
 *   (n_frames - 1) * src_step + 1 <= n_samples, evaluated without wrapping, FVAD_ERR_OUT_OF_RANGE otherwise.
 * fvad_egress_resample_strided_device / fvad_egress_resample_strided: fvad_egress_resample_device's and
 *   fvad_egress_resample's forms.  Both run the check (and refuse NULL pointers and lanes not aligned to 4 bytes) before any
 *   launch, return when the bytes are written and name `egress_strided` in fvad_ctx_kernel_times (one launch per file format
 *   present).  The tap table is uploaded once per call; the host form cuts rows at the ring as fvad_egress_resample does. */
#define FVAD_EGRESS_STEP_MAX 16
int fvad_egress_resample_strided_check(const uint64_t *sinks, size_t n_sinks, uint64_t out_bytes, uint32_t up, uint32_t down,
                                       const float *taps, uint32_t n_taps, uint32_t src_step, int src_format, size_t n_lanes,
                                       size_t lane_stride, size_t n_samples);
int fvad_egress_resample_strided_device(fvad_ctx *ctx, const void *d_lanes, int src_format, size_t n_lanes, size_t lane_stride,
                                        size_t n_samples, const uint64_t *sinks, size_t n_sinks, uint32_t up, uint32_t down,
                                        const float *taps, uint32_t n_taps, uint32_t src_step, void *d_out, uint64_t out_bytes);
int fvad_egress_resample_strided(fvad_ctx *ctx, const void *d_lanes, int src_format, size_t n_lanes, size_t lane_stride,
                                 size_t n_samples, const uint64_t *sinks, size_t n_sinks, uint32_t up, uint32_t down,
                                 const float *taps, uint32_t n_taps, uint32_t src_step, void *const *dst_host);

/* ------------------------------------------------------------------ two-source egress: the original beside the denoised
 * fvad_egress writes one lane set.  A user of a denoiser also wants the original to compare against, what was taken out (the
 * residual) and a wet/dry mix -- all of them functions of the ORIGINAL lanes and the DENOISED lanes, which the engine has on
 * the device side by side.  ONE kernel (csrc/kernels_egress_mix.hip) is the egress kernel with two sources and two weights;
 * it needs no third lane set, and each kind of file is one more call.
 * THE DEFINITION
 * - Both lane sets are planar f32 (src_format FVAD_INGEST_F32; PCM16 lanes are refused with FVAD_ERR_INVALID_ARGUMENT, as the
 *   conversions are): d_orig is n_lanes lanes of orig_samples, orig_stride apart, d_den n_lanes lanes of den_samples,
 *   den_stride apart; lane l of one pairs with lane l of the other.  Nothing needs alignment beyond 4 bytes.
 * - A sink row is FVAD_EGRESS_MIX_FIELDS uint64: fvad_egress's six -- byte_offset, n_frames, n_channels (1 .. 64), format (the
 *   FILE's), first_lane, src_offset (into the DENOISED lanes) -- then orig_offset and orig_zeros.  For frame f, channel c:
 *       y = den[first_lane + c][src_offset + f]
 *       x = +0.0f                                                  for f < orig_zeros
 *       x = orig[first_lane + c][orig_offset + (f - orig_zeros)]   otherwise.
 *   The kernel knows nothing of fvad_nsnet2_delay: the caller states the pairing (a whole recording: src_offset = orig_offset
 *   = 0, orig_zeros = the delay; a time slice pairs its own buffers with orig_zeros = 0).
 * - Two finite f32 weights per call, not both zero:
 *       w_orig == 0:  v = w_den (x) y; the original lanes are not read, d_orig may be NULL;
 *       w_den == 0:   v = w_orig (x) x; the denoised lanes are not read, d_den may be NULL;
 *       otherwise:    v = (w_orig (x) x) (+) (w_den (x) y),
 *   (x) and (+) single f32 operations, each rounded to nearest even, never contracted into an fma: numpy's float32 arithmetic
 *   is the exact model.  A zero weight never meets an infinity.  (1, 0) is the aligned original, (1, -1) the residual,
 *   (1 - W, W) a wet/dry mix.
 * - v is converted and interleaved exactly as fvad_egress converts an f32 lane sample: its bits, PCM16 or PCM24 by the rules
 *   above.  A NaN input gives a NaN in an f32 file (the payload is not promised) and the minimum in a PCM file.
 * - INVARIANTS, all bit for bit.  No byte outside [byte_offset, byte_offset + n_frames * n_channels * bytes per sample) of a
 *   sink is written; no denoised sample outside [src_offset, src_offset + n_frames) and no original sample outside
 *   [orig_offset, orig_offset + n_frames - min(orig_zeros, n_frames)) of its lanes is read.  The output does not depend on the
 *   order of the sinks, on how a file is cut into sinks or calls, on ingest_ring_bytes, on the call form (device bytes or host
 *   bytes), or on the alignment of any of the three sides.  No atomics.  With w_orig = 0, w_den = 1 and no NaN in the lanes
 *   the bytes are fvad_egress's.
 *
 * fvad_egress_mix_check (host only, csrc/host_egress_mix.cpp): every argument rule of the two calls below, in this order:
 *   FVAD_ERR_INVALID_ARGUMENT for a weight that is not finite, two zero weights, a src_format other than FVAD_INGEST_F32;
 *   n_sinks == 0 succeeds here; NULL sinks, a stride smaller than its length with several lanes (of a source whose weight is
 *   not zero); then per sink FVAD_ERR_INVALID_ARGUMENT for a bad format, n_channels outside 1 .. 64; then per sink
 *   FVAD_ERR_OUT_OF_RANGE for lanes past n_lanes, src_offset + n_frames > den_samples (only when w_den != 0), orig_offset +
 *   (n_frames - min(orig_zeros, n_frames)) > orig_samples (only when w_orig != 0), byte_offset + bytes > out_bytes (all sums
 *   checked for 64-bit overflow); then FVAD_ERR_INVALID_ARGUMENT when two sinks' byte ranges overlap (ranges that touch are
 *   fine).  A sink with n_frames == 0 writes nothing.
 * fvad_egress_mix_device / fvad_egress_mix: fvad_egress_device's and fvad_egress's forms.  Both run the check (and refuse a NULL
 *   output, and lanes of a source whose weight is not zero that are NULL or not aligned to 4 bytes) before any launch, return when
 *   the bytes are written and name `egress_mix` in fvad_ctx_kernel_times (one launch per file format present, fewer than 2^24
 *   tiles each).  The host form goes through the ring fvad_ingest and fvad_egress use and cuts a sink at multiples of 4 frames:
 *   the piece from frame k on is the sink with src_offset + k, orig_zeros - min(orig_zeros, k) and orig_offset + k -
 *   min(orig_zeros, k), so the bytes cannot depend on the cut. */
#define FVAD_EGRESS_MIX_FIELDS 8
int fvad_egress_mix_check(const uint64_t *sinks, size_t n_sinks, uint64_t out_bytes, int src_format, float w_orig, float w_den,
                          size_t n_lanes, size_t orig_stride, size_t orig_samples, size_t den_stride, size_t den_samples);
int fvad_egress_mix_device(fvad_ctx *ctx, const void *d_orig, size_t orig_stride, size_t orig_samples, const void *d_den,
                           size_t den_stride, size_t den_samples, int src_format, size_t n_lanes, float w_orig, float w_den,
                           const uint64_t *sinks, size_t n_sinks, void *d_out, uint64_t out_bytes);
int fvad_egress_mix(fvad_ctx *ctx, const void *d_orig, size_t orig_stride, size_t orig_samples, const void *d_den,
                    size_t den_stride, size_t den_samples, int src_format, size_t n_lanes, float w_orig, float w_den,
                    const uint64_t *sinks, size_t n_sinks, void *const *dst_host);

/* ------------------------------------------------------------------ Evaluator (host)
 * src/Evaluator.zig:90-156 + src/Evaluator/statistics.zig */
typedef struct {
    float total_positives_sec, true_positives_sec, false_positives_sec, false_negatives_sec;
    float true_positive_rate, false_negative_rate, false_discovery_rate, precision;
    float fm_index, f_score, f_score_beta;
} fvad_single_stats;                          /* statistics.SingleStats :8-37 */
typedef struct { float overall, min, max, avg; } fvad_agg_stat;          /* :39-44 */
typedef struct {
    float total_positives_sec, true_positives_sec, false_positives_sec, false_negatives_sec;
    fvad_agg_stat true_positive_rate, false_negative_rate, false_discovery_rate, precision;
    float fm_index, f_score, f_score_beta;
} fvad_aggregate_stats;                       /* statistics.AggregateStats :46-75 */
typedef struct {
    float ignore_shorter_than_sec, extrude_start, extrude_end, fill_gaps;
} fvad_stat_config;                           /* statistics.StatConfig :77-83 */
typedef struct { float from_sec, to_sec; } fvad_segment_sec;

/* SimulationInstance.storeResult's sample->second conversion (SimulationInstance.zig:237-238) */
fvad_segment_sec fvad_segment_to_sec(const fvad_speech_segment *s, size_t sample_rate);
/* Evaluator.initAndRun + statistics.fromEvaluator */
int fvad_stats_from_segments(const fvad_segment_sec *vad, size_t n_vad,
                             const fvad_segment_sec *ref, size_t n_ref,
                             const fvad_stat_config *cfg, fvad_single_stats *out);
/* statistics.aggregate(stats)  statistics.zig:116-172 -- in slice order */
int fvad_stats_aggregate(const fvad_single_stats *stats, size_t n, fvad_aggregate_stats *out);

/* ---- scoring a VAD batch (fvad_vad_batch_create or _create_sweep): the statistics of every (stream, config) machine against
 * its stream's labels, fvad_single_stats machine by machine, each bit for bit fvad_stats_from_segments of the machine's
 * fvad_segment_to_sec-converted segments and the stream's labels.
 * fvad_vad_batch_set_references: stream s's labels are refs[ref_offsets[s] .. ref_offsets[s + 1]) (ref_offsets has
 * n_streams + 1 entries, ref_offsets[0] == 0, non-decreasing); the batch keeps its own copy, stably sorted by start
 * (Evaluator.initAndRun).  stat_cfgs has one fvad_stat_config per config.  NULL arguments, bad offsets or a NaN label:
 * FVAD_ERR_INVALID_ARGUMENT.  Once references are set, fvad_vad_batch_run_device also scores every machine on the device
 * (csrc/kernels_eval.hip) after its last launch; without references it does not score.
 * fvad_vad_batch_score scores the segments in b on n_threads host threads (FVAD_ERR_INVALID_ARGUMENT without references
 * or segments).  fvad_vad_batch_config_stats: config `config`'s stats of every stream (out has n_streams entries) from the
 * last scoring, host or device; FVAD_ERR_INVALID_ARGUMENT if the segments in b have not been scored.
 * fvad_vad_batch_set_keep_segments(b, 0): fvad_vad_batch_run_device leaves the segments on the device (counts, audits,
 * lazy statistics and scores still come back); until a run keeps segments again, fvad_vad_batch_segments and
 * _config_segments return FVAD_ERR_INVALID_ARGUMENT and fvad_vad_batch_total_segments returns SIZE_MAX.  Default 1. */
int fvad_vad_batch_set_references(fvad_vad_batch *b, const fvad_segment_sec *refs, const size_t *ref_offsets,
                                  const fvad_stat_config *stat_cfgs);
int fvad_vad_batch_set_keep_segments(fvad_vad_batch *b, int keep);
int fvad_vad_batch_score(fvad_vad_batch *b, int n_threads);
int fvad_vad_batch_config_stats(const fvad_vad_batch *b, size_t config, fvad_single_stats *out);
/* ---- multi-GPU: the plan's streams are dealt round-robin to one rank (process or thread) per GPU, nothing but
 * these per-stream statistics ever crosses GPUs.  Replaces the join of the reference's one-thread-per-file
 * instances (src/simulator.zig:221-232) in front of report_generator.zig:48-68: every rank hands in the
 * SingleStats of its streams, every rank receives all n_streams of them in PLAN order (stream id = index in
 * the plan), ready for fvad_stats_aggregate -- bit-identical to a single-process run.  Transport: one
 * ncclAllGather over RCCL / xGMI (RCCL is dlopen'ed on first use), behind a header all-gather of {n_streams, local
 * status}: n_streams must be the same on every rank, and a rank whose arguments are bad still takes part, so every
 * rank returns an error instead of some of them waiting in the collective.  Bootstrap like NCCL's own: rank 0 makes
 * the 128-byte id and hands it to the other ranks by whatever channel the host has (file, socket, env). */
#define FVAD_COMM_ID_BYTES 128
typedef struct fvad_comm fvad_comm;
int fvad_comm_unique_id(uint8_t *id, size_t n_bytes);                   /* ncclGetUniqueId */
int fvad_comm_create(fvad_ctx *ctx, const uint8_t *id, size_t n_bytes, int world, int rank,
                     fvad_comm **out);                                   /* ncclCommInitRank on ctx's device */
void fvad_comm_destroy(fvad_comm *c);
int fvad_comm_world(const fvad_comm *c);
int fvad_comm_rank(const fvad_comm *c);
int fvad_stats_allgather(fvad_comm *c, const uint32_t *local_ids, const fvad_single_stats *local_stats,
                         size_t n_local, size_t n_streams, fvad_single_stats *out /* [n_streams] */);
/* formats.parseAudacitySegments / serialize  (Evaluator/formats.zig:7-56) */
int fvad_parse_audacity(const char *txt, size_t len, fvad_segment_sec *out, size_t cap,
                        size_t *n);

/* ------------------------------------------------------------------ audio file input (host)
 * Minimal RIFF/WAVE reader standing in for AudioBuffer.loadFromFile / AudioFileStream
 * (src/audio_utils/AudioBuffer.zig:26-59, AudioFileStream.zig:18-102): PCM16 or float32, any
 * channel count, returned channel-planar f32.  Free with fvad_wav_free. */
int fvad_wav_read(const char *path, float ***channel_pcm, size_t *n_channels, size_t *n_frames,
                  size_t *sample_rate);
void fvad_wav_free(float **channel_pcm, size_t n_channels);
/* The same for a PCM16 file without the conversion: channel-planar int16 for fvad_lane.pcm_i16
 * (FVAD_ERR_MODEL_FORMAT if the file is not PCM16).  Free with fvad_wav_free_i16. */
int fvad_wav_read_i16(const char *path, int16_t ***channel_pcm, size_t *n_channels, size_t *n_frames,
                      size_t *sample_rate);
void fvad_wav_free_i16(int16_t **channel_pcm, size_t n_channels);
/* AudioBuffer.saveToFile (src/audio_utils/AudioBuffer.zig:61-118) for the WAV container -- what a recording
 * callback does with its clip (main.zig saves them): planar channels -> float32 (as_pcm16 == 0) or PCM16 WAV. */
int fvad_wav_write(const char *path, const float *const *channel_pcm, size_t n_channels,
                   size_t n_frames, size_t sample_rate, int as_pcm16);
/* The same for samples that already are PCM16 (clips packed by fvad_clips_export as FVAD_CLIP_PCM16, whose rule is not
 * libsndfile's): written as they are, so that fvad_wav_read_i16 returns them. */
int fvad_wav_write_i16(const char *path, const int16_t *const *channel_pcm, size_t n_channels, size_t n_frames,
                       size_t sample_rate);

#ifdef __cplusplus
}
#endif
#endif /* FVAD_H */
