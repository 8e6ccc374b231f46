// kernels.h -- launch wrappers of the gfx950 kernels (internal; the public ABI is include/fvad.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/fvad.h"
#include "feature_frames.h"

enum { FVAD_ACT_NONE = 0, FVAD_ACT_RELU = 1, FVAD_ACT_SIGMOID = 2 };

// ------------------------------------------------------------------ geometry (NSNet2.zig:12-16)
constexpr int kNFft = 320;
constexpr int kNHop = 160;
constexpr int kFramesPerChunk = 50;
constexpr int kWarmupRows = 4;                 // artifact_mitigation_window
constexpr int kRowsPerChunk = kFramesPerChunk + kWarmupRows; // 54
constexpr int kNBins = 161;
constexpr int kFeatStride = 176;               // 161 padded to 11 x 16 (zero-filled tail)
constexpr int kDown = 3;                       // 48 kHz -> 16 kHz
constexpr int kChunk48 = kFramesPerChunk * kNHop * kDown; // 24000
constexpr int kVadFft = 1024;               // VADPipeline.Config.fft_size default (VADPipeline.zig:21)
constexpr int kVadFftMax = 16384;           // any even size up to this: 512 / 1024 / 2048 on the wavefront FFT, the others on the generic kernel

// cross-call carry of one lane (all device floats); mirrors NSNet2.zig:27-33 state
struct LaneCarry {
    float in_tail[kNHop * kDown];          // last 480 raw 48 kHz samples (-> audio_input[0..160])
    float feat_tail[kWarmupRows * kNBins]; // features rows 50..53 of the previous chunk
    float ola_tail[kNHop];                 // audio_output[8000..8160)
    float last_sample;                     // resample carry
    float pad[3];
};

// one 0.5 s chunk of one lane inside a launch
struct ChunkDesc {
    const float* in;    // 24000 samples of this chunk (device)
    float* den;         // 24000 denoised samples out (device)
    const LaneCarry* carry_in; // read by the lane's first chunk of a launch (never null)
    LaneCarry* carry_out;      // written by the lane's last chunk of a launch (!= carry_in)
    uint32_t first;     // first chunk of its lane in this launch -> history comes from carry_in
    uint32_t last;      // last chunk of its lane in this launch -> writes carry_out
    float* rms;         // where this chunk's RMS goes (device), or null
    // 16-bit transport (optional): when in16 != null the chunk's samples are PCM16 and K1 converts them while
    // loading, x = (float)s * (1 / 32768) -- the decode of AudioFileStream.zig:56-102 / host_io.cpp, exact in
    // f32 -- so a 48 kHz stream crosses PCIe and HBM at 2 bytes per sample; den16 != null: K3 also writes the
    // denoised chunk as PCM16, rint(clamp(y * 32768, -32768, 32767))
    const int16_t* in16;
    int16_t* den16;
};

// one lane's worth of 1024-sample frames for K4
struct VadFftJob {
    const float* den;   // first frame's first sample (device, 8-byte aligned)
    float* band_sum;    // [n_frames]
    float* bins;        // [n_frames][n_fft/2 + 1] or null
    long n_frames;
};

// constant tables (device), built on the host in double like kissfft does and rounded once
struct FftTables {
    const float* win320;     // sqrt-Hann, NSNet2.zig:384-396
    const float* win320n;    // win320 * (1/320)  (NSNet2.zig:323,335)
    const float* tw160;      // [160][2] exp(-2 pi i j / 160)
    const float* st320;      // [80][2]  exp(-i pi ((k+1)/160 + 1/2))  real-FFT un-mixing
};

// tables of the VAD-side real FFT of n = 512 / 1024 / 2048 samples (device), built like FftTables
struct VadFftPlan {
    int n;
    const float* win;        // periodic Hann, window_fn.zig:22-28
    const float* tw;         // [n/2][2] exp(-2 pi i j / (n/2))
    const float* st;         // [n/4][2] real-FFT un-mixing
    float norm;              // windowNormFactor / n, BufferedFFT.zig:99
    // any other even size (FFT.init takes whatever kissfft factors, FFT.zig:35-60): the generic mixed-radix kernel, one
    // workgroup per frame, Stockham passes over the radices of n / 2 (4s first, then 2, 3, 5, ... like kissfft's kf_factor)
    int generic;             // 0: one of the wavefront sizes (512 / 1024 / 2048)
    int n_fac;
    int fac[14];
};

int fvad_launch_panel_gemm(const float* A, int lda, const float* Wfrag, const float* bias, float* C,
                           int ldc, long rows, int nt, int n_blocks, int S_steps, int act,
                           int map_T, int map_skip, hipStream_t stream, int n_valid_tiles = 0,
                           const unsigned* guard = nullptr);
// rows of a small-batch GEMM launch (panel_gemm_s_kernel): n_rows compact rows in ceil(n_rows / 64) panels; L > 0: compact row
// r = seq * L + tt is A's row seq * in_T + in_t0 + tt and C's row seq * out_T + out_t0 + tt (steps [t0, t0 + L) of every
// sequence); L == 0: rows as they are
struct GemmRowMap {
    int n_rows = 0, L = 0, in_T = 0, in_t0 = 0, out_T = 0, out_t0 = 0;
};
int fvad_launch_panel_gemm_s_rows(const float* A, int lda, const float* Wfrag, const float* bias, float* C, int ldc,
                                  GemmRowMap rm, int nt, int n_blocks, int S_steps, int act, hipStream_t stream,
                                  int n_valid_tiles = 0, const unsigned* guard = nullptr);
// small batches (kernels_nn.hip: panel_gemm_s_kernel): nt = 2 or 4 tiles per column block, S_steps in {11, 25, 38}
int fvad_launch_panel_gemm_s(const float* A, int lda, const float* Wfrag, const float* bias, float* C, int ldc,
                             long rows, int nt, int n_blocks, int S_steps, int act, int map_T, int map_skip,
                             hipStream_t stream, int n_valid_tiles = 0, const unsigned* guard = nullptr);
// rows of A and C of a panel_gemm3 launch: compact row i = qd * per + tt (qd < n_q) is row qd * T + skip + tt of both; the
// rows that pad the launch to whole 256-row panels repeat rows of qd = n_q - 1
struct Gemm3RowMap {
    int per = 0, T = 0, skip = 0;
    long n_q = 0;
};
int fvad_launch_panel_gemm3(const float* A, int lda, const float* Wfrag, const float* bias, float* C,
                            int ldc, long rows, int nt, int n_blocks, int S_steps, int K, int act,
                            int n_valid_tiles, int map_T, int map_skip, int n_wg, hipStream_t stream, bool trim_tiles = false,
                            const Gemm3RowMap* cmap = nullptr);
// f16x3 form (kernels_h3.hip): Wfrag from pack_panel_h3, K = true reduction length, sx / sw = input / weight scales.
// in_ts: A in the split tiled layout (a_ld = K-steps per row tile) or row-major f32 [sequence][seq_T][a_ld];
// out: 0 row-major f32, 1 tiled f32 (c_ld unit tiles per row tile), 2 split tiled (c_ld K-steps, scaled by out_sx);
// row_tiles = output row tiles of 16 rows
int fvad_launch_panel_gemm_h3(const float* A, int in_ts, int a_ld, const float* Wfrag, const float* bias, float* C,
                              int out, int c_ld, int seq_T, long row_tiles, int nt, int n_blocks, int K, int act,
                              int n_valid_tiles, int map_T, int map_skip, float sx, float sw, float out_sx, int n_wg,
                              hipStream_t stream);
// gi: tiled f32; hsplit: h as split fragments (13 K-steps per row tile), the only form h exists in
int fvad_launch_gru_rec_h3(const float* gi, const float* Rfrag, const float* bR, float* hsplit,
                           long n_seq_pad, int T, int waves, float sx, float sw, hipStream_t stream);
// guard != nullptr: the kernel returns at once unless *guard != 0 (fallback behind fvad_launch_gru_ws)
// tile_major: gi rows are [25 J][3 gates][16] (large-batch GEMM) instead of [3 gates][400] (small-batch GEMM)
// the pipelined recurrence's whole fallback + pass count + reset of the polled words in one launch (kernels_nn.hip)
// feat != nullptr: gi does not hold layer 1's input projection yet (the pipelined kernel computed it in-kernel): the fallback
// computes it first from feat, W1frag_nt2 (the small-batch GEMM's 2-tile column blocks of W') and bG1 (tile-major)
int fvad_launch_gru_ws2_fallback(float* gi, const float* feat, const float* W1frag_nt2, const float* bG1, const float* R1frag, const float* bR1,
                                 const float* W2frag_nt2, const float* bW2, const float* R2frag, const float* bR2, float* h1, float* h2,
                                 long n_seq_pad, int T, unsigned* sync, unsigned long long* fallbacks, hipStream_t stream,
                                 int zero_at = 0, int zero_n = 0); // sync[zero_at, zero_at + zero_n): more words the last workgroup zeroes for the next pass
int fvad_launch_gru_lat(const float* gi, const float* R2frag, const float* bR, float* hout,
                        long n_seq_pad, int T, const unsigned* guard, int tile_major, hipStream_t stream, int row_tiles = 1);
// small batches: recurrent weights stationary in registers across 25 x G workgroups, h exchanged per step
// (kernels_ws.hip).  hx: fvad_gru_ws_exchange_floats(n_seq_pad) floats; flags: 256 zeroed words per launch;
// err: one zeroed word shared by the launches of a network pass.  Returns -1 when the batch is too large.
void fvad_launch_zero_words(unsigned* p, int n, hipStream_t stream);
// *counter += (*word != 0): how the context counts the network passes in which gru_ws gave up (a kernel node, so it
// also works inside a captured graph)
void fvad_launch_count_word(unsigned long long* counter, const unsigned* word, hipStream_t stream);
bool fvad_gru_ws_shape(long n_seq_pad, int n_cu, int* RT, int* G);
size_t fvad_gru_ws_exchange_floats(long n_seq_pad);
int fvad_launch_gru_ws(const float* gi, const float* R2frag, const float* bR, float* hout, float* hx, unsigned* flags,
                       unsigned* err, long n_seq_pad, int T, int n_cu, int tile_major, unsigned long long spin_ticks,
                       hipStream_t stream);
// any hidden size (16 J padded units, J <= 64): gi rows of gi_ld floats with gate g of unit tile j at g * 16 J + 16 j,
// bR [3][16 J], R2frag = pack_gru_r2 of the padded matrix, hout rows of h_ld floats
// both GRU layers in one launch, pipelined layer over layer (kernels_ws.hip gru_ws2_kernel): gi1 tile-major rows
// (layer 1's input projection), W2frag = pack_gru_r2 of layer 2's input weights, bW2 = its bias Wb [3][400];
// hx: fvad_gru_ws2_exchange_floats floats; flags: 512 zeroed words; returns -1 when the batch does not fit
bool fvad_gru_ws2_shape(long n_seq_pad, int n_cu, int* RT, int* G);
size_t fvad_gru_ws2_exchange_floats(long n_seq_pad);
// One row tile per group (up to 96 sequences): the 16-wavefront kernel, which computes layer 1's input projection itself from
// feat (rows of kFeatStride floats), W1frag = pack_gru_frag of W' = W_ih W_fc1 and bG1 = its bias, tile-major -- gi1 is not
// read and the GEMM in front is not needed (fvad_gru_ws2_gi1_in_kernel says which case a launch is)
bool fvad_gru_ws2_gi1_in_kernel(long n_seq_pad, int T, int n_cu, int variant);
// whether any of the pipelined kernels takes a launch of this shape (gru_ws2k: one row tile per group; gru_ws2m: 2..16 row tiles
// per group; gru_ws2: the 8-wavefront form, up to 4, which ws2_variant bit 8 forces) and the name of the one that does
bool fvad_gru_ws2_ok(long n_seq_pad, int T, int n_cu, int variant);
const char* fvad_gru_ws2_kernel_name(long n_seq_pad, int T, int n_cu, int variant);
int fvad_launch_gru_ws2(const float* gi1, const float* feat, const float* W1frag, const float* bG1, const float* R1frag, const float* bR1,
                        const float* W2frag, const float* bW2, const float* R2frag, const float* bR2, float* hout2, float* hx,
                        unsigned* flags, unsigned* err, long n_seq_pad, int T, int n_cu, unsigned long long spin_ticks, int variant,
                        unsigned waits, hipStream_t stream, unsigned* lsync = nullptr); // waits: gru_ws2k's first-poll waits (layer 1 | layer 2 << 16, 10 ns ticks); 0 = built in
// lsync: kWs2LocalWords zeroed words (layer 1's XCD-local flags and the placement tickets): gru_ws2k's layer 1 exchanges h1 inside
// one XCD where fvad_gru_ws2_local_layer1 says the launch's shape allows it
constexpr int kWs2LocalWords = 336;
bool fvad_gru_ws2_local_layer1(long n_seq_pad, int T, int n_cu, int variant);
// which table of built-in first-poll waits gru_ws2k uses for this launch: 0 not that kernel, 1 groups of 25 + 25, 2 groups of 13 + 25,
// 3 groups of 13 + 25 with layer 1's input projection in the kernel (what ws2_calibrate measures and overrides)
int fvad_gru_ws2_wait_class(long n_seq_pad, int T, int n_cu, int variant);
unsigned fvad_gru_ws2_builtin_waits(int wait_class, bool local_layer1 = false); // the table's entry, packed like `waits` (local_layer1: the table of launches whose layer 1 exchanges inside one XCD)
int fvad_launch_gru_gen(const float* gi, int gi_ld, const float* R2frag, const float* bR, float* hout, int h_ld,
                        long n_seq_pad, int T, int J, hipStream_t stream);
int fvad_launch_gru_rec3(const float* gi, const float* R2frag, const float* bR, float* hout,
                         long n_seq_pad, int T, int waves, hipStream_t stream, float* hs3 = nullptr,
                         const ChunkDesc* first_of = nullptr, long n_real = 0);
// bf16x3 form of the dense layers (kernels_b3.hip): Wfrag from pack_panel_b3, K = true reduction length.
// in_ts: A in the three-piece tiled layout TS3 (a_ld = K-steps per row tile) or row-major f32 [sequence][seq_T][a_ld];
// out: 0 row-major f32 [sequence][seq_T][c_ld], 2 TS3 (c_ld K-steps per row tile); row_tiles = output row tiles of 16 rows
int fvad_launch_panel_gemm_b3(const float* A, int in_ts, int a_ld, const float* Wfrag, const float* bias, float* C,
                              int out, int c_ld, int seq_T, long row_tiles, int nt, int n_blocks, int K, int act,
                              int n_valid_tiles, int map_T, int map_skip, int n_wg, hipStream_t stream);

// K1: per chunk: RMS, decimate, STFT-320, log-power features (+ warm-up rows)
// (parts: 1, or 2 / 3 to cut a chunk's frames over several workgroups in launches of a few chunks; same bits)
void fvad_launch_stft(const ChunkDesc* descs, int n_chunks, FftTables tb, float* feat,
                      float* spec, hipStream_t stream, int parts = 1);
// K3: per chunk: gain, inverse STFT, overlap-add, x3 upsample
void fvad_launch_istft(const ChunkDesc* descs, int n_chunks, FftTables tb, const float* spec,
                       const float* gains, int gains_rows_per_chunk, int gains_row0,
                       hipStream_t stream, int parts = 1);
// K4: n-point periodic-Hann rFFT magnitude + band sum over [min_bin, max_bin], n = pl.n
void fvad_launch_vadfft(const float* den, long n_frames, VadFftPlan pl, int min_bin, int max_bin,
                        float* band_sum, float* bins_or_null, hipStream_t stream);
// all lanes in one launch: jobs is a device array of n_jobs entries, max_frames = max n_frames
// any_bins: some job has a `bins` tap (the full-spectrum kernel must run; band sums come from the band kernel either way);
// plain_loads: the band kernel stages its frames with plain 8-byte loads, the path of unaligned jobs (context option k4_plain_loads)
// (returns a hipError_t as int: a failed hipFuncSetAttribute must not leave the caller with stale band sums and FVAD_OK)
int fvad_launch_vadfft_jobs(const VadFftJob* jobs, int n_jobs, long max_frames, VadFftPlan pl,
                            int min_bin, int max_bin, hipStream_t stream, int any_bins, int n_cu, int plain_loads = 0);
// K4 with several bands per pass (fvad_engine_band_sums_device): band b of the set is bins lo[b]..hi[b], written for a job's frame f at
// job.band_sum + idx[b] * step + f; per band the bits of fvad_launch_vadfft_jobs with that band.  pruned: every band of the set lies
// inside bins 1..47 at 1024 points (vadfft1024_band_kernel's pass, where the single-band launch takes those bands' bits); else the
// full-spectrum kernel of the size (512 / 1024 / 2048) or the generic one
constexpr int kVadBandsPerLaunch = 256;
struct VadBandSet {
    long step;
    int n;
    int16_t lo[kVadBandsPerLaunch], hi[kVadBandsPerLaunch];
    int32_t idx[kVadBandsPerLaunch];
};
int fvad_launch_vadfft_bands(const VadFftJob* jobs, int n_jobs, long max_frames, VadFftPlan pl, const VadBandSet& bs, int pruned,
                             hipStream_t stream, int n_cu, int plain_loads = 0); // hipError_t as int
// batched FFT.fft for B3 / BASELINE config 2: n_fft in {320, 512, 1024, 2048} (pl is used for n_fft != 320)
int fvad_launch_rfft_batch(const float* frames, long n_frames, int n_fft, const float* window,
                           FftTables tb, VadFftPlan pl, float* bins_or_null, float* mag_or_null,
                           hipStream_t stream); // hipError_t as int
void fvad_launch_irfft_batch(const float* bins, long n_frames, FftTables tb, float* out,
                             hipStream_t stream);
// FFT.invFft for any even size (pl.generic plans; tables of the FORWARD transform, conjugated in the kernel): bins
// [n_frames][n/2 + 1][2] -> out [n_frames][n], unscaled like kiss_fftri
int fvad_launch_irfft_generic(const float* bins, long n_frames, VadFftPlan pl, float* out, hipStream_t stream); // hipError_t as int

// ------------------------------------------------------------------ VAD machines of a parameter sweep (kernels_vad.hip)
namespace fvad { struct VadMachineCfg; struct VadLaneState; } // vad_machine.h
struct VadAvgKey;
struct VadTrigKey;
struct VadMachinesArgs {
    const fvad::VadMachineCfg* cfgs; // [n_configs] (device), with their bands
    int n_configs, n_channels;
    long n_streams;
    int by_config;             // lane mapping: 0 = a stream's configs side by side, 1 = a config's streams side by side
    long n_machines;           // n_streams * n_configs, machine = stream * n_configs + config
    long n_lanes;              // n_streams * n_channels
    const float* band;         // band j of lane l at band + (j * n_lanes + l) * band_stride
    long band_stride;
    const float* ratio;        // stream s's frame ratios at ratio + s * ratio_stride (NaN: none)
    long ratio_stride;
    const long* n_frames;      // [n_streams] (device)
    uint64_t fft_size;
    float* lt_rings;           // [(max long_len rounded up to 64) / 4 + 16][n_machines][4]
    float* rings;              // [st_max + cr_max][n_machines] when !rings_in_lds
    int rings_in_lds, st_max, cr_max;
    fvad_speech_segment* segs; // [n_machines][seg_cap]
    uint32_t seg_cap;
    uint32_t* seg_count;       // [n_machines]: segments the machine closed (may exceed seg_cap: then only seg_cap were written)
    fvad_vad_audit* audits;    // [n_machines]
    unsigned long long* stats; // [n_machines][2]: exact evaluations of the long-term chain, lazy pushes
    // ---- the resume form (resume = 1, fvad_vad_batch_run_device_part): every machine's state lives on between launches in
    // state[machine]; the short-term and channel-ratio rings in `rings` (copied into LDS and back when rings_in_lds); frames
    // [first_frame, first_frame + n_frames[s]) of the stream, band / ratio from the part's first frame.  A machine whose
    // segment room (seg_cap past its seg_base) is full before its last frame stops there and sets *paused: the next launch
    // with fresh = 0 goes on from that frame.  rebase: seg_base = the machine's segment count on entry (segments are written
    // at seg[count - seg_base]); else seg_base is kept.
    // coop = 1 (context option vad_chain "coop", any of the forms): the exact long-term chains by the whole wavefront, the same bits
    int resume, fresh, rebase, coop;
    uint64_t first_frame;
    fvad::VadLaneState* state;  // [n_machines], machine = stream * n_configs + config
    unsigned* paused;
    // ---- several frame sizes in one launch (sized = 1, fvad_vad_batch_create_sweep_sized): config c runs on frames of
    // sizes[size_of[c]] samples; then n_frames is [n_sizes][n_streams] (size g, stream s at g * n_streams + s), the frame
    // ratios of (g, s) at ratio + (g * n_streams + s) * ratio_stride, and frame k of a machine is at sample
    // first_sample + k * F (fft_size and first_frame unused; a machine's next_frame counts frames of its own size).
    // lane_config (by stream, may be null): lane j of a stream's n_configs runs config lane_config[j]
    int sized;
    const uint64_t* sizes;      // [n_sizes] (device)
    const uint32_t* size_of;    // [n_configs] (device)
    const int* lane_config;     // [n_configs] (device)
    uint64_t first_sample;
    // ---- the table form (table = 1 with coop = 1; context option vad_avgs "table"): the short-term and channel-ratio averages
    // of every frame of the part come from the tables fvad_launch_vad_avgs filled (VadAvgsArgs below: the same pointers), the
    // frame's min_volume from minvol; the machine pushes no short ring.  A launch that stores state (resume = 1) leaves in
    // `rings` and state[] what the ring form would have left, bit for bit
    int table;
    const float* minvol;        // [n_bands][n_streams][minvol_stride]
    long minvol_stride;
    const double* st_tab;       // key j's average of (stream s, frame k of the part) at tab[key.base + (s * tab_frames[key.size] + k) * key.nk]
    const double* cr_tab;
    const VadAvgKey* st_keys;   // (VadAvgKey: below, with the tables' kernels)
    const VadAvgKey* cr_keys;
    const uint32_t* st_key;     // [n_configs] (device): each config's short key, ratio key
    const uint32_t* cr_key;
    const long* tab_frames;     // [n_sizes] (device): the frames of a stream's table rows, per size
    // ---- the shared-trigger form (context option vad_trigger "shared", vad_finish.h).  emit = 1 (with coop = 1): a machine runs
    // its trigger as ever but, in place of the state machine, shifts each frame's threshold_met into 64-bit words -- bit k % 64 of
    // word k / 64 is frame k of the part, the last word's upper bits zero; it writes no segment, never pauses for room and
    // leaves seg_count 0.  Config c of the launch is trigger machine c: its word w of stream s at
    // bits[trig_keys[c].base + (s * trig_keys[c].words + w) * trig_keys[c].nk] (per size [stream][word][machines of that size]).
    // fvad_launch_vad_finish reads the same words: its config c's are those of trigger machine trig_of[c].
    int emit;
    unsigned long long* bits;
    const VadTrigKey* trig_keys; // [trigger machines] (device)
    const uint32_t* trig_of;            // [n_configs] (device), the finishing launch only
};
struct VadTrigKey {
    long base;       // the machine's word 0 of stream 0
    uint32_t nk;     // trigger machines of its size (the stride between two words)
    uint32_t words;  // words of a stream's row at its size
};
int fvad_launch_vad_machines(const VadMachinesArgs& a, hipStream_t stream); // hipError_t as int
// The finishing kernel of the shared-trigger form (kernels_vadfinish.hip): one lane per (stream, config), a stream's configs in
// lane_config's order (may be null); it walks the part's bits (vad_finish.h) from state[machine].next_frame on with the resume
// form's segment protocol (seg_cap, seg_base, rebase, paused, next_frame, seg_count) and reads of `a` only cfgs, the counts,
// ratio, n_frames, fft_size / first_frame or sizes / size_of / first_sample, segs, seg_count, state, paused, fresh, rebase,
// lane_config, bits, trig_keys and trig_of.  Of state[machine] only m's state-machine fields, n_segs, seg_base and next_frame
// are read and written.
int fvad_launch_vad_finish(const VadMachinesArgs& a, hipStream_t stream); // hipError_t as int

// ------------------------------------------------------------------ the averages' tables of a part (kernels_vadavgs.hip, vad_avgs.h)
// A short key is (band, short_len), a ratio key (size, ratio_len): every config with the same key has the same average in every
// frame.  Per size the table is [stream][frame][keys of that size], so that a wavefront of one stream's configs reads a frame's
// averages from a few lines.
struct VadAvgKey {
    uint32_t src;     // short key: the band block; ratio key: the size index
    uint32_t len;     // the ring's length
    uint32_t size;    // the size index of the key's frame clock
    uint32_t nk;      // keys of that size in the table (the stride between two frames)
    long base;        // the key's entry of (stream 0, frame 0)
    long rep;         // the lane of a machine with this key: its place is rep * n_streams + s by config, s * n_configs + rep by stream
    double scalar;    // 1 / len as VadMachineCfg has it
};
struct VadAvgsArgs {
    const float* band;          // as VadMachinesArgs
    long band_stride, n_lanes;
    int n_channels, n_bands, n_sizes;
    long n_streams;
    const uint32_t* size_of_band; // [n_bands] (device); null with one size
    const long* n_frames;       // [n_sizes][n_streams] (device)
    long max_frames;            // the longest row of the part
    float* minvol;              // out: [n_bands][n_streams][minvol_stride]
    long minvol_stride;
    const float* ratio;         // row (size, stream) at ratio + row * ratio_stride
    long ratio_stride;
    const VadAvgKey* st_keys;   // (device)
    const VadAvgKey* cr_keys;
    int n_st_keys, n_cr_keys;
    double* st_tab;             // out
    double* cr_tab;
    const long* tab_frames;     // [n_sizes] (device)
    const uint64_t* first_frame; // [n_sizes] (device): the part's first frame in each size's frames
    int fresh;                  // no earlier frames: the homes are not read
    const float* rings;         // the rings' home [st_max + cr_max][n_machines] at the part's start
    int st_max, by_config, n_configs;
    long n_machines;
};
// the frame tile of vad_avgs_kernel and vad_minvol_kernel: frames per workgroup
constexpr int kAvgsTile = 256;
// (grid: frame tiles x streams x bands or keys -- the caller keeps streams, bands and keys at or below kAvgsGridMax)
constexpr long kAvgsGridMax = 65535;
int fvad_launch_vad_minvol(const VadAvgsArgs& a, hipStream_t stream); // hipError_t as int
int fvad_launch_vad_avgs(const VadAvgsArgs& a, hipStream_t stream);   // (after fvad_launch_vad_minvol on the same stream)

// ------------------------------------------------------------------ the frame ratios of a device part (kernels_vadratio.hip)
// row (size g, stream s) = g * n_streams + s: frames [0, n_frames[row]) of sizes[g] samples from sample first_sample on (a chunk
// boundary), ratio row at ratio + row * ratio_stride; frames [n_frames[row], max_frames) of the row are set to 0
struct VadRatioArgs {
    const float* chunk_rms;    // lane l = s * n_channels + c, chunk k of the part at chunk_rms[l * rms_stride + k] (device)
    long rms_stride;
    int n_channels, n_sizes;
    long n_streams;
    const uint64_t* sizes;     // [n_sizes] (device); null with one size: fft_size
    uint64_t fft_size;
    const long* n_frames;      // [n_sizes][n_streams] (device)
    const long* n_chunks;      // [n_streams] (device): the chunks of the part chunk_rms holds for the stream
    uint64_t chunk_size, first_sample;
    float* ratio;
    long ratio_stride, max_frames; // max_frames <= ratio_stride
};
int fvad_launch_vad_frame_ratios(const VadRatioArgs& a, hipStream_t stream); // hipError_t as int

// ------------------------------------------------------------------ scoring the machines of a VAD batch (kernels_eval.hip)
// one lane per machine, machine = stream * n_configs + config: the Evaluator statistics of its segments (eval_walk.h)
struct VadScoreArgs {
    const fvad_speech_segment* segs;      // [n_machines][seg_cap], as fvad_launch_vad_machines wrote them
    const uint32_t* seg_count;            // [n_machines] (counts above seg_cap are read as seg_cap)
    uint32_t seg_cap;
    long n_machines;
    int n_configs;
    float sample_rate_f;                  // (float)sample_rate
    const fvad_segment_sec* refs;         // every stream's labels, sorted by start
    const float* ref_pmax;                // prefix max of their ends, per stream
    const unsigned long long* ref_off;    // [n_streams + 1]
    const fvad_stat_config* stat_cfgs;    // [n_configs]
    fvad_single_stats* out;               // [n_machines]
};
int fvad_launch_vad_score(const VadScoreArgs& a, hipStream_t stream); // hipError_t as int

// ------------------------------------------------------------------ dropping configs from a batch between device parts (kernels_vadretain.hip)
// fvad_vad_batch_retain_configs: the resume-form state of the kept machines gathered into freshly allocated buffers of the smaller
// batch.  Places (a lane's rings, VadMachinesArgs' lane map) and machines (the outputs, stream * n_configs + config) are gathered
// through host-built maps new -> old; every index of the maps is < the old count.
struct VadRetainArgs {
    long n_places, old_places;        // new / old machine counts (places and machines are the same number)
    const long* place_src;            // [n_places]: the old place of new place p
    const long* machine_src;          // [n_places]: the old machine of new machine m
    const float4* lt_src;             // old long-term rings [old lt_rows][old_places] float4
    float4* lt_dst;                   // new [lt_rows][n_places] float4
    long lt_rows;                     // rows of the new allocation (<= the old one's)
    const float* rings_src;           // old [old_st + old_cr][old_places]
    float* rings_dst;                 // new [st + cr][n_places]
    int st, cr, old_st;               // new short-term / channel-ratio rows, the old short-term rows (the old cr rows follow them)
    const fvad::VadLaneState* state_src;
    fvad::VadLaneState* state_dst;
    const uint32_t* count_src;
    uint32_t* count_dst;
    const fvad_vad_audit* audit_src;
    fvad_vad_audit* audit_dst;
    const unsigned long long* stats_src; // [machine][2]
    unsigned long long* stats_dst;
    const fvad_speech_segment* segs_src; // [old machine][seg_cap]
    fvad_speech_segment* segs_dst;       // [machine][seg_cap]: min(count, seg_cap) of each
    uint32_t seg_cap;
};
int fvad_launch_vad_retain(const VadRetainArgs& a, hipStream_t stream); // hipError_t as int

// ------------------------------------------------------------------ the batch Recorder (kernels_clips.hip)
// fvad_clips_export*: a work unit is a tile of kClipTile samples of one (clip, channel).  Unit u of clip c is
// unit_prefix[c] + channel * n_tiles + tile (the partial sums have the units' order); the gather's tiles are counted by
// tile_prefix[c] + tile.
constexpr int kClipTile = 8192;
struct ClipJob {
    uint64_t src_off;    // elements from `src` to the clip's first sample in its first lane
    uint64_t len;        // samples
    uint64_t out_off;    // elements from `out` to the clip's slot (a multiple of 16 bytes)
    uint32_t first_unit; // == unit_prefix[c]
    uint32_t n_tiles, n_channels;
    uint32_t skip;       // the strided gathers' first kept sample (< step); 0 and unused everywhere else
};
struct ClipInfo {        // what fvad_clips_export* reports per clip
    int32_t best_channel;
    float best_rms, runner_up_rms;
    uint64_t out_offset;
};
struct ClipArgs {
    const void* src;     // f32 or PCM16 lanes
    void* out;
    uint64_t lane_stride;
    const ClipJob* jobs;           // [n_clips] (device)
    const uint32_t* unit_prefix;   // [n_clips + 1]
    const uint32_t* tile_prefix;   // [n_clips + 1]
    double* partials;              // [n_units]
    ClipInfo* infos;               // [n_clips]
    uint32_t n_clips, n_units, n_tiles;
    int src_i16, out_i16;
};

// The split-source form (fvad_clips_export_split*; staged by clip_source_device.h): a clip's channel ch is a_len samples at
// a + a_off + ch * a_stride followed by len - a_len samples at b + b_off + ch * b_stride, and is read as if it were one run.
// Units, tiles (counted from the clip's first sample), partials and infos are ClipArgs', and clip_pick_kernel runs on `c` as it
// is; c.src / c.lane_stride are piece A's, c.jobs[i].src_off is not used.
struct ClipSplit {
    uint64_t a_off, a_len, b_off, pad; // elements; a_len <= c.jobs[i].len
};
struct ClipSplitArgs {
    ClipArgs c;
    const void* b;
    uint64_t b_stride;
    const ClipSplit* splits; // [n_clips] (device)
};
// every launch of the Recorder: hipError_t as int, and one overload per source (B below is ClipArgs or ClipSplitArgs)
int fvad_launch_clip_rms(const ClipArgs& a, hipStream_t stream);
int fvad_launch_clip_rms(const ClipSplitArgs& a, hipStream_t stream);
int fvad_launch_clip_pick(const ClipArgs& a, hipStream_t stream);   // (after fvad_launch_clip_rms on the same stream; a split call's a.c)
int fvad_launch_clip_gather(const ClipArgs& a, hipStream_t stream); // (after fvad_launch_clip_pick)
int fvad_launch_clip_gather(const ClipSplitArgs& a, hipStream_t stream);

// The strided gathers (kernels_clips_strided.hip, fvad_clips_export*_strided): of the picked channel the samples skip,
// skip + step, ... of the clip (skip = jobs[i].skip < step), out_len = ceil((len - skip) / step) of them into the clip's slot.
// RMS and pick are the kernels above over every sample; only the gather differs.  Its tiles are counted in OUTPUT samples from
// the clip's first kept sample: tile k holds outputs [k * tile_out, ...), i.e. source samples from skip + k * tile_out * step,
// and c.tile_prefix / c.n_tiles count these tiles (the RMS units keep kClipTile and jobs[i].n_tiles).
constexpr uint32_t kClipStepMax = 16; // FVAD_CLIP_STEP_MAX
// floor(kClipTile / step) rounded down to a multiple of 8: a tile's first output is on a 16-byte boundary of its slot in
// either output format, and its (tile_out - 1) * step + 1 source samples fit stage_tile's LDS image
constexpr uint32_t clip_tile_out(uint32_t step) { return (uint32_t)kClipTile / step / 8 * 8; }
template <typename B> struct ClipStridedArgs {
    B s; // the source
    uint32_t step, tile_out;
};
int fvad_launch_clip_gather_strided(const ClipStridedArgs<ClipArgs>& a, hipStream_t stream); // (after fvad_launch_clip_pick)
int fvad_launch_clip_gather_strided(const ClipStridedArgs<ClipSplitArgs>& a, hipStream_t stream);

// The filtered gathers (kernels_clips_fir.hip, fvad_clips_export*_fir): output q of a clip is the FIR sum of n_taps taps over the
// picked channel's samples around c = skip + q * step, the clip zero-extended.  Tiles are counted in OUTPUT samples from the
// clip's first kept sample as the strided gathers' are, with a tile that leaves room for the filter's halo on both sides.
constexpr uint32_t kClipFirTapsMax = 513; // FVAD_CLIP_FIR_TAPS_MAX
// ((kClipTile - n_taps) / step + 1) rounded down to a multiple of 8: the (tile_out - 1) * step + n_taps source samples of a
// tile, halo and zero extension included, fit kClipTile
constexpr uint32_t clip_fir_tile_out(uint32_t step, uint32_t n_taps) { return (((uint32_t)kClipTile - n_taps) / step + 1) / 8 * 8; }
template <typename B> struct ClipFirArgs {
    B s;
    const float* taps;   // [n_taps] (device), branch by branch: taps[j], taps[j + step], ... for j = 0 .. step - 1
    uint32_t step, tile_out, n_taps, pad;
};
int fvad_launch_clip_gather_fir(const ClipFirArgs<ClipArgs>& a, hipStream_t stream); // (after fvad_launch_clip_pick)
int fvad_launch_clip_gather_fir(const ClipFirArgs<ClipSplitArgs>& a, hipStream_t stream);

// The resampling gathers (kernels_clips_resample.hip, fvad_clips_export*_resampled): output o of a clip is the polyphase sum
// sum_j table[j * up + o mod up] * x[q - j], q = (K + o * down) / up, over the picked channel's samples, the clip zero-extended;
// out_len = ceil(len * up / down).  Tiles are counted in OUTPUT samples from the clip's first output (tile_out of them, a
// multiple of 8: resampled_tile_out of clips_resample.h); a tile's window of at most kClipTile clip samples is staged once.
constexpr uint32_t kClipResampleTableLds = 6144; // table entries (24 KB) that are kept in LDS beside the window; a longer table stays in global memory
template <typename B> struct ClipResampleArgs {
    B s;
    const float* table;  // [ceil(n_taps / up) * up] (device): resample_table of resample.h
    uint32_t up, down, tile_out, n_taps;
};
int fvad_launch_clip_gather_resampled(const ClipResampleArgs<ClipArgs>& a, hipStream_t stream); // (after fvad_launch_clip_pick)
int fvad_launch_clip_gather_resampled(const ClipResampleArgs<ClipSplitArgs>& a, hipStream_t stream);

// The feature exports (kernels_clips_mel.hip), one argument struct for both families.  RMS and pick are the kernels above over
// every sample.  Of the picked channel's strided stream s[i] = sample skip + i * step (L of them) the frames t < T, a tile
// feat_tile_frames consecutive frames of one clip (feature_frames.h states L, T and the tile); c.tile_prefix / c.n_tiles count
// these tiles, c.out is f32 and jobs[i].out_off the clip's slot of [T][n_mels] floats.
// - log-mel (fvad_clips_export_mel*): frames of n_fft taps centred with reflection, as power spectrum -> mel bands -> log10;
//   tile_frames = feat_tile_frames(n_fft, hop), log_floor = log10(floor).  The fields from tile_sum on are not used.
// - Kaldi-style filter bank (fvad_clips_export_fbank*): of the stream times `scale` frames of `win` taps from t * hop on
//   (snip_edges: no tap outside the stream), each with its mean removed, pre-emphasised, windowed and zero-padded to pl.n, then
//   power spectrum -> bands -> ln; window [win], tile_frames = feat_tile_frames(win, hop), log_floor = ln(floor).  tile_max,
//   feat_max, the norm and fft400 are not used.
constexpr uint32_t kClipMelNfftMax = 2048;  // FVAD_CLIP_MEL_NFFT_MAX
constexpr uint32_t kClipMelBandsMax = 128;  // FVAD_CLIP_MEL_BANDS_MAX
static_assert(fvad::kFeatSrcTile == (uint32_t)kClipTile, "a feature tile's window is staged as a clip tile is");
struct ClipFeatArgs {
    ClipArgs c;
    VadFftPlan pl;         // n = n_fft: tw, st and the radices of the generic transform (win and norm are not used)
    const float* window;   // [n_fft] or [win] (device), the caller's
    const float* matrix_t; // [n_fft / 2 + 1][n_mels] (device): the caller's matrix transposed, so that lanes m read neighbours
    float* tile_max;       // [c.n_tiles]: a tile's largest feature
    float* feat_max;       // [c.n_clips]: a clip's largest feature (clip_mel_max)
    uint32_t step, hop, n_mels, tile_frames;
    float floor, log_floor; // the logarithm of the floor, evaluated on the host in double and rounded once
    float norm_range, norm_offset, norm_scale;
    int fft400;            // the eight-frames-per-wavefront transform (n_fft == 400 only)
    float* tile_sum;       // [c.n_tiles][n_mels]: a tile's features added over ascending t, band by band
    float* means;          // [c.n_clips][n_mels]: the tiles' sums added in tile order, over f32(T) (clip_fbank_mean)
    uint32_t win;
    float scale, preemph;
    int remove_dc;
};
int fvad_launch_clip_mel(const ClipFeatArgs& a, hipStream_t stream);        // (after fvad_launch_clip_pick)
int fvad_launch_clip_mel_max(const ClipFeatArgs& a, hipStream_t stream);    // (after fvad_launch_clip_mel)
int fvad_launch_clip_mel_norm(const ClipFeatArgs& a, hipStream_t stream);   // (after fvad_launch_clip_mel_max)
int fvad_launch_clip_fbank(const ClipFeatArgs& a, hipStream_t stream);      // (after fvad_launch_clip_pick)
int fvad_launch_clip_fbank_mean(const ClipFeatArgs& a, hipStream_t stream); // (after fvad_launch_clip_fbank)
int fvad_launch_clip_fbank_sub(const ClipFeatArgs& a, hipStream_t stream);  // (after fvad_launch_clip_fbank_mean)
// The split-source form (fvad_clips_export_split_mel*, _split_fbank*): f.c is the split call's ClipArgs (piece A's src and
// lane_stride), and stream sample i of a clip is clip sample e = skip + i * step, in piece A when e < a_len, else in piece B at
// e - a_len: the stride is counted from the clip's first sample and runs through the seam, as do the tiles and the frames.  Only
// the two tile kernels read samples; every other launch above serves a split call on `f` as it is.
struct ClipFeatSplitArgs {
    ClipFeatArgs f;
    const void* b;
    uint64_t b_stride;
    const ClipSplit* splits; // [f.c.n_clips] (device)
};
// the tile kernels' argument by source B
template <typename B> struct ClipFeatOf { using type = ClipFeatArgs; };
template <> struct ClipFeatOf<ClipSplitArgs> { using type = ClipFeatSplitArgs; };
int fvad_launch_clip_mel(const ClipFeatSplitArgs& a, hipStream_t stream);   // (after fvad_launch_clip_pick on a.f.c)
int fvad_launch_clip_fbank(const ClipFeatSplitArgs& a, hipStream_t stream); // (after fvad_launch_clip_pick on a.f.c)

// ------------------------------------------------------------------ device-side ingest (kernels_ingest.hip)
// fvad_ingest*: a work unit is a tile of one source -- kIngestTileBytes of its interleaved bytes rounded down to whole frames in
// multiples of 4 (tile_frames), every channel of them -- or, after the source's n_data_tiles, kIngestFillTile zeros of one lane
// of its fill range: unit r of job j is data tile r for r < n_data_tiles, else fill tile (r - n_data_tiles) % n_fill_tiles of
// channel (r - n_data_tiles) / n_fill_tiles.  A launch serves the jobs of ONE source format; unit_prefix[j] counts the units
// in front of job j (a job has at least one unit).
constexpr int kIngestTileBytes = 16384;
constexpr int kIngestFillTile = 8192;
constexpr int kIngestMaxChannels = 64;
struct IngestJob {
    uint64_t src_off;   // bytes from `raw` to the source's frame 0
    uint64_t n_frames;
    uint64_t dst_off;   // elements from `lanes` to the sample frame 0 of channel 0 is written to
    uint64_t fill_len;  // zeros behind the frames, in every lane of the source
    uint32_t n_data_tiles, n_fill_tiles; // n_fill_tiles: per lane
    uint32_t tile_frames, n_channels;
};
struct IngestArgs {
    const uint8_t* raw;
    void* lanes;        // f32 or PCM16 lanes
    uint64_t lane_stride;
    const IngestJob* jobs;        // [n_jobs] (device)
    const uint32_t* unit_prefix;  // [n_jobs + 1]
    uint32_t n_jobs, n_units;
    int src_format, out_i16;      // FVAD_INGEST_*
};
int fvad_launch_ingest(const IngestArgs& a, hipStream_t stream); // hipError_t as int

// ------------------------------------------------------------------ resampling ingest (kernels_ingest_resample.hip)
// fvad_ingest_resample*: a work unit is a tile of one source -- tile_out consecutive outputs (resample_tile of resample.h, a
// multiple of 4) of every channel, whose window of source frames is staged through LDS -- or, after the n_data_tiles, a fill
// tile as above.  Output i of the job is output out_from + i of the FILE; frame f of the file lies at raw + src_off +
// (f - frame_base) * frame bytes.  One ratio and one tap table (resample_table's layout) per launch.
struct IngestResampleJob {
    uint64_t src_off;    // bytes from `raw` to the file's frame frame_base
    uint64_t frame_base, file_frames;
    uint64_t out_from, n_out;
    uint64_t dst_off;    // elements from `lanes` to the sample output out_from of channel 0 is written to
    uint64_t fill_len;   // zeros behind the outputs, in every lane of the source
    uint32_t n_data_tiles, n_fill_tiles; // n_fill_tiles: per lane
    uint32_t tile_out, n_channels;
};
struct IngestResampleArgs {
    const uint8_t* raw;
    float* lanes;
    uint64_t lane_stride;
    const IngestResampleJob* jobs; // [n_jobs] (device)
    const uint32_t* unit_prefix;   // [n_jobs + 1]
    const float* table;            // [ceil(n_taps / up)][up] (device)
    uint32_t n_jobs, n_units;
    uint32_t up, down, n_taps;
    int src_format;                // FVAD_INGEST_*
    uint32_t lds_bytes;            // the largest window of a tile of these jobs + 16
};
int fvad_launch_ingest_resample(const IngestResampleArgs& a, hipStream_t stream); // hipError_t as int

// ------------------------------------------------------------------ device-side egress (kernels_egress.hip)
// fvad_egress*: the ingest's inverse.  A work unit is a tile of one sink -- kIngestTileBytes of its DESTINATION bytes rounded
// down to whole frames in multiples of 4 (tile_frames, the ingest's rule), every channel of them.  A launch serves the jobs of
// ONE format pair; unit_prefix[j] counts the units in front of job j (a job has at least one unit).
struct EgressJob {
    uint64_t dst_off;   // bytes from `out` to the sink's frame 0
    uint64_t n_frames;
    uint64_t src_off;   // elements from `lanes` to the sample frame 0 of channel 0 is taken from
    uint32_t n_tiles, tile_frames;
    uint32_t n_channels, pad_;
};
struct EgressArgs {
    const void* lanes;  // f32 or PCM16 lanes
    uint64_t lane_stride;
    uint8_t* out;
    const EgressJob* jobs;        // [n_jobs] (device)
    const uint32_t* unit_prefix;  // [n_jobs + 1]
    uint32_t n_jobs, n_units;
    int src_format, file_format;  // FVAD_INGEST_*
};
int fvad_launch_egress(const EgressArgs& a, hipStream_t stream); // hipError_t as int

// ------------------------------------------------------------------ resampling egress (kernels_egress_resample.hip)
// fvad_egress_resample*: the egress with the clips' polyphase resampler in front of its conversion.  A work unit is a tile of
// one row -- tile_out consecutive OUTPUT frames (egress_resample_tile of egress_resample.h: a multiple of 4 whose bytes fit
// kIngestTileBytes and whose window of one channel fits kClipTile lane samples), every channel of them.  Output i of the job
// is output out_from + i of the STREAM; stream sample s of channel c lies at lanes + src_off + c * lane_stride +
// (s - frame_base).  One ratio and one tap table (resample_table's layout) per launch, the jobs of ONE file format.
struct EgressResampleJob {
    uint64_t dst_off;    // bytes from `out` to output out_from
    uint64_t out_from, n_out;
    uint64_t src_off;    // elements from `lanes` to stream sample frame_base of channel 0
    uint64_t frame_base, stream_frames;
    uint32_t n_tiles, tile_out;
    uint32_t n_channels, pad_;
};
struct EgressResampleArgs {
    const float* lanes;
    uint64_t lane_stride;
    uint8_t* out;
    const EgressResampleJob* jobs; // [n_jobs] (device)
    const uint32_t* unit_prefix;   // [n_jobs + 1]
    const float* table;            // [ceil(n_taps / up)][up] (device)
    uint32_t n_jobs, n_units;
    uint32_t up, down, n_taps;
    int file_format;               // FVAD_INGEST_*
};
int fvad_launch_egress_resample(const EgressResampleArgs& a, hipStream_t stream); // hipError_t as int

// ------------------------------------------------------------------ strided resampling egress (kernels_egress_resample.hip, egress_strided_kernel)
// fvad_egress_resample_strided*: the resampling egress over a stream that lies `step` apart in its lanes.  The jobs, the tile
// and the tables are the resampling egress's, counted in STRIDED samples; stream sample s of channel c lies at lanes + src_off
// + c * lane_stride + (s - frame_base) * step.
struct EgressStridedArgs {
    EgressResampleArgs r;
    uint32_t step;                 // 1 .. FVAD_EGRESS_STEP_MAX
};
int fvad_launch_egress_strided(const EgressStridedArgs& s, hipStream_t stream); // hipError_t as int
