// host_vad.h -- host-side VAD state machine (mirrors the reference's VADMachine / RollingAverage)
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <vector>

#include "../../include/fvad.h"
#include "vad_machine.h"

namespace fvad {

struct RollingAverage {            // src/structures/RollingAverage.zig
    std::vector<double> data;
    size_t len = 0;
    bool has_last_avg = false;
    double last_avg = 0;
    size_t write_idx = 0;
    size_t written_count = 0;
    // steady state (ring full): products data[i] * (1/len) and the running sum below write_idx
    bool steady = false;
    double scalar = 0, pref = 0;
    std::vector<double> q;
    RollingAverage(size_t count, bool has_initial, double initial_val);
    double push(float sample);
    double avg();
    void enter_steady();
};

struct MetaResult {                // VADMetadata.Result, VADMetadata.zig:5-9 (optionals)
    bool has_ratio = false, has_min = false, has_max = false;
    float volume_ratio = 0, volume_min = 0, volume_max = 0;
};
struct Metadata {                  // VADMetadata.zig:11-60
    bool has_ratio = false, has_min = false, has_max = false;
    float ratio_sum = 0, ratio_weight = 0, volume_min = 0, volume_max = 0;
    void push(const MetaResult& v, float weight);
    MetaResult to_result() const;
    void reset() { *this = Metadata(); }
};
MetaResult analyse_volume(const float* channel_rms, size_t n_channels);

struct VadMachine : VadMachineState { // src/AudioPipeline/VADMachine.zig; the step itself is vad_machine.h's
    VadMachineCfg cf;
    size_t n_channels;
    RollingAverage long_term, short_term, ch_ratio;
    std::vector<fvad_speech_segment> segments;
    uint64_t next_index = 0; // the first sample of the next frame to run (fvad_vad_batch_hold_from)
    // the long-term average is lazily exact (see host_vad.cpp): pushes on the full ring update the bound of vad_machine.h, and
    // the chain over the ring's cached products runs only when that bound cannot settle a comparison
    bool lt_lazy = true; // FVAD_VAD_EAGER=1 in the environment: run the chain on every push (testing aid)
    void long_term_push(float mv);
    void long_term_exact();

    VadMachine(const fvad_vad_config& c, size_t sample_rate, size_t n_channels, size_t fft_size);
    fvad_vad_result run(uint64_t index, const float* channel_volumes, bool has_ratio, float ratio);
    float min_volume(const float* channel_volumes) const;
};

// what a machine derives from (c, sample_rate, fft_size) -- *out is filled either way; FVAD_ERR_INVALID_ARGUMENT when a ring
// length is zero (channel ratio: RollingAverage.zig:36 would divide by zero) or does not fit in 32 bits
int vad_machine_cfg(const fvad_vad_config& c, size_t sample_rate, size_t fft_size, VadMachineCfg* out);

// items 0 .. n - 1 dealt to up to n_threads host threads
void deal(size_t n, int n_threads, const std::function<void(size_t)>& fn);

// ratio[s][k] is NaN where the frame carries no volume_ratio (null in the reference)
void run_many(VadMachine* const* vads, size_t n_streams, const float* const* band,
              const float* const* ratio, const size_t* n_frames, size_t n_channels,
              const uint64_t* first_index, size_t fft_size, int n_threads);

// the volume ratio of each of a stream's first n_frames FFT frames from its channels' chunk RMS (channel c's chunk k at
// chunk_rms[c * rms_stride + k]), as fvad_vad_batch_run hands it to the machines (every frame covers a chunk: each has a ratio)
// (frames from first_frame on, first_frame * fft_size a multiple of chunk_size: chunk_rms starts at the part's first chunk)
void sweep_frame_ratios(const float* chunk_rms, size_t rms_stride, size_t n_channels, size_t n_chunks, size_t n_frames, size_t fft_size,
                        size_t chunk_size, float* out, uint64_t first_frame = 0);

// the device state of a batch run in parts on the GPU (engine_sweep.cpp owns it; this file only releases it)
struct DevPartsDeleter {
    void (*fn)(void*) = nullptr;
    void operator()(void* p) const { if (fn) fn(p); }
};

} // namespace fvad

struct fvad_vad_batch;
namespace fvad {
// fvad_vad_batch_retain_configs in two steps, so that a failure leaves b as it was.  retain_stage: check keep (strictly
// increasing, < n_configs, n_keep > 0) and build in *nb what b becomes -- the kept configs with their sizes and bands
// recomputed in first-seen order, audits, lazy statistics, stat configs and scores compacted; nb->machines and nb->segs sized but
// empty (b is not touched).  retain_commit (cannot fail): move b's kept machines and segments into nb, then nb's fields into b
// (b's device part state too, unless nb already holds the compacted one).
// b's keys of the averages' tables from its configs, bands and sizes (fvad_vad_batch::st_keys ...): at creation and after a retain
int derive_avg_keys(fvad_vad_batch* b);
// b's trigger keys (fvad_vad_batch::trig_key, trig_rep) from its configs, bands and sizes: at creation and after a retain
int derive_trigger_keys(fvad_vad_batch* b);
int retain_stage(const fvad_vad_batch* b, const uint32_t* keep, size_t n_keep, fvad_vad_batch* nb);
void retain_commit(fvad_vad_batch* b, const uint32_t* keep, size_t n_keep, fvad_vad_batch* nb);
} // namespace fvad

// fvad_vad_batch (include/fvad.h): n_configs machines per stream, machine s * n_configs + c; a batch from
// fvad_vad_batch_create has one config.  Segments and audits of the last run, machine by machine.
struct fvad_vad_batch {
    std::vector<fvad_vad_config> cfgs;
    std::vector<int32_t> bins;      // distinct speech bands (min, max bin): size-major, first-seen order within a size
    std::vector<uint32_t> band_of;  // band of each config
    size_t sample_rate, n_channels, fft_size, n_streams; // (fft_size: sizes[0])
    // frame sizes (fvad_vad_batch_create_sweep_sized): the distinct sizes in first-seen config order, the size index of each
    // config and of each band; one size, all indices 0, for the other batches
    std::vector<size_t> sizes;
    std::vector<uint32_t> size_of, size_of_band;
    std::vector<std::vector<fvad_speech_segment>> segs;
    std::vector<fvad_vad_audit> audits;
    std::vector<uint64_t> exact_evals, lazy_pushes; // exact evaluations of the long-term chain / lazily absorbed pushes per machine
    // a run in parts (fvad_vad_batch_run_part): the streams' machines live on between the parts
    std::vector<std::unique_ptr<fvad::VadMachine>> machines;
    uint64_t next_sample = 0; // where the next host part starts, in samples (UINT64_MAX: the sizes' parts ended apart, none can follow)
    // a run in parts on the GPU (fvad_vad_batch_run_device_part): the machines' state in device memory between the parts
    std::unique_ptr<void, fvad::DevPartsDeleter> dev_parts;
    // fvad_vad_batch_run_device_part_async has launched a part and fvad_vad_batch_part_wait has not finished it: until then every
    // call that runs, scores, retains, reads results of or sets something on the batch returns FVAD_ERR_INVALID_ARGUMENT
    bool part_in_flight = false;
    // the last run was a device run: the machines' state is in device memory or gone, not in `machines` (fvad_vad_batch_hold_from)
    bool state_on_device = false;
    // fvad_vad_batch_chain_form: 0 = no device launch yet, 1 = the last one ran the lane form of the machines' kernel, 2 = the cooperative form
    int chain_form = 0;
    // The keys of the averages' tables (context option vad_avgs "table", kernels_vadavgs.hip), in first-seen config order: a short
    // key is (band, short_len) -- st_keys holds the pairs --, a ratio key (size index, ratio_len); st_key[c] / cr_key[c] are
    // config c's.  Configs with one key have the same short-term (channel-ratio) average in every frame of a stream.
    std::vector<uint32_t> st_keys, cr_keys, st_key, cr_key;
    // fvad_vad_batch_avgs_form: 0 = no device launch yet, 1 = the last one pushed the short rings, 2 = it read the tables;
    // avgs_bytes: the tables and min_volume rows of the last launch's part (0 with the rings)
    int avgs_form = 0;
    size_t avgs_bytes = 0;
    // The trigger keys (context option vad_trigger "shared", vad_finish.h), in first-seen config order: configs share a key when
    // everything their trigger derives is equal -- size index, band, the three ring lengths, has_init and initial, factor and
    // ratio_threshold (floating-point members as bit patterns).  trig_key[c]: config c's key; trig_rep[k]: key k's first config.
    std::vector<uint32_t> trig_key, trig_rep;
    // A shared run (engine_sweep.cpp): `trig` is an ordinary batch of one config per key whose machines emit bits instead of
    // finishing (it owns the trigger machines' part state); trig_of[c]: config c's machine in it (its order is private: after a
    // retain it is the old order, not first-seen).  trigger_form: 0 = no device launch yet, 1 = per-config machines, 2 = shared.
    std::unique_ptr<fvad_vad_batch> trig;
    std::vector<uint32_t> trig_of;
    int trigger_form = 0;
    size_t trigger_bytes = 0;                           // the bits of the last part
    uint64_t trig_machine_launches = 0, trig_finish_launches = 0; // cumulative, shared form
    // scoring (host_eval.cpp, kernels_eval.hip): each stream's labels stably sorted by start with the prefix max of their ends
    // (ref_off: n_streams + 1 offsets), one fvad_stat_config per config; the scores of the segments last run, machine by machine
    bool has_refs = false;
    std::vector<fvad_segment_sec> refs;
    std::vector<float> ref_pmax;
    std::vector<size_t> ref_off;
    std::vector<fvad_stat_config> stat_cfgs;
    bool scored = false;
    std::vector<fvad_single_stats> scores;
    // fvad_vad_batch_set_keep_segments: 0 = a device run leaves the segments on the device (segs_kept is false until a run keeps them)
    bool keep_segments = true, segs_kept = true;
};
