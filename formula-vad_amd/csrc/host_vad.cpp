// host_vad.cpp -- the sequential tail of the path, on the host by design.
//
// Mirrors src/structures/RollingAverage.zig, src/AudioPipeline/VADMetadata.zig and
// src/AudioPipeline/VADMachine.zig of the reference: f64 rolling averages re-summed in index
// order on every push (RollingAverage.zig:45-56), integer sample arithmetic, @intFromFloat
// truncations.  Segment boundaries are integers decided by `short_term > threshold`
// (VADMachine.zig:171), so this code keeps the reference's exact operation order; the GPU only
// supplies the per-frame band sums and per-chunk RMS values that feed it.  The machine's step past
// its rolling averages is vad_machine.h's, which the sweep kernel (kernels_vad.hip) shares.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "host_vad.h"
#include "vad_avgs.h"
#include "vad_finish.h"
#include "vad_ratio.h"

namespace fvad {

// ------------------------------------------------------------------ RollingAverage
RollingAverage::RollingAverage(size_t count, bool has_initial, double initial_val)
    : data(count ? count : 1, 0.0), len(count)
{
    if (has_initial) { // RollingAverage.zig:20-26
        std::fill(data.begin(), data.begin() + (long)count, initial_val);
        written_count = count;
        avg();
        if (count) enter_steady();
    }
}

double RollingAverage::avg() // RollingAverage.zig:45-56
{
    double a = 0.0;
    const double scalar = 1.0 / (double)written_count;
    const double* d = data.data();
    for (size_t i = 0; i < written_count; ++i) a += d[i] * scalar;
    last_avg = a;
    has_last_avg = true;
    return a;
}

// The reference re-sums the whole ring on every push (RollingAverage.zig:45-56): a chain of `len`
// dependent f64 adds.  Once the ring is full the terms below the write index have not changed since
// the previous push, so the running sum up to (not including) the write index -- `pref` -- is still
// exactly what the reference's loop would have in its accumulator at that point.  Resuming the
// chain from there performs the very same additions in the very same order for the remaining
// terms: bit-identical result, half the work on average.
double RollingAverage::push(float sample) // RollingAverage.zig:34-43
{
    if (steady) {
        const size_t w = write_idx;
        data[w] = (double)sample;
        q[w] = data[w] * scalar;
        double acc = (w == 0) ? 0.0 : pref;
        acc += q[w];
        const double new_pref = acc;
        const double* qq = q.data();
        for (size_t i = w + 1; i < len; ++i) acc += qq[i];
        last_avg = acc;
        has_last_avg = true;
        write_idx = (w + 1) % len;
        pref = (write_idx == 0) ? 0.0 : new_pref;
        return acc;
    }
    data[write_idx] = (double)sample;
    write_idx = (write_idx + 1) % len;
    if (written_count < len) written_count += 1;
    const double a = avg();
    if (written_count == len && write_idx == 0) enter_steady();
    return a;
}

void RollingAverage::enter_steady()
{
    scalar = 1.0 / (double)len;
    q.resize(len);
    for (size_t i = 0; i < len; ++i) q[i] = data[i] * scalar;
    pref = 0.0;
    for (size_t i = 0; i < write_idx; ++i) pref += q[i]; // same chain the full loop would run
    steady = true;
}

// ------------------------------------------------------------------ VADMetadata
void Metadata::push(const MetaResult& v, float weight) // VADMetadata.zig:29-60
{
    if (v.has_ratio) {
        if (!has_ratio) { has_ratio = true; ratio_sum = 0.0f; ratio_weight = 0.0f; }
        ratio_sum += v.volume_ratio * weight;
        ratio_weight += weight;
    }
    if (v.has_min && (!has_min || v.volume_min < volume_min)) { has_min = true; volume_min = v.volume_min; }
    if (v.has_max && (!has_max || v.volume_max > volume_max)) { has_max = true; volume_max = v.volume_max; }
}

MetaResult Metadata::to_result() const // VADMetadata.zig:16-27
{
    MetaResult r;
    r.has_min = has_min; r.volume_min = volume_min;
    r.has_max = has_max; r.volume_max = volume_max;
    if (has_ratio) { r.has_ratio = true; r.volume_ratio = ratio_sum / ratio_weight; }
    return r;
}

// BufferedVolumeAnalyzer.analyseVolume (BufferedVolumeAnalyzer.zig:48-69) from per-channel RMS
MetaResult analyse_volume(const float* channel_rms, size_t n_channels)
{
    float vol_min = 1, vol_max = 0;
    for (size_t c = 0; c < n_channels; ++c) {
        const float vol = channel_rms[c];
        if (vol < vol_min) vol_min = vol;
        if (vol > vol_max) vol_max = vol;
    }
    MetaResult r;
    r.has_ratio = r.has_min = r.has_max = true;
    r.volume_ratio = (vol_max == 0) ? 0 : vol_min / vol_max;
    r.volume_min = vol_min;
    r.volume_max = vol_max;
    return r;
}

// ------------------------------------------------------------------ VADMachine
int vad_machine_cfg(const fvad_vad_config& c, size_t sample_rate, size_t fft_size, VadMachineCfg* out)
{
    // VADMachine.zig:75-106
    const float sample_rate_f = (float)sample_rate;
    const float fft_size_f = (float)fft_size;
    const float eval_per_sec = sample_rate_f / fft_size_f;
    const size_t long_len = std::max<size_t>(1, (size_t)(eval_per_sec * c.long_term_speech_avg_sec));
    const size_t short_len = std::max<size_t>(1, (size_t)(eval_per_sec * c.short_term_speech_avg_sec));
    const size_t ratio_len = (size_t)(eval_per_sec * c.channel_vol_ratio_avg_sec);
    VadMachineCfg& k = *out;
    k.lt_scalar = 1.0 / (double)long_len;
    k.st_scalar = 1.0 / (double)short_len;
    k.cr_scalar = 1.0 / (double)ratio_len;
    k.lt_q_init = c.initial_long_term_avg * k.lt_scalar;
    k.initial = c.initial_long_term_avg;
    k.factor = (double)c.speech_threshold_factor;
    k.ratio_threshold = (double)c.channel_vol_ratio_threshold;
    const double n = (double)long_len;
    k.gamma = n * kU / (1.0 - n * kU);
    k.min_open = (uint64_t)(sample_rate_f * c.min_consecutive_sec_to_open); // :161
    k.max_gap = (uint64_t)(sample_rate_f * c.max_speech_gap_sec);           // :163
    k.start_buffer = (uint64_t)(sample_rate_f * 2);                          // :312-325
    k.end_buffer = (uint64_t)(sample_rate_f * 2);
    k.input_len_sec = fft_size_f / sample_rate_f;
    k.sample_rate_f = sample_rate_f;
    k.min_vad_duration_sec = c.min_vad_duration_sec;
    k.long_len = (uint32_t)long_len;
    k.short_len = (uint32_t)short_len;
    k.ratio_len = (uint32_t)ratio_len;
    k.has_init = c.has_initial_long_term_avg != 0;
    k.band = 0;
    if (ratio_len == 0 || long_len > 0xFFFFFFFFu || short_len > 0xFFFFFFFFu || ratio_len > 0xFFFFFFFFu) return FVAD_ERR_INVALID_ARGUMENT;
    return FVAD_OK;
}

VadMachine::VadMachine(const fvad_vad_config& c, size_t sample_rate, size_t n_channels_, size_t fft_size)
    : n_channels(n_channels_), long_term(1, false, 0), short_term(1, false, 0), ch_ratio(1, false, 0)
{
    vad_machine_cfg(c, sample_rate, fft_size, &cf); // (every caller has checked c with it)
    long_term = RollingAverage(cf.long_len, cf.has_init != 0, cf.initial);
    short_term = RollingAverage(cf.short_len, false, 0);
    ch_ratio = RollingAverage(cf.ratio_len, false, 0);
    lt_last = long_term.last_avg; // (an initial value fills the ring and evaluates its average)
    has_last = long_term.has_last_avg;
    segments.reserve(100); // :111
    const char* eager = getenv("FVAD_VAD_EAGER");
    lt_lazy = !(eager && eager[0] == '1');
}

// ---- lazily exact long-term average
// The long-term average feeds exactly one thing: the comparison `short_term > long_term * factor`
// (VADMachine.zig:169-171; plus this build's margin audit).  Re-running the reference's chain of `len`
// dependent f64 adds on every push (RollingAverage.zig:45-56) makes a stream cost ~4.5 us per frame and a
// two-hour stream three seconds, however many cores there are.  Instead the machine keeps
//   lt_approx = the chain's last exact value, updated as fl(fl(lt_approx + q_new) - q_old) per push,
//   lt_err    = a running bound on the rounding error of those updates,
//   lt_abs    = (approximately) sum |q_i|,
// and bounds the distance to what the chain would return *now*:
//   |lt_approx - chain| <= gamma_N sum|q_i|(anchor) + lt_err + gamma_N sum|q_i|(now)
// (gamma_N = N u / (1 - N u), u = 2^-53: the chain's error against the real-number sum when lt_approx was
// anchored on it, the updates' rounding, the chain's own error now).
// decide() (vad_machine.h) evaluates the comparison with the threshold interval this gives; only if `short_term` falls
// inside the interval, or the frame could lower the audit's minimum margin, is the chain run for real
// (long_term_exact: the reference's additions in the reference's order).  Every decision and every
// audited number is therefore the one the eager evaluation produces; the tests compare whole runs
// bit for bit with the oracle.
void VadMachine::long_term_exact()
{
    const double* qq = long_term.q.data();
    double acc = 0.0, abs_sum = 0.0;
    for (size_t i = 0; i < long_term.len; ++i) {
        acc += qq[i]; // == a += data[i] * scalar (RollingAverage.zig:50-53), products cached in q
        abs_sum += std::fabs(qq[i]);
    }
    anchor(acc, abs_sum);
}

void VadMachine::long_term_push(float mv) // RollingAverage.push for the long-term ring
{
    RollingAverage& a = long_term;
    if (!a.steady || !lt_lazy) { // ring not full yet (or eager mode): the reference's path as is
        const bool was_steady = a.steady;
        lt_last = a.push(mv);
        has_last = true;
        if (lt_lazy && !was_steady && a.steady) long_term_exact();
        return;
    }
    if (!lt_anchored) long_term_exact(); // first lazy push: anchor on the chain's current value
    const size_t w = a.write_idx;
    const double qn = (double)mv * a.scalar, qo = a.q[w];
    a.data[w] = (double)mv;
    a.q[w] = qn;
    a.write_idx = (w + 1) % a.len;
    if (lazy_update(qn, qo)) long_term_exact();
}

float VadMachine::min_volume(const float* channel_volumes) const // :153-158
{
    float min_v = 999, max_v = 0;
    for (size_t c = 0; c < n_channels; ++c) {
        const float v = channel_volumes[c];
        if (v < min_v) min_v = v;
        if (v > max_v) max_v = v;
    }
    (void)max_v;
    return min_v;
}

fvad_vad_result VadMachine::run(uint64_t index, const float* channel_volumes, bool has_ratio, float ratio)
{
    const float mv = min_volume(channel_volumes);
    const double st = short_term.push(mv);                       // :166
    const double cr = ch_ratio.push(has_ratio ? ratio : 0);      // :167
    const bool met = decide(cf, st, cr, [&] { long_term_exact(); });
    if (!met) long_term_push(mv);                                // :176-178
    return finish_step(cf, index, met, has_ratio, ratio, [&](const fvad_speech_segment& s) { segments.push_back(s); });
}

// items 0 .. n - 1 dealt to up to n_threads host threads
void deal(size_t n, int n_threads, const std::function<void(size_t)>& fn)
{
    const int nt = (int)std::min<size_t>((size_t)std::max(n_threads, 1), n);
    if (nt <= 1) { for (size_t i = 0; i < n; ++i) fn(i); return; }
    std::vector<std::thread> th;
    std::atomic<size_t> next{0};
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&]() { for (;;) { const size_t i = next.fetch_add(1); if (i >= n) break; fn(i); } });
    for (auto& t : th) t.join();
}

// ------------------------------------------------------------------ many streams
// Streams are independent (one pipeline per file, simulator.zig:225-231); with the lazily exact
// long-term average a frame costs ~0.1 us, so the streams are simply dealt to threads.
void run_many(VadMachine* const* vads, size_t n_streams, const float* const* band,
              const float* const* ratio, const size_t* n_frames, size_t n_channels,
              const uint64_t* first_index, size_t fft_size, int n_threads)
{
    deal(n_streams, n_threads, [&](size_t s) {
        VadMachine* m = vads[s];
        for (size_t k = 0; k < n_frames[s]; ++k) {
            const float r = ratio[s][k];
            const bool has_ratio = !std::isnan(r);
            m->run(first_index[s] + (uint64_t)k * fft_size, band[s] + k * n_channels, has_ratio, r);
        }
    });
}

} // namespace fvad

// ------------------------------------------------------------------ C ABI
struct fvad_vad { fvad::VadMachine m; fvad_vad(const fvad_vad_config& c, size_t sr, size_t nc, size_t fs) : m(c, sr, nc, fs) {} };
struct fvad_rolling_average { fvad::RollingAverage ra; fvad_rolling_average(size_t n, bool h, double v) : ra(n, h, v) {} };

extern "C" {

void fvad_vad_config_default(fvad_vad_config* c)
{
    c->speech_min_freq = 500; c->speech_max_freq = 2000;
    c->long_term_speech_avg_sec = 180; c->has_initial_long_term_avg = 1; c->initial_long_term_avg = 0.005;
    c->short_term_speech_avg_sec = 0.2f; c->speech_threshold_factor = 10;
    c->channel_vol_ratio_avg_sec = 0.5f; c->channel_vol_ratio_threshold = 0.5f;
    c->min_consecutive_sec_to_open = 0.2f; c->max_speech_gap_sec = 2; c->min_vad_duration_sec = 0.7f;
}

int fvad_vad_create(const fvad_vad_config* cfg, size_t sample_rate, size_t n_channels, size_t fft_size, fvad_vad** out)
{
    if (!cfg || !out || n_channels == 0 || fft_size == 0 || sample_rate == 0) return FVAD_ERR_INVALID_ARGUMENT;
    fvad::VadMachineCfg k;
    if (const int rc = fvad::vad_machine_cfg(*cfg, sample_rate, fft_size, &k)) return rc;
    *out = new (std::nothrow) fvad_vad(*cfg, sample_rate, n_channels, fft_size);
    return *out ? FVAD_OK : FVAD_ERR_ALLOC_FAILED;
}
void fvad_vad_destroy(fvad_vad* v) { delete v; }

int fvad_vad_run(fvad_vad* v, uint64_t index, const float* channel_volumes, int has_ratio, float volume_ratio, fvad_vad_result* out)
{
    if (!v || !channel_volumes) return FVAD_ERR_INVALID_ARGUMENT;
    const fvad_vad_result r = v->m.run(index, channel_volumes, has_ratio != 0, volume_ratio);
    if (out) *out = r;
    return FVAD_OK;
}
size_t fvad_vad_segment_count(const fvad_vad* v) { return v ? v->m.segments.size() : 0; }
int fvad_vad_segments(const fvad_vad* v, fvad_speech_segment* out, size_t cap, size_t* n)
{
    if (!v || !n) return FVAD_ERR_INVALID_ARGUMENT;
    *n = v->m.segments.size();
    if (cap < *n) return FVAD_ERR_BUFFER_TOO_SMALL;
    if (*n) memcpy(out, v->m.segments.data(), *n * sizeof(fvad_speech_segment));
    return FVAD_OK;
}
int fvad_vad_lazy_stats(const fvad_vad* v, uint64_t* exact_evaluations, uint64_t* lazy_pushes)
{
    if (!v) return FVAD_ERR_INVALID_ARGUMENT;
    if (exact_evaluations) *exact_evaluations = v->m.exact_evals;
    if (lazy_pushes) *lazy_pushes = v->m.lazy_pushes;
    return FVAD_OK;
}

int fvad_vad_audit_get(const fvad_vad* v, fvad_vad_audit* out)
{
    if (!v || !out) return FVAD_ERR_INVALID_ARGUMENT;
    *out = v->m.audit;
    return FVAD_OK;
}

int fvad_vad_run_many(fvad_vad* const* vads, size_t n_streams, const float* const* band, const float* const* ratio,
                      const size_t* n_frames, size_t n_channels, const uint64_t* first_index, size_t fft_size, int n_threads)
{
    if (!vads || !band || !ratio || !n_frames || !first_index) return FVAD_ERR_INVALID_ARGUMENT;
    std::vector<fvad::VadMachine*> ms(n_streams);
    for (size_t i = 0; i < n_streams; ++i) {
        if (!vads[i] || vads[i]->m.n_channels != n_channels) return FVAD_ERR_CHANNEL_COUNT_MISMATCH;
        ms[i] = &vads[i]->m;
    }
    fvad::run_many(ms.data(), n_streams, band, ratio, n_frames, n_channels, first_index, fft_size, n_threads);
    return FVAD_OK;
}

int fvad_ra_create(size_t count, int has_initial, double initial_val, fvad_rolling_average** out)
{
    if (!out || count == 0) return FVAD_ERR_INVALID_ARGUMENT;
    *out = new (std::nothrow) fvad_rolling_average(count, has_initial != 0, initial_val);
    return *out ? FVAD_OK : FVAD_ERR_ALLOC_FAILED;
}
void fvad_ra_destroy(fvad_rolling_average* ra) { delete ra; }
double fvad_ra_push(fvad_rolling_average* ra, float sample) { return ra->ra.push(sample); }
int fvad_ra_last_avg(const fvad_rolling_average* ra, double* out)
{
    if (ra->ra.has_last_avg && out) *out = ra->ra.last_avg;
    return ra->ra.has_last_avg ? 1 : 0;
}

// ------------------------------------------------------------------ host stage for a whole batch
// What VADPipeline does between the kernels' outputs and the segment list, for many streams at once and
// straight from the engine's lane-major buffers: per-chunk volume ratio (BufferedVolumeAnalyzer.zig:48-69) ->
// the two metadata hand-overs (BufferedVolumeAnalyzer.zig:33-45, BufferedDenoiser.zig:83-86,115) -> the
// sample-weighted ratio of every FFT frame (BufferedFFT.zig:137-140,153) -> VADMachine.run per frame
// (VADMachine.zig:138-239).  Streams are dealt to threads like simulator.zig:221-232 deals files.
int fvad_vad_batch_create(const fvad_vad_config* cfg, size_t sample_rate, size_t n_channels, size_t fft_size, size_t n_streams,
                          fvad_vad_batch** out)
{
    if (!cfg || !out || n_channels == 0 || fft_size == 0 || sample_rate == 0 || n_streams == 0) return FVAD_ERR_INVALID_ARGUMENT;
    fvad::VadMachineCfg k;
    if (const int rc = fvad::vad_machine_cfg(*cfg, sample_rate, fft_size, &k)) return rc;
    auto* b = new (std::nothrow) fvad_vad_batch();
    if (!b) return FVAD_ERR_ALLOC_FAILED;
    b->cfgs.assign(1, *cfg); b->sample_rate = sample_rate; b->n_channels = n_channels; b->fft_size = fft_size; b->n_streams = n_streams;
    // the band of a plain batch is whatever the caller summed: one block, whatever the config's edges say
    const float bin_width = (float)sample_rate / (float)fft_size;
    b->bins = {(int32_t)roundf(cfg->speech_min_freq / bin_width), (int32_t)roundf(cfg->speech_max_freq / bin_width)};
    b->band_of.assign(1, 0);
    b->sizes.assign(1, fft_size); b->size_of.assign(1, 0); b->size_of_band.assign(1, 0);
    b->segs.resize(n_streams);
    b->audits.resize(n_streams);
    b->exact_evals.assign(n_streams, 0);
    b->lazy_pushes.assign(n_streams, 0);
    if (const int rc = fvad::derive_avg_keys(b)) { delete b; return rc; }
    if (const int rc = fvad::derive_trigger_keys(b)) { delete b; return rc; }
    *out = b;
    return FVAD_OK;
}

// The checks fvad_vad_create and fvad_pipeline_create make of a VADMachine.Config, with their status codes: the speech band's
// edges as FFT.freqToBin sees them (FFT.zig:156-167, then the pipeline's max < min), the ring lengths (vad_machine_cfg)
static int check_sweep_config(const fvad_vad_config& c, size_t sample_rate, size_t fft_size, int32_t* lo, int32_t* hi)
{
    const float bin_width = (float)sample_rate / (float)fft_size;
    const float nyq = (float)sample_rate / 2;
    if (c.speech_min_freq > nyq || c.speech_max_freq > nyq) return FVAD_ERR_OUT_OF_RANGE;
    if (c.speech_min_freq < 0 || c.speech_max_freq < 0) return FVAD_ERR_NEGATIVE_FREQUENCY;
    *lo = (int32_t)roundf(c.speech_min_freq / bin_width);
    *hi = (int32_t)roundf(c.speech_max_freq / bin_width);
    if (*hi < *lo) return FVAD_ERR_INVALID_ARGUMENT;
    fvad::VadMachineCfg k;
    return fvad::vad_machine_cfg(c, sample_rate, fft_size, &k);
}

// The bands of configs cfgs[c] at frame sizes sizes[size_of[c]]: a band is (size, min bin, max bin); bands size-major, first-seen
// config order within a size.  The configs are checked at their own sizes.
static int make_sweep(const fvad_vad_config* cfgs, size_t n_configs, const std::vector<size_t>& sizes, const std::vector<uint32_t>& size_of,
                      size_t sample_rate, size_t n_channels, size_t n_streams, fvad_vad_batch** out)
{
    std::vector<std::vector<int32_t>> bins(sizes.size()); // per size, first-seen order
    std::vector<uint32_t> local(n_configs);
    for (size_t c = 0; c < n_configs; ++c) {
        int32_t lo = 0, hi = 0;
        const int rc = check_sweep_config(cfgs[c], sample_rate, sizes[size_of[c]], &lo, &hi);
        if (rc) return rc;
        std::vector<int32_t>& bg = bins[size_of[c]];
        size_t j = 0;
        while (j < bg.size() / 2 && !(bg[2 * j] == lo && bg[2 * j + 1] == hi)) ++j;
        if (j == bg.size() / 2) { bg.push_back(lo); bg.push_back(hi); }
        local[c] = (uint32_t)j;
    }
    auto* b = new (std::nothrow) fvad_vad_batch();
    if (!b) return FVAD_ERR_ALLOC_FAILED;
    std::vector<uint32_t> first(sizes.size()); // each size's first band
    for (size_t g = 0; g < sizes.size(); ++g) {
        first[g] = (uint32_t)(b->bins.size() / 2);
        b->bins.insert(b->bins.end(), bins[g].begin(), bins[g].end());
        b->size_of_band.insert(b->size_of_band.end(), bins[g].size() / 2, (uint32_t)g);
    }
    b->band_of.resize(n_configs);
    for (size_t c = 0; c < n_configs; ++c) b->band_of[c] = first[size_of[c]] + local[c];
    b->cfgs.assign(cfgs, cfgs + n_configs); b->sample_rate = sample_rate; b->n_channels = n_channels; b->fft_size = sizes[0];
    b->n_streams = n_streams;
    b->sizes = sizes;
    b->size_of = size_of;
    b->segs.resize(n_streams * n_configs);
    b->audits.resize(n_streams * n_configs);
    b->exact_evals.assign(n_streams * n_configs, 0);
    b->lazy_pushes.assign(n_streams * n_configs, 0);
    if (const int rc = fvad::derive_avg_keys(b)) { delete b; return rc; }
    if (const int rc = fvad::derive_trigger_keys(b)) { delete b; return rc; }
    *out = b;
    return FVAD_OK;
}

int fvad_vad_batch_create_sweep(const fvad_vad_config* cfgs, size_t n_configs, size_t sample_rate, size_t n_channels, size_t fft_size,
                                size_t n_streams, fvad_vad_batch** out)
{
    if (!cfgs || !out || n_configs == 0 || n_channels == 0 || fft_size == 0 || sample_rate == 0 || n_streams == 0) return FVAD_ERR_INVALID_ARGUMENT;
    return make_sweep(cfgs, n_configs, {fft_size}, std::vector<uint32_t>(n_configs, 0), sample_rate, n_channels, n_streams, out);
}

int fvad_vad_batch_create_sweep_sized(const fvad_vad_config* cfgs, const size_t* fft_sizes, size_t n_configs, size_t sample_rate,
                                      size_t n_channels, size_t n_streams, fvad_vad_batch** out)
{
    if (!cfgs || !fft_sizes || !out || n_configs == 0 || n_channels == 0 || sample_rate == 0 || n_streams == 0) return FVAD_ERR_INVALID_ARGUMENT;
    std::vector<size_t> sizes; // distinct, first-seen order
    std::vector<uint32_t> size_of(n_configs);
    for (size_t c = 0; c < n_configs; ++c) {
        const size_t F = fft_sizes[c];
        if (F < 4 || F > 16384 || F % 2) return FVAD_ERR_INVALID_ARGUMENT; // (fvad_engine_band_sums_device's sizes)
        size_t g = 0;
        while (g < sizes.size() && sizes[g] != F) ++g;
        if (g == sizes.size()) sizes.push_back(F);
        size_of[c] = (uint32_t)g;
    }
    return make_sweep(cfgs, n_configs, sizes, size_of, sample_rate, n_channels, n_streams, out);
}

int fvad_vad_batch_frame_sizes(const fvad_vad_batch* b, size_t* sizes, size_t cap, size_t* n_sizes, uint32_t* size_of_band)
{
    if (!b || !n_sizes) return FVAD_ERR_INVALID_ARGUMENT;
    *n_sizes = b->sizes.size();
    if (size_of_band) memcpy(size_of_band, b->size_of_band.data(), b->size_of_band.size() * sizeof(uint32_t));
    if (cap < *n_sizes) return FVAD_ERR_BUFFER_TOO_SMALL;
    if (!sizes) return FVAD_ERR_INVALID_ARGUMENT;
    memcpy(sizes, b->sizes.data(), b->sizes.size() * sizeof(size_t));
    return FVAD_OK;
}

void fvad_vad_batch_destroy(fvad_vad_batch* b) { delete b; }

size_t fvad_vad_batch_n_configs(const fvad_vad_batch* b) { return b ? b->cfgs.size() : 0; }

int fvad_vad_batch_avg_keys(const fvad_vad_batch* b, uint32_t* st_keys, uint32_t* cr_keys, size_t cap, size_t* n_st_keys,
                            size_t* n_cr_keys, uint32_t* st_key, uint32_t* cr_key)
{
    if (!b || !n_st_keys || !n_cr_keys) return FVAD_ERR_INVALID_ARGUMENT;
    *n_st_keys = b->st_keys.size() / 2;
    *n_cr_keys = b->cr_keys.size() / 2;
    if (st_key) memcpy(st_key, b->st_key.data(), b->st_key.size() * sizeof(uint32_t));
    if (cr_key) memcpy(cr_key, b->cr_key.data(), b->cr_key.size() * sizeof(uint32_t));
    if (cap < *n_st_keys || cap < *n_cr_keys) return FVAD_ERR_BUFFER_TOO_SMALL;
    if (!st_keys || !cr_keys) return FVAD_ERR_INVALID_ARGUMENT;
    memcpy(st_keys, b->st_keys.data(), b->st_keys.size() * sizeof(uint32_t));
    memcpy(cr_keys, b->cr_keys.data(), b->cr_keys.size() * sizeof(uint32_t));
    return FVAD_OK;
}

int fvad_vad_batch_trigger_keys(const fvad_vad_batch* b, uint32_t* key_of, size_t cap, size_t* n_keys, uint32_t* rep)
{
    if (!b || !n_keys) return FVAD_ERR_INVALID_ARGUMENT;
    *n_keys = b->trig_rep.size();
    if (key_of) memcpy(key_of, b->trig_key.data(), b->trig_key.size() * sizeof(uint32_t));
    if (!rep) return FVAD_OK; // (the counts, and each config's key, only)
    if (cap < *n_keys) return FVAD_ERR_BUFFER_TOO_SMALL;
    memcpy(rep, b->trig_rep.data(), b->trig_rep.size() * sizeof(uint32_t));
    return FVAD_OK;
}

int fvad_vad_finish_bits(const fvad_vad_config* cfg, size_t sample_rate, size_t fft_size, const uint64_t* words, const float* ratios,
                         size_t n_frames, uint64_t first_sample, uint64_t* state, fvad_speech_segment* segs, size_t seg_cap,
                         size_t* n_segs)
{
    if (!cfg || !state || !n_segs || sample_rate == 0 || fft_size == 0) return FVAD_ERR_INVALID_ARGUMENT;
    if (n_frames && (!words || !ratios)) return FVAD_ERR_INVALID_ARGUMENT;
    if (seg_cap && !segs) return FVAD_ERR_INVALID_ARGUMENT;
    fvad::VadMachineCfg k;
    if (const int rc = fvad::vad_machine_cfg(*cfg, sample_rate, fft_size, &k)) return rc;
    if (state[0] > 3) return FVAD_ERR_INVALID_ARGUMENT;
    fvad::VadMachineState m;
    uint32_t f32s[2];
    m.state = (int)state[0];
    m.speech_start = state[1];
    m.speech_end = state[2];
    m.ratio_count = state[3];
    f32s[0] = (uint32_t)state[4];
    f32s[1] = (uint32_t)(state[4] >> 32);
    memcpy(&m.ratio_sum, &f32s[0], 4);
    memcpy(&m.met_cum, &f32s[1], 4);
    size_t n = 0;
    fvad::finish_walk(m, k, 0, n_frames, first_sample, fft_size, [&](uint64_t w) { return words[w]; },
                      [&](uint64_t f) { return ratios[f]; }, [] { return true; },
                      [&](const fvad_speech_segment& sg) { if (n < seg_cap) segs[n] = sg; ++n; });
    state[0] = (uint64_t)m.state;
    state[1] = m.speech_start;
    state[2] = m.speech_end;
    state[3] = m.ratio_count;
    memcpy(&f32s[0], &m.ratio_sum, 4);
    memcpy(&f32s[1], &m.met_cum, 4);
    state[4] = (uint64_t)f32s[0] | (uint64_t)f32s[1] << 32;
    state[5] += n;
    *n_segs = n;
    return n > seg_cap ? FVAD_ERR_BUFFER_TOO_SMALL : FVAD_OK;
}

int fvad_vad_avg_chain(const float* x, size_t n_frames, size_t first_frame, uint32_t len, const float* ring, double* out)
{
    if (len == 0 || (n_frames && (!x || !out)) || (first_frame && !ring)) return FVAD_ERR_INVALID_ARGUMENT;
    const double scalar = 1.0 / (double)len;
    for (size_t k = 0; k < n_frames; ++k)
        out[k] = fvad::ring_avg_at((uint64_t)(first_frame + k), len, scalar,
                                   [&](uint32_t i, uint64_t f) { return f >= first_frame ? x[f - first_frame] : ring[i]; });
    return FVAD_OK;
}

int fvad_vad_batch_bands(const fvad_vad_batch* b, int32_t* bins, size_t cap, size_t* n_bands, uint32_t* band_of)
{
    if (!b || !n_bands) return FVAD_ERR_INVALID_ARGUMENT;
    *n_bands = b->bins.size() / 2;
    if (band_of) memcpy(band_of, b->band_of.data(), b->band_of.size() * sizeof(uint32_t));
    if (cap < *n_bands) return FVAD_ERR_BUFFER_TOO_SMALL;
    if (*n_bands && !bins) return FVAD_ERR_INVALID_ARGUMENT;
    memcpy(bins, b->bins.data(), b->bins.size() * sizeof(int32_t));
    return FVAD_OK;
}

} // extern "C"

namespace fvad {

int derive_avg_keys(fvad_vad_batch* b)
{
    const size_t NC = b->cfgs.size();
    b->st_keys.clear(); b->cr_keys.clear();
    b->st_key.assign(NC, 0); b->cr_key.assign(NC, 0);
    auto find = [](std::vector<uint32_t>& keys, uint32_t src, uint32_t len) {
        size_t j = 0;
        while (j < keys.size() / 2 && !(keys[2 * j] == src && keys[2 * j + 1] == len)) ++j;
        if (j == keys.size() / 2) { keys.push_back(src); keys.push_back(len); }
        return (uint32_t)j;
    };
    for (size_t c = 0; c < NC; ++c) {
        VadMachineCfg k;
        if (const int rc = vad_machine_cfg(b->cfgs[c], b->sample_rate, b->sizes[b->size_of[c]], &k)) return rc;
        b->st_key[c] = find(b->st_keys, b->band_of[c], k.short_len);
        b->cr_key[c] = find(b->cr_keys, b->size_of[c], k.ratio_len);
    }
    return FVAD_OK;
}

int derive_trigger_keys(fvad_vad_batch* b)
{
    struct Key {
        uint32_t size, band, long_len, short_len, ratio_len;
        int32_t has_init;
        uint64_t initial, factor, ratio_threshold; // bit patterns
        bool operator==(const Key& o) const
        {
            return size == o.size && band == o.band && long_len == o.long_len && short_len == o.short_len && ratio_len == o.ratio_len &&
                   has_init == o.has_init && initial == o.initial && factor == o.factor && ratio_threshold == o.ratio_threshold;
        }
    };
    auto bits = [](double d) { uint64_t u; memcpy(&u, &d, 8); return u; };
    const size_t NC = b->cfgs.size();
    std::vector<Key> keys;
    b->trig_key.assign(NC, 0);
    b->trig_rep.clear();
    for (size_t c = 0; c < NC; ++c) {
        VadMachineCfg k;
        if (const int rc = vad_machine_cfg(b->cfgs[c], b->sample_rate, b->sizes[b->size_of[c]], &k)) return rc;
        const Key key{b->size_of[c], b->band_of[c], k.long_len, k.short_len, k.ratio_len, k.has_init, bits(k.initial), bits(k.factor),
                      bits(k.ratio_threshold)};
        size_t j = 0;
        while (j < keys.size() && !(keys[j] == key)) ++j;
        if (j == keys.size()) { keys.push_back(key); b->trig_rep.push_back((uint32_t)c); }
        b->trig_key[c] = (uint32_t)j;
    }
    return FVAD_OK;
}

int retain_stage(const fvad_vad_batch* b, const uint32_t* keep, size_t n_keep, fvad_vad_batch* nb)
{
    const size_t NC = b->cfgs.size(), S = b->n_streams;
    if (n_keep == 0 || !keep) return FVAD_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n_keep; ++i)
        if (keep[i] >= NC || (i && keep[i] <= keep[i - 1])) return FVAD_ERR_INVALID_ARGUMENT;
    try {
        // the sizes and bands of the kept configs as make_sweep finds them: sizes in first-seen order, bands size-major and
        // first-seen within a size (a band's bins are the old band's: the same config at the same size)
        std::vector<uint32_t> size_of(n_keep);
        for (size_t c = 0; c < n_keep; ++c) {
            const size_t F = b->sizes[b->size_of[keep[c]]];
            size_t g = 0;
            while (g < nb->sizes.size() && nb->sizes[g] != F) ++g;
            if (g == nb->sizes.size()) nb->sizes.push_back(F);
            size_of[c] = (uint32_t)g;
        }
        const size_t G = nb->sizes.size();
        std::vector<std::vector<int32_t>> bins(G);
        std::vector<uint32_t> local(n_keep);
        for (size_t c = 0; c < n_keep; ++c) {
            const uint32_t ob = b->band_of[keep[c]];
            const int32_t lo = b->bins[2 * ob], hi = b->bins[2 * ob + 1];
            std::vector<int32_t>& bg = bins[size_of[c]];
            size_t j = 0;
            while (j < bg.size() / 2 && !(bg[2 * j] == lo && bg[2 * j + 1] == hi)) ++j;
            if (j == bg.size() / 2) { bg.push_back(lo); bg.push_back(hi); }
            local[c] = (uint32_t)j;
        }
        std::vector<uint32_t> first(G);
        for (size_t g = 0; g < G; ++g) {
            first[g] = (uint32_t)(nb->bins.size() / 2);
            nb->bins.insert(nb->bins.end(), bins[g].begin(), bins[g].end());
            nb->size_of_band.insert(nb->size_of_band.end(), bins[g].size() / 2, (uint32_t)g);
        }
        nb->band_of.resize(n_keep);
        for (size_t c = 0; c < n_keep; ++c) nb->band_of[c] = first[size_of[c]] + local[c];
        nb->size_of = std::move(size_of);
        nb->sample_rate = b->sample_rate; nb->n_channels = b->n_channels; nb->fft_size = nb->sizes[0]; nb->n_streams = S;
        nb->cfgs.resize(n_keep);
        for (size_t c = 0; c < n_keep; ++c) nb->cfgs[c] = b->cfgs[keep[c]];
        if (const int rc = derive_avg_keys(nb)) return rc; // (the survivors' keys in their first-seen order, as the bands above)
        if (const int rc = derive_trigger_keys(nb)) return rc;
        // per machine (stream s, config c) -> (s, keep[c])
        const size_t M = S * n_keep;
        nb->segs.resize(M);
        nb->audits.resize(M);
        nb->exact_evals.resize(M);
        nb->lazy_pushes.resize(M);
        if (b->scored) nb->scores.resize(M);
        for (size_t s = 0; s < S; ++s)
            for (size_t c = 0; c < n_keep; ++c) {
                const size_t m = s * n_keep + c, o = s * NC + keep[c];
                nb->audits[m] = b->audits[o];
                nb->exact_evals[m] = b->exact_evals[o];
                nb->lazy_pushes[m] = b->lazy_pushes[o];
                if (b->scored) nb->scores[m] = b->scores[o];
            }
        if (!b->machines.empty()) nb->machines.resize(M);
        if (b->has_refs) {
            nb->refs = b->refs;
            nb->ref_pmax = b->ref_pmax;
            nb->ref_off = b->ref_off;
            nb->stat_cfgs.resize(n_keep);
            for (size_t c = 0; c < n_keep; ++c) nb->stat_cfgs[c] = b->stat_cfgs[keep[c]];
        }
    } catch (const std::bad_alloc&) {
        return FVAD_ERR_ALLOC_FAILED;
    }
    nb->has_refs = b->has_refs;
    nb->scored = b->scored;
    nb->keep_segments = b->keep_segments;
    nb->segs_kept = b->segs_kept;
    nb->next_sample = b->next_sample;
    nb->chain_form = b->chain_form;
    nb->state_on_device = b->state_on_device;
    nb->avgs_form = b->avgs_form;
    nb->avgs_bytes = b->avgs_bytes;
    nb->trigger_form = b->trigger_form;
    nb->trigger_bytes = b->trigger_bytes;
    nb->trig_machine_launches = b->trig_machine_launches;
    nb->trig_finish_launches = b->trig_finish_launches;
    return FVAD_OK;
}

void retain_commit(fvad_vad_batch* b, const uint32_t* keep, size_t n_keep, fvad_vad_batch* nb)
{
    const size_t NC = b->cfgs.size();
    for (size_t s = 0; s < b->n_streams; ++s)
        for (size_t c = 0; c < n_keep; ++c) {
            nb->segs[s * n_keep + c] = std::move(b->segs[s * NC + keep[c]]);
            if (!nb->machines.empty()) nb->machines[s * n_keep + c] = std::move(b->machines[s * NC + keep[c]]);
        }
    if (!nb->dev_parts) nb->dev_parts = std::move(b->dev_parts); // (else nb holds the compacted device state: b's is freed here)
    *b = std::move(*nb);
}

} // namespace fvad

namespace fvad {
// The volume ratio of every FFT frame of a stream (BufferedVolumeAnalyzer.zig:48-69 per chunk, the two metadata hand-overs
// BufferedVolumeAnalyzer.zig:33-45 / BufferedDenoiser.zig:83-86,115, the sample-weighted frame ratio BufferedFFT.zig:137-140,153).
// Frames [first_frame, first_frame + n_frames); chunk_rms(c, k) = channel c's RMS of chunk first_chunk + k.  Every frame
// covers at least one chunk, so every frame has a ratio (has[f] = 1; the flag is still carried, not inferred from the value: a
// NaN ratio from NaN audio is a ratio, pushed as it is).
template <class Rms>
static void frame_ratios(Rms chunk_rms, size_t C, size_t n_chunks, size_t n_frames, uint64_t first_frame, uint64_t first_chunk,
                         size_t fft_size, size_t chunk_size, float* out, uint8_t* has)
{
    // the arithmetic is vad_ratio.h's (the device computes the same frames from the same header, kernels_vadratio.hip)
    std::vector<float> ratio(n_chunks);
    for (size_t k = 0; k < n_chunks; ++k)
        ratio[k] = chunk_volume_ratio([&](size_t c) { return chunk_rms(c, k); }, C, (float)chunk_size);
    for (size_t f = 0; f < n_frames; ++f) {
        out[f] = frame_volume_ratio([&](uint64_t k) { return ratio[(size_t)(k - first_chunk)]; }, (first_frame + f) * fft_size, fft_size, chunk_size);
        if (has) has[f] = 1;
    }
}

void sweep_frame_ratios(const float* chunk_rms, size_t rms_stride, size_t C, size_t n_chunks, size_t n_frames, size_t fft_size,
                        size_t chunk_size, float* out, uint64_t first_frame)
{
    frame_ratios([&](size_t c, size_t k) { return chunk_rms[c * rms_stride + k]; }, C, n_chunks, n_frames, first_frame,
                 first_frame * fft_size / chunk_size, fft_size, chunk_size, out, nullptr);
}

} // namespace fvad

extern "C" {

int fvad_vad_batch_frame_ratios(const fvad_vad_batch* b, const float* chunk_rms, size_t rms_stride, const size_t* n_frames,
                                const size_t* n_chunks, size_t chunk_size, uint64_t first_sample, float* ratio, size_t ratio_stride)
{
    if (!b || !n_frames || !n_chunks || chunk_size == 0) return FVAD_ERR_INVALID_ARGUMENT;
    if (first_sample % chunk_size) return FVAD_ERR_INVALID_ARGUMENT;
    const size_t S = b->n_streams, C = b->n_channels, G = b->sizes.size();
    for (size_t g = 0; g < G; ++g) {
        if (first_sample % b->sizes[g]) return FVAD_ERR_INVALID_ARGUMENT;
        for (size_t s = 0; s < S; ++s) {
            const size_t nf = n_frames[g * S + s];
            if (nf > (n_chunks[s] * chunk_size) / b->sizes[g] || nf > ratio_stride || n_chunks[s] > rms_stride) return FVAD_ERR_INVALID_ARGUMENT;
            if (nf && (!chunk_rms || !ratio)) return FVAD_ERR_INVALID_ARGUMENT;
        }
    }
    for (size_t i = 0; i < G * S; ++i) {
        const size_t s = i % S, F = b->sizes[i / S];
        fvad::sweep_frame_ratios(chunk_rms + s * C * rms_stride, rms_stride, C, n_chunks[s], n_frames[i], F, chunk_size, ratio + i * ratio_stride,
                                 first_sample / F);
    }
    return FVAD_OK;
}

} // extern "C"

// Every machine of b over frames of its own size: n_frames[g] frames of size g from sample first_sample on (every stream the same
// length), band blocks as fvad_vad_batch_bands lists them.  The part rules are fvad_vad_batch_run_part's, in samples.
static int run_host(fvad_vad_batch* b, const float* band, size_t band_stride, const size_t* n_frames, const float* chunk_rms,
                    size_t rms_stride, size_t n_chunks, size_t chunk_size, uint64_t first_sample, int n_threads)
{
    const size_t NC = b->cfgs.size(), G = b->sizes.size();
    if (b->part_in_flight) return FVAD_ERR_INVALID_ARGUMENT; // (a device part in flight: fvad_vad_batch_part_wait first)
    // parts follow each other without gaps, and a part starts where a chunk and a frame of every size start (its first chunk is
    // chunk_rms' first column)
    if (first_sample != 0 && (first_sample != b->next_sample || b->machines.size() != b->n_streams * NC)) return FVAD_ERR_INVALID_ARGUMENT;
    if (first_sample % chunk_size) return FVAD_ERR_INVALID_ARGUMENT;
    for (size_t g = 0; g < G; ++g) {
        if (first_sample % b->sizes[g]) return FVAD_ERR_INVALID_ARGUMENT;
        if (n_frames[g] * b->sizes[g] > n_chunks * chunk_size) return FVAD_ERR_INVALID_ARGUMENT; // a frame without its chunk's ratio
    }
    const uint64_t first_chunk = first_sample / chunk_size;
    const size_t C = b->n_channels, n_lanes = b->n_streams * C;
    if (first_sample == 0) { // fresh machines (VADMachine.init per pipeline, VADPipeline.zig:60-75); machine s * NC + c
        b->dev_parts.reset(); // (a device run in parts cannot go on after a host run)
        b->machines.clear();
        for (size_t s = 0; s < b->n_streams; ++s)
            for (size_t c = 0; c < NC; ++c)
                b->machines.emplace_back(new fvad::VadMachine(b->cfgs[c], b->sample_rate, C, b->sizes[b->size_of[c]]));
    }
    auto run_machine = [&](size_t s, size_t c, const float* ratio, const uint8_t* has) {
        fvad::VadMachine& m = *b->machines[s * NC + c];
        const size_t F = b->sizes[b->size_of[c]], nf = n_frames[b->size_of[c]];
        const uint64_t first_frame = first_sample / F;
        const float* bb = band + ((size_t)b->band_of[c] * n_lanes + s * C) * band_stride; // config c's band block, stream s's lanes
        std::vector<float> vols(C);
        for (size_t f = 0; f < nf; ++f) {
            for (size_t ch = 0; ch < C; ++ch) vols[ch] = bb[ch * band_stride + f];
            m.run((first_frame + f) * F, vols.data(), has[f] != 0, ratio[f]);
        }
        m.next_index = (first_frame + nf) * F;
        b->segs[s * NC + c] = m.segments; // (everything so far: a segment is appended when it closes)
        b->audits[s * NC + c] = m.audit;
        b->exact_evals[s * NC + c] = m.exact_evals;
        b->lazy_pushes[s * NC + c] = m.lazy_pushes;
    };
    auto stream_ratios = [&](size_t g, size_t s, float* out, uint8_t* has) {
        const size_t F = b->sizes[g];
        fvad::frame_ratios([&](size_t c, size_t k) { return chunk_rms[(s * C + c) * rms_stride + k]; }, C, n_chunks, n_frames[g],
                           first_sample / F, first_chunk, F, chunk_size, out, has);
    };
    if (NC == 1) {
        // one machine per stream: a stream's frame ratios and its machine on the same thread
        fvad::deal(b->n_streams, n_threads, [&](size_t s) {
            std::vector<float> ratio(n_frames[0]);
            std::vector<uint8_t> has(n_frames[0]);
            stream_ratios(0, s, ratio.data(), has.data());
            run_machine(s, 0, ratio.data(), has.data());
        });
    } else {
        // a sweep: the frame ratios of every (size, stream) (they do not depend on the config), then every (stream, config) machine
        size_t rs = 0;
        for (size_t g = 0; g < G; ++g) rs = std::max(rs, n_frames[g]);
        const size_t S = b->n_streams;
        std::vector<float> ratio(G * S * rs);
        std::vector<uint8_t> has(G * S * rs);
        fvad::deal(G * S, n_threads, [&](size_t i) { stream_ratios(i / S, i % S, ratio.data() + i * rs, has.data() + i * rs); });
        fvad::deal(S * NC, n_threads, [&](size_t i) {
            const size_t row = ((size_t)b->size_of[i % NC] * S + i / NC) * rs;
            run_machine(i / NC, i % NC, ratio.data() + row, has.data() + row);
        });
    }
    b->next_sample = first_sample + n_frames[0] * b->sizes[0];
    for (size_t g = 1; g < G; ++g)
        if (first_sample + n_frames[g] * b->sizes[g] != b->next_sample) b->next_sample = UINT64_MAX; // (the sizes ended apart)
    b->segs_kept = true;
    b->state_on_device = false;
    b->scored = false; // the scores were of the previous segments
    return FVAD_OK;
}

extern "C" {

int fvad_vad_batch_run_part(fvad_vad_batch* b, const float* band, size_t band_stride, size_t n_frames, const float* chunk_rms,
                            size_t rms_stride, size_t n_chunks, size_t chunk_size, uint64_t first_frame, int n_threads)
{
    if (!b || (n_frames && !band) || (n_chunks && !chunk_rms) || chunk_size == 0) return FVAD_ERR_INVALID_ARGUMENT;
    if (b->sizes.size() != 1) return FVAD_ERR_INVALID_ARGUMENT; // (several frame sizes: fvad_vad_batch_run_sized)
    if (first_frame > UINT64_MAX / b->fft_size) return FVAD_ERR_INVALID_ARGUMENT;
    return run_host(b, band, band_stride, &n_frames, chunk_rms, rms_stride, n_chunks, chunk_size, first_frame * b->fft_size, n_threads);
}

int fvad_vad_batch_run(fvad_vad_batch* b, const float* band, size_t band_stride, size_t n_frames, const float* chunk_rms,
                       size_t rms_stride, size_t n_chunks, size_t chunk_size, int n_threads)
{
    return fvad_vad_batch_run_part(b, band, band_stride, n_frames, chunk_rms, rms_stride, n_chunks, chunk_size, 0, n_threads);
}

int fvad_vad_batch_run_sized(fvad_vad_batch* b, const float* band, size_t band_stride, const size_t* n_frames, const float* chunk_rms,
                             size_t rms_stride, size_t n_chunks, size_t chunk_size, uint64_t first_sample, int n_threads)
{
    if (!b || !n_frames || (n_chunks && !chunk_rms) || chunk_size == 0) return FVAD_ERR_INVALID_ARGUMENT;
    for (size_t g = 0; g < b->sizes.size(); ++g)
        if ((n_frames[g] && !band) || band_stride < n_frames[g]) return FVAD_ERR_INVALID_ARGUMENT;
    return run_host(b, band, band_stride, n_frames, chunk_rms, rms_stride, n_chunks, chunk_size, first_sample, n_threads);
}

size_t fvad_vad_batch_total_segments(const fvad_vad_batch* b) // (config 0's on a sweep batch)
{
    if (b && (!b->segs_kept || b->part_in_flight)) return SIZE_MAX; // a device run without keeping its segments, or a part in flight
    size_t n = 0;
    if (b) for (size_t s = 0; s < b->n_streams; ++s) n += b->segs[s * b->cfgs.size()].size();
    return n;
}

int fvad_vad_batch_segments(const fvad_vad_batch* b, fvad_speech_segment* out, size_t cap, size_t* offsets)
{
    return fvad_vad_batch_config_segments(b, 0, out, cap, offsets);
}

int fvad_vad_batch_config_segments(const fvad_vad_batch* b, size_t config, fvad_speech_segment* out, size_t cap, size_t* offsets)
{
    if (!b || !offsets || config >= b->cfgs.size()) return FVAD_ERR_INVALID_ARGUMENT;
    if (!b->segs_kept || b->part_in_flight) return FVAD_ERR_INVALID_ARGUMENT; // a device run without keeping its segments: none to give; a part in flight
    const size_t NC = b->cfgs.size();
    size_t n = 0;
    for (size_t s = 0; s < b->n_streams; ++s) { offsets[s] = n; n += b->segs[s * NC + config].size(); }
    offsets[b->n_streams] = n;
    if (cap < n) return FVAD_ERR_BUFFER_TOO_SMALL;
    if (n && !out) return FVAD_ERR_INVALID_ARGUMENT;
    for (size_t s = 0; s < b->n_streams; ++s) {
        const auto& v = b->segs[s * NC + config];
        if (!v.empty()) memcpy(out + offsets[s], v.data(), v.size() * sizeof(fvad_speech_segment));
    }
    return FVAD_OK;
}

int fvad_vad_batch_hold_from(const fvad_vad_batch* b, size_t config, uint64_t* hold_from)
{
    if (!b || !hold_from || config >= b->cfgs.size() || b->part_in_flight) return FVAD_ERR_INVALID_ARGUMENT;
    if (b->state_on_device) return FVAD_ERR_INVALID_ARGUMENT; // after a device run the machines' state is not on the host
    const size_t NC = b->cfgs.size();
    for (size_t s = 0; s < b->n_streams; ++s) {
        if (b->machines.empty()) { hold_from[s] = 0; continue; } // nothing has run
        const fvad::VadMachine& m = *b->machines[s * NC + config];
        // a closed machine's next segment starts at the next frame at the earliest, less its pre-roll; an opening, open or closing
        // one has fixed its speech_start, and sample_from with it (vad_machine.h)
        hold_from[s] = fvad::offset_start(m.cf, m.state == fvad::VadMachineState::CLOSED ? m.next_index : m.speech_start);
    }
    return FVAD_OK;
}

int fvad_vad_batch_audit(const fvad_vad_batch* b, size_t stream, fvad_vad_audit* out)
{
    return fvad_vad_batch_config_audit(b, stream, 0, out);
}

int fvad_vad_batch_lazy_stats(const fvad_vad_batch* b, size_t stream, size_t config, uint64_t* exact_evaluations, uint64_t* lazy_pushes)
{
    if (!b || stream >= b->n_streams || config >= b->cfgs.size() || b->part_in_flight) return FVAD_ERR_INVALID_ARGUMENT;
    if (exact_evaluations) *exact_evaluations = b->exact_evals[stream * b->cfgs.size() + config];
    if (lazy_pushes) *lazy_pushes = b->lazy_pushes[stream * b->cfgs.size() + config];
    return FVAD_OK;
}

int fvad_vad_batch_config_audit(const fvad_vad_batch* b, size_t stream, size_t config, fvad_vad_audit* out)
{
    if (!b || !out || stream >= b->n_streams || config >= b->cfgs.size() || b->part_in_flight) return FVAD_ERR_INVALID_ARGUMENT;
    *out = b->audits[stream * b->cfgs.size() + config];
    return FVAD_OK;
}

} // extern "C"
