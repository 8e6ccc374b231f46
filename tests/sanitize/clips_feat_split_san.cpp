// clips_feat_split_san.cpp -- fvad_clips_split_mel_check and fvad_clips_split_fbank_check (csrc/host_clips_features.cpp, host only)
// under AddressSanitizer + UBSan: seeded random split rows, buffers and frame parameters, with values near UINT64_MAX for the
// overflow paths of the lengths' sum, the pieces' ranges and the buffers' byte ranges.  Whatever a check accepts must have every
// piece inside its buffer -- restated with 128-bit arithmetic --, the output beside both sources, and the frame counts, slots and
// total that the family's plan gives for lens[i] = a_len + b_len; a refusal is one of the three statuses the rules name; nothing
// is written past n_clips.  Built by tests/test_sanitizers_clips_feat_split.py; never loaded into Python.
//   usage: clips_feat_split_san <seed>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fvad.h"

typedef unsigned __int128 u128;

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: clips_feat_split_san <seed>\n"); return 2; }
    std::mt19937_64 rng((uint64_t)atoll(argv[1]));
    auto pick = [&](uint64_t n) { return n ? (uint64_t)(rng() % n) : 0; }; // (a range that wrapped to 0 gives 0)
    auto near_max = [&]() -> uint64_t {
        switch (pick(6)) {
        case 0: return UINT64_MAX - pick(40);
        case 1: return (UINT64_MAX >> pick(9)) + pick(3);
        case 2: return (1ull << 63) + pick(5) - 2;
        default: return pick(200);
        }
    };
    long tables = 0, ok = 0, invalid = 0, range = 0, small = 0;
    for (int round = 0; round < 4000; ++round) {
        const bool fbank = pick(2) == 1, wild = pick(4) == 0;
        const size_t n = 1 + (size_t)pick(6);
        const uint32_t step = pick(25) == 0 ? 0 : 1 + (uint32_t)pick(FVAD_CLIP_STEP_MAX);
        const uint32_t n_fft = pick(25) == 0 ? 7 : 2 * (2 + (uint32_t)pick(pick(2) ? 8 : 300));
        const uint32_t win = fbank ? (pick(25) == 0 ? n_fft + 1 : 2 + (uint32_t)pick(n_fft - 1)) : n_fft;
        const uint32_t hop = pick(25) == 0 ? win + 1 : 1 + (uint32_t)pick(win ? win : 1);
        const uint32_t n_mels = pick(25) == 0 ? 0 : 1 + (uint32_t)pick(FVAD_CLIP_MEL_BANDS_MAX);
        const int fmt = pick(20) == 0 ? 3 : (int)pick(2);
        const uint64_t sb = fmt == FVAD_CLIP_PCM16 ? 2 : 4;
        // two buffers far apart and an output behind both; sometimes the output inside one of them
        const uint64_t a_lanes = 3 + pick(3), b_lanes = 3 + pick(3);
        const uint64_t a_samples = wild && pick(3) == 0 ? near_max() : 2000 + pick(60000), b_samples = wild && pick(3) == 0 ? near_max() : 2000 + pick(60000);
        const uint64_t a_stride = pick(20) == 0 ? a_samples / 2 : a_samples + pick(9), b_stride = pick(20) == 0 ? b_samples / 2 : b_samples + pick(9);
        const uint64_t d_a = 0x100000 + sb * pick(8) + (pick(30) == 0 ? 1 : 0), d_b = (1ull << 40) + sb * pick(8);
        const uint64_t out = pick(15) == 0 ? d_a + 16 * pick(50) : pick(15) == 0 ? d_b + 16 * pick(50) : (1ull << 50) + (pick(20) == 0 ? 4 : 0);
        std::vector<uint64_t> rows((n + 1) * FVAD_CLIP_SPLIT_FIELDS, 0), lens(n), frames(n + 1, 77), offsets(n + 1, 77), pf(n + 1), po(n + 1);
        std::vector<uint32_t> skips(n + 1, 0);
        bool pieces_ok = true, rows_ok = true;
        for (size_t i = 0; i < n; ++i) {
            uint64_t* r = &rows[i * FVAD_CLIP_SPLIT_FIELDS];
            const uint64_t need = (uint64_t)(win ? win : 1) * (step ? step : 1) + 1 + pick(3000);
            r[0] = pick(30) == 0 ? 0 : 1 + pick(3);                                   // n_channels
            r[3] = wild && pick(4) == 0 ? near_max() : pick(5) == 0 ? 0 : pick(need);   // a_len
            r[6] = wild && pick(4) == 0 ? near_max() : pick(40) == 0 ? 0 : need - (r[3] < need ? r[3] : need) + pick(50);
            r[1] = pick(15) == 0 ? pick(a_lanes + 1) : pick(a_lanes - r[0] + 1); r[4] = pick(15) == 0 ? pick(b_lanes + 1) : pick(b_lanes - r[0] + 1);
            r[2] = wild && pick(6) == 0 ? near_max() : pick(a_samples > r[3] ? a_samples - r[3] + (pick(12) == 0 ? 5 : 1) : 3);
            r[5] = wild && pick(6) == 0 ? near_max() : pick(b_samples > r[6] ? b_samples - r[6] + (pick(12) == 0 ? 5 : 1) : 3);
            skips[i] = step ? (uint32_t)pick(step + (pick(25) == 0)) : 0;
            const u128 len = (u128)r[3] + r[6];
            rows_ok = rows_ok && r[0] != 0 && len != 0 && len <= UINT64_MAX;
            lens[i] = (uint64_t)len;
            if (r[3] && ((u128)r[2] + r[3] > a_samples || r[1] >= a_lanes || r[0] > a_lanes - r[1])) pieces_ok = false;
            if (r[6] && ((u128)r[5] + r[6] > b_samples || r[4] >= b_lanes || r[0] > b_lanes - r[4])) pieces_ok = false;
        }
        std::vector<float> window(win ? win : 1, 0.5f), matrix((size_t)(n_mels ? n_mels : 1) * (n_fft / 2 + 1), 0.25f); // (exactly the values the rules read)
        const bool bad_value = pick(40) == 0;
        if (bad_value) matrix[pick(matrix.size())] = INFINITY;
        const float norm[3] = {8.0f, 4.0f, 0.25f};
        const uint64_t cap = pick(12) == 0 ? pick(2000) : UINT64_MAX >> 3;
        const bool null_skips = pick(6) == 0;
        const uint32_t* sk = null_skips ? nullptr : skips.data();
        uint64_t total = 99, plan_total = 99;
        int rc, rp;
        if (fbank) {
            rc = fvad_clips_split_fbank_check((const void*)d_a, a_lanes, a_stride, a_samples, (const void*)d_b, b_lanes, b_stride, b_samples, fmt, rows.data(), n,
                                              FVAD_CLIP_F32, (const void*)out, cap, 1, step, sk, win, n_fft, hop, window.data(), n_mels, matrix.data(), 32768.0f,
                                              0.97f, (int)pick(2), 1.1920929e-07f, (int)pick(2), frames.data(), offsets.data(), &total);
            rp = fvad_clips_plan_fbank(lens.data(), sk, n, step, win, hop, n_mels, pf.data(), po.data(), &plan_total);
        } else {
            rc = fvad_clips_split_mel_check((const void*)d_a, a_lanes, a_stride, a_samples, (const void*)d_b, b_lanes, b_stride, b_samples, fmt, rows.data(), n,
                                            FVAD_CLIP_F32, (const void*)out, cap, 1, step, sk, n_fft, hop, window.data(), n_mels, matrix.data(), 1e-10f,
                                            pick(2) ? norm : nullptr, frames.data(), offsets.data(), &total);
            rp = fvad_clips_plan_mel(lens.data(), sk, n, step, n_fft, hop, n_mels, pf.data(), po.data(), &plan_total);
        }
        ++tables;
        if (frames[n] != 77 || offsets[n] != 77) { fprintf(stderr, "written past n_clips (round %d)\n", round); return 9; }
        if (rc == FVAD_OK) {
            if (!rows_ok || !pieces_ok || bad_value || rp != FVAD_OK || total != plan_total || total > cap || fmt > 1 || out % 16 != 0 || d_a % sb != 0) {
                fprintf(stderr, "an accepted call breaks a rule (round %d)\n", round);
                return 8;
            }
            for (size_t i = 0; i < n; ++i)
                if (frames[i] != pf[i] || offsets[i] != po[i]) { fprintf(stderr, "the check's numbers are not the plan's (round %d)\n", round); return 8; }
            // the output beside the sources, by address
            const u128 o_lo = out, o_hi = (u128)out + (u128)total * 4;
            const u128 a_hi = (u128)d_a + ((u128)(a_lanes - 1) * (a_lanes > 1 ? a_stride : 0) + a_samples) * sb;
            const u128 b_hi = (u128)d_b + ((u128)(b_lanes - 1) * (b_lanes > 1 ? b_stride : 0) + b_samples) * sb;
            if (total && ((o_lo < a_hi && d_a < o_hi) || (o_lo < b_hi && d_b < o_hi))) { fprintf(stderr, "an accepted output overlaps a source (round %d)\n", round); return 8; }
            ++ok;
        } else if (rc == FVAD_ERR_INVALID_ARGUMENT) {
            ++invalid;
        } else if (rc == FVAD_ERR_OUT_OF_RANGE) {
            if (pieces_ok || rp != FVAD_OK) { fprintf(stderr, "out of range without a piece past its buffer, or in front of the family's rules (round %d)\n", round); return 8; }
            ++range;
        } else if (rc == FVAD_ERR_BUFFER_TOO_SMALL) {
            if (!pieces_ok || rp != FVAD_OK || plan_total <= cap) { fprintf(stderr, "too small in front of an earlier rule (round %d)\n", round); return 8; }
            ++small;
        } else {
            fprintf(stderr, "an unexpected status %d (round %d)\n", rc, round);
            return 6;
        }
    }
    if (ok < 200 || invalid < 200 || range < 50 || small < 20) {
        fprintf(stderr, "the driver is one-sided: ok %ld, invalid %ld, out of range %ld, too small %ld\n", ok, invalid, range, small);
        return 10;
    }
    printf("tables=%ld ok=%ld invalid=%ld out_of_range=%ld too_small=%ld\n", tables, ok, invalid, range, small);
    return 0;
}
