// vad_finish.h -- the second stage of a shared-trigger sweep (context option vad_trigger "shared"): the part of a VAD machine that
// follows `threshold_met` (VADMachine.zig:186-309: the four-state machine, trackSpeechStats, onSpeechEnd), walked over the bits a
// trigger machine emitted.  The trigger -- the rolling averages, the long-term chain, decide -- reads none of
// min_consecutive_sec_to_open, max_speech_gap_sec and min_vad_duration_sec and nothing flows back into it from the state machine,
// so one trigger serves every config that differs in those three fields only.  Shared by the finishing kernel
// (kernels_vadfinish.hip) and the host (fvad_vad_finish_bits): the same walk, the same finish_step (vad_machine.h), the same bits.
//
// Bits: bit k % 64 of word k / 64 is threshold_met of frame k of the part (parts start on chunk boundaries: words are relative to
// the part, not to the stream); bits past the part's last frame are never read.
#pragma once
#include "vad_machine.h"

namespace fvad {

// Frames [k0, n_frames) of a part whose frame k is at sample first_sample + k * F: word(w) gives word w of the bits, ratio(k) the
// frame's volume ratio, room() whether a segment closed by the next frame has a place, sink(segment) takes a closed segment.
// Returns the first frame not run: n_frames, or the frame before which room() said no.
// While the machine is CLOSED a frame whose bit is clear changes nothing (finish_step: CLOSED and !met is the identity and returns
// NONE), so the walk jumps to the next set bit -- a zero word costs one test.  Every other frame is finish_step as it is, one
// after the other, so the f32 sums keep their per-frame order.
template <class Word, class Ratio, class Room, class Sink>
FVAD_HD inline uint64_t finish_walk(VadMachineState& m, const VadMachineCfg& cf, uint64_t k0, uint64_t n_frames, uint64_t first_sample,
                                    uint64_t F, Word&& word, Ratio&& ratio, Room&& room, Sink&& sink)
{
    uint64_t k = k0;
    while (k < n_frames) {
        const uint64_t left = n_frames - k, in_word = 64 - (k & 63);
        const uint64_t n = left < in_word ? left : in_word; // frames of this word from k on
        uint64_t w = word(k >> 6) >> (k & 63);
        if (n < 64) w &= (1ull << n) - 1; // (what lies past the part's last frame is not the part's)
        const uint64_t end = k + n;
        while (k < end) {
            if (m.state == VadMachineState::CLOSED) {
                if (w == 0) { k = end; break; }
                const int z = __builtin_ctzll(w);
                k += (uint64_t)z;
                w >>= z;
            }
            if (!room()) return k;
            m.finish_step(cf, first_sample + k * F, (w & 1) != 0, true, ratio(k), sink);
            ++k;
            w >>= 1;
        }
    }
    return k;
}

// words a part of n_frames frames has
FVAD_HD inline uint64_t finish_words(uint64_t n_frames) { return (n_frames + 63) / 64; }

} // namespace fvad
