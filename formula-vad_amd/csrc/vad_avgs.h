// vad_avgs.h -- the short-term and channel-ratio rolling averages of a VAD machine as a function of the frame number alone.
//
// VADMachine.run pushes min_volume and the frame's volume ratio into two rings without an initial value whatever the machine
// decides (VADMachine.zig:166-167), so after frame n of a stream (n >= 0 from the stream's start) a ring of `len` slots holds
// inputs that n and len fix, and RollingAverage.avg (RollingAverage.zig:45-56) is the chain over its slots in slot order:
//   n + 1 < len (not yet full): slot i holds x[i], i = 0 .. n; the chain of (double)x[i] * (1.0 / (double)(n + 1)) from 0.0;
//   else, with w = n % len: slots 0 .. w hold x[n - w .. n], slots w + 1 .. len - 1 hold x[n - len + 1 .. n - w - 1]; the chain
//   of (double)slot * scalar from 0.0 over slots 0 .. len - 1 (scalar = 1 / len: VadMachineCfg's st_scalar / cr_scalar).
// These are the products and additions of kernels_vad.hip's Ring::push and of host_vad.cpp's prefix form, in their order (the
// library is built with -ffp-contract=off): the same bits.  Shared by the table kernel (kernels_vadavgs.hip), the table form of
// the machines' kernel (kernels_vad.hip) and the host's check of both (fvad_vad_avg_chain).
#pragma once
#include <stdint.h>

#include "vad_machine.h"

namespace fvad {

// The average after the push of frame n.  x(slot, frame) -> float: the input of `frame`, which the ring holds in `slot` (a
// caller that has only part of the stream reads the earlier frames from the ring as it was when its part began: slot `slot`).
template <class X>
FVAD_HD inline double ring_avg_at(uint64_t n, uint32_t len, double scalar, X&& x)
{
    double acc = 0.0;
    if (n + 1 < (uint64_t)len) {
        const double sc = 1.0 / (double)(n + 1);
        for (uint32_t i = 0; i <= (uint32_t)n; ++i) acc += (double)x(i, (uint64_t)i) * sc;
        return acc;
    }
    const uint32_t w = (uint32_t)(n % len);
    for (uint32_t i = 0; i <= w; ++i) acc += (double)x(i, n - w + i) * scalar;
    for (uint32_t i = w + 1; i < len; ++i) acc += (double)x(i, n - len + (i - w)) * scalar;
    return acc;
}

// What Ring::push leaves in a ring's cursors after `count` pushes since the stream's start: the write index, the written count
// (the prefix sum below the write index is the chain over slots [0, w) once the ring is full, else 0.0)
FVAD_HD inline uint32_t ring_w_after(uint64_t count, uint32_t len) { return (uint32_t)(count % len); }
FVAD_HD inline uint32_t ring_wc_after(uint64_t count, uint32_t len) { return count < (uint64_t)len ? (uint32_t)count : len; }

} // namespace fvad
