// clip_split_device.h -- the staging of a split clip's tile, shared by the split-source kernels (kernels_clips_split.hip,
// kernels_clips_strided.hip).  A tile that lies wholly in one piece is staged as kernels_clips.hip stages it.  The tile that holds
// the seam is staged as two runs, each by stage_tile with its own shift into its own 16-byte aligned LDS region: aligned bodies by
// 16-byte loads and stores, the elements in front of and behind them one by one, no byte outside either piece.  Every later read
// is by sample index within the tile (Staged::at).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "stage_tile.h"

// LDS elements of a tile staged as up to two runs: run 1 ends below V - 1 + kClipTile, run 2 starts at the next multiple of V
// plus its own shift (< V) -- 3 V elements more than the samples
template <typename S> constexpr int lds_elems() { return kClipTile + 3 * (16 / (int)sizeof(S)); }

struct Staged {
    int n1, off1, off2; // sample e of the tile is lds[off1 + e] for e < n1, else lds[off2 + e - n1]
    __device__ int at(int e) const { return e < n1 ? off1 + e : off2 + (e - n1); }
};

// samples [e0, e0 + n) of channel ch of a split clip into lds; ends with a barrier
template <typename S>
__device__ inline Staged stage_split(const ClipSplitArgs& a, const ClipSplit& sp, uint32_t ch, uint64_t e0, int n, S* lds)
{
    constexpr int V = 16 / (int)sizeof(S);
    const S* pa = static_cast<const S*>(a.c.src) + sp.a_off + (uint64_t)ch * a.c.lane_stride + e0;
    const S* pb = static_cast<const S*>(a.b) + sp.b_off + (uint64_t)ch * a.b_stride;
    if (e0 + (uint64_t)n <= sp.a_len) return {n, stage_tile(pa, n, lds), 0};             // wholly in A
    if (e0 >= sp.a_len) return {n, stage_tile(pb + (e0 - sp.a_len), n, lds), 0};           // wholly in B
    const int n1 = (int)(sp.a_len - e0);                                                   // the seam: 0 < n1 < n
    const int s1 = stage_tile(pa, n1, lds);
    const int base2 = (s1 + n1 + V - 1) / V * V;
    const int s2 = stage_tile(pb, n - n1, lds + base2);
    return {n1, s1, base2 + s2};
}
