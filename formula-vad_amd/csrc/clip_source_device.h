// clip_source_device.h -- where a clip's samples are, stated once for every Recorder kernel (kernels_clips.hip,
// kernels_clips_strided.hip, kernels_clips_fir.hip, kernels_clips_resample.hip).  ClipSource<B> is over the arguments B of a
// source: ClipArgs, a clip's channel as one run, or ClipSplitArgs, a head piece in buffer A followed by a body piece in buffer B.
// Each gives the LDS elements a staged tile takes (lds_elems<S>()) and stage<S>(), which brings samples [e0, e0 + n) of a clip's
// channel into LDS, ends with the staging barrier and returns the functor from sample index within the tile to LDS index.  Every
// later read of the tile is through that functor, so a kernel body is written once and a split clip gives the bits of the same
// samples laid out contiguously, wherever the seam is.  Also here: the launch by format pair that every gather shares.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "stage_tile.h"

__host__ __device__ inline const ClipArgs& clip_args(const ClipArgs& a) { return a; }
__host__ __device__ inline const ClipArgs& clip_args(const ClipSplitArgs& a) { return a.c; }

template <typename B> struct ClipSource;

// One run.  clip starts are arbitrary sample indices, so the tile's first byte has any alignment: stage_tile reads the 16-byte
// aligned body strictly inside the tile with 16-byte loads, the elements in front of and behind it one by one -- no byte outside
// [sample_from, sample_to) is read -- and the LDS image keeps the global address's offset within 16 bytes (At::shift).
template <> struct ClipSource<ClipArgs> {
    struct At {
        int shift;
        __device__ int operator()(int e) const { return shift + e; }
    };
    template <typename S> static constexpr int lds_elems() { return kClipTile + 16 / (int)sizeof(S); }
    template <typename S>
    __device__ static At stage(const ClipArgs& a, uint32_t clip, uint32_t ch, uint64_t e0, int n, S* lds)
    {
        return {stage_tile(static_cast<const S*>(a.src) + a.jobs[clip].src_off + (uint64_t)ch * a.lane_stride + e0, n, lds)};
    }
};

// Two pieces.  A tile that lies wholly in one piece is staged as the contiguous source stages it.  The tile that holds the seam
// is staged as two runs, each by stage_tile with its own shift into its own 16-byte aligned LDS region: aligned bodies by
// 16-byte loads and stores, the elements in front of and behind them one by one, no byte outside either piece.  Tiles are
// counted from the clip's first sample, never from the seam, so strides and filters run through it.
template <> struct ClipSource<ClipSplitArgs> {
    struct At {
        int n1, off1, off2; // sample e of the tile is lds[off1 + e] for e < n1, else lds[off2 + e - n1]
        __device__ int operator()(int e) const { return e < n1 ? off1 + e : off2 + (e - n1); }
    };
    // run 1 ends below V - 1 + kClipTile, run 2 starts at the next multiple of V plus its own shift (< V): 3 V elements more
    // than the samples
    template <typename S> static constexpr int lds_elems() { return kClipTile + 3 * (16 / (int)sizeof(S)); }
    template <typename S>
    __device__ static At stage(const ClipSplitArgs& a, uint32_t clip, uint32_t ch, uint64_t e0, int n, S* lds)
    {
        constexpr int V = 16 / (int)sizeof(S);
        const ClipSplit sp = a.splits[clip];
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
};

// a gather by the call's format pair: launch(D{}, S{}, grid, block) starts the <D out, S src> instance of its kernel, one
// workgroup per gather tile
template <typename L>
inline int launch_clip_formats(const ClipArgs& c, L launch)
{
    const dim3 grid(c.n_tiles), block(kStageThreads);
    if (c.src_i16 && c.out_i16) launch(int16_t{}, int16_t{}, grid, block);
    else if (c.src_i16) launch(float{}, int16_t{}, grid, block);
    else if (c.out_i16) launch(int16_t{}, float{}, grid, block);
    else launch(float{}, float{}, grid, block);
    return (int)hipGetLastError();
}
