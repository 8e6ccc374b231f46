// stage_tile.h -- a run of elements with an arbitrary start staged through LDS once, by a workgroup of kStageThreads lanes
// (kernels_clips.hip: a tile of a clip; kernels_ingest.hip: a tile of a source's interleaved bytes).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int kStageThreads = 256;

// n (1 .. the tile) elements from p into lds[shift ..), shift = p's offset within 16 bytes in elements (returned).  lds holds
// the tile + 16 / sizeof(S) elements and is 16-byte aligned.  The 16-byte aligned body strictly inside [p, p + n) is read with
// 16-byte loads, the elements in front of and behind it one by one: no byte outside the run is read.  Ends with a barrier.
template <typename S>
__device__ inline int stage_tile(const S* __restrict__ p, int n, S* lds)
{
    constexpr int V = 16 / (int)sizeof(S);
    const int t = threadIdx.x;
    const int shift = (int)(((uintptr_t)p & 15) / sizeof(S));
    const int head = min(n, (V - shift) % V);
    const int nvec = (n - head) / V;
    const uint4* pv = reinterpret_cast<const uint4*>(p + head);
    uint4* lv = reinterpret_cast<uint4*>(lds + shift + head); // shift + head is 0 or V whenever nvec > 0
    for (int v = t; v < nvec; v += kStageThreads) lv[v] = pv[v];
    const int tail0 = head + nvec * V;
    if (t < head) lds[shift + t] = p[t];
    if (t < n - tail0) lds[shift + tail0 + t] = p[tail0 + t];
    __syncthreads();
    return shift;
}
