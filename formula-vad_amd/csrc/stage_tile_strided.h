// stage_tile_strided.h -- every step-th f32 of a run staged COMPACTED through LDS once, by a workgroup of kStageThreads lanes
// (kernels_egress_resample.hip, egress_strided_kernel: a tile's window of a stream that lies `step` apart in its lane).  stage_tile's sibling for a
// source of which only one sample in `step` is wanted.
#pragma once
#include "stage_tile.h"

// n (1 .. the tile) samples p[0], p[step], ..., p[(n - 1) step] into lds[0 .. n).  One dword load per sample, lane l of the
// workgroup the samples l, l + 256, ...: only the on-stride samples are read at all, so no byte outside the span from the first
// to the last of them is read and no other sample can reach LDS.  (n - 1) step < 2^17 (n <= 8192, step <= 16): 32-bit.  The
// LDS writes are consecutive words: conflict-free.  Ends with a barrier.
__device__ inline void stage_tile_strided(const float* __restrict__ p, int n, uint32_t step, float* lds)
{
    for (int i = threadIdx.x; i < n; i += kStageThreads) lds[i] = p[(uint32_t)i * step];
    __syncthreads();
}
