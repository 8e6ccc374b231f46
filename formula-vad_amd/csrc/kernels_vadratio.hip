// kernels_vadratio.hip -- the frame ratios of a device part from the chunk RMS the engine left on the device
// (fvad_vad_batch_frame_ratios_device, fvad_vad_batch_run_device_part_async): what sweep_frame_ratios (host_vad.cpp) computes on
// the host, by the same header (vad_ratio.h), so the same bits.
//
// One lane per frame, one row per (size g, stream s).  A frame of F samples overlaps at most ceil(F / chunk) + 1 chunks, so a
// lane's chain is short; each chunk's ratio is recomputed by the lanes that need it (n_channels loads and two divisions) rather
// than staged, since neighbouring frames read the same or the next chunk: a wavefront's loads of the lane-major RMS rows fall in
// one or two cache lines per channel, and its 64 stores are one 256-byte run of the row.
// Bounds: f < max_frames <= ratio_stride for the stores; a chunk is read only when its index is below the stream's n_chunks (the
// host has checked that every frame's chunks are: frame_counts, engine_sweep.cpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "vad_ratio.h"

// x: frames (grid-stride), y: rows (grid-stride)
__global__ __launch_bounds__(256) void vad_frame_ratios_kernel(VadRatioArgs a)
{
    const long rows = (long)a.n_sizes * a.n_streams;
    const uint64_t first_chunk = a.first_sample / a.chunk_size;
    const float chunk_size_f = (float)a.chunk_size;
    for (long i = blockIdx.y; i < rows; i += gridDim.y) {
        const long s = i % a.n_streams;
        const uint64_t F = a.sizes ? a.sizes[i / a.n_streams] : a.fft_size;
        const long nf = a.n_frames[i];
        const uint64_t nc = (uint64_t)a.n_chunks[s];
        const float* rms = a.chunk_rms + s * a.n_channels * a.rms_stride;
        float* out = a.ratio + i * a.ratio_stride;
        for (long f = (long)blockIdx.x * 256 + threadIdx.x; f < a.max_frames; f += (long)gridDim.x * 256) {
            float r = 0.0f; // (past the row's frames: what the host's zero-filled rows hold)
            if (f < nf)
                r = fvad::frame_volume_ratio(
                    [&](uint64_t k) {
                        const uint64_t rel = k - first_chunk;
                        if (rel >= nc) return 0.0f;
                        return fvad::chunk_volume_ratio([&](size_t c) { return rms[(long)c * a.rms_stride + (long)rel]; }, (size_t)a.n_channels,
                                                        chunk_size_f);
                    },
                    a.first_sample + (uint64_t)f * F, F, a.chunk_size);
            out[f] = r;
        }
    }
}

int fvad_launch_vad_frame_ratios(const VadRatioArgs& a, hipStream_t stream)
{
    const long rows = (long)a.n_sizes * a.n_streams;
    if (rows <= 0 || a.max_frames <= 0) return (int)hipSuccess;
    const unsigned gx = (unsigned)std::min<long>((a.max_frames + 255) / 256, 4096);
    const unsigned gy = (unsigned)std::min<long>(rows, 4096);
    hipLaunchKernelGGL(vad_frame_ratios_kernel, dim3(gx, gy), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}
