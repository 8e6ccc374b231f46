// fftgen_device.h -- the generic mixed-radix transform of kernels_fftgen.hip as device functions, for the kernels that run it
// inside a larger workgroup program (kernels_fftgen.hip: one frame per workgroup; kernels_clips_mel.hip: frame after frame of a
// staged tile).  Workgroups of 256 lanes; see kernels_fftgen.hip for the scheme.
#pragma once
#include "fft_device.h"

__device__ __forceinline__ void generic_cfft(cpx* a, cpx* b, int M, const VadFftPlan& pl, bool inverse, cpx*& result)
{
    const int tid = threadIdx.x;
    int Ns = 1;
    cpx* src = a;
    cpx* dst = b;
    for (int f = 0; f < pl.n_fac; ++f) {
        const int R = pl.fac[f];
        const int span = M / R;             // inputs of one output: src[j + r span]
        const int tstep = M / (Ns * R);     // table stride of the pass
        for (int o = tid; o < M; o += 256) {
            const int q = o / span, j = o - q * span;
            const int k = j % Ns;
            const int stride = (int)(((long long)(k + q * Ns) * tstep) % M);
            cpx acc = {0.0f, 0.0f};
            int idx = 0;
            if (R <= 5) {
                for (int r = 0; r < R; ++r) {
                    const cpx x = src[j + r * span];
                    const float wr = pl.tw[2 * idx], wi = inverse ? -pl.tw[2 * idx + 1] : pl.tw[2 * idx + 1];
                    acc.r += x.r * wr - x.i * wi;
                    acc.i += x.r * wi + x.i * wr;
                    idx += stride;
                    if (idx >= M) idx -= M;
                }
            } else {
                // a long direct sum (a prime radix such as 127): accumulated in double, so that its round-off stays at the
                // level of the short butterflies' (kissfft's generic butterfly sums in f32 in another order; both are
                // compared with the oracle at 1e-4 of bins that may be 1e-3 of the frame's largest)
                double ar = 0.0, ai = 0.0;
                for (int r = 0; r < R; ++r) {
                    const cpx x = src[j + r * span];
                    const double wr = pl.tw[2 * idx], wi = inverse ? -pl.tw[2 * idx + 1] : pl.tw[2 * idx + 1];
                    ar += (double)x.r * wr - (double)x.i * wi;
                    ai += (double)x.r * wi + (double)x.i * wr;
                    idx += stride;
                    if (idx >= M) idx -= M;
                }
                acc = {(float)ar, (float)ai};
            }
            dst[(j / Ns) * Ns * R + k + q * Ns] = acc;
        }
        __syncthreads();
        Ns *= R;
        cpx* t = src; src = dst; dst = t;
    }
    result = src;
}

// forward: frame (n samples) x window -> X[0 .. n/2] in `X` (LDS, M + 1 entries)
__device__ __forceinline__ void generic_rfft(const float* __restrict__ x, const float* __restrict__ win, const VadFftPlan& pl, cpx* bufA, cpx* bufB, cpx*& X)
{
    const int M = pl.n / 2;
    for (int j = threadIdx.x; j < M; j += 256) bufA[j] = {x[2 * j] * win[2 * j], x[2 * j + 1] * win[2 * j + 1]};
    __syncthreads();
    cpx* F;
    generic_cfft(bufA, bufB, M, pl, false, F);
    cpx* out = F == bufA ? bufB : bufA;
    // kiss_fftr's un-mixing (k and M - k together; at k == M - k the X[M - k] form is the one written last)
    for (int k = threadIdx.x; k <= M / 2; k += 256) {
        if (k == 0) {
            out[0] = {F[0].r + F[0].i, 0.0f};
            out[M] = {F[0].r - F[0].i, 0.0f};
        } else {
            cpx xk, xnk;
            unmix_fwd(F[k], F[M - k], {pl.st[2 * (k - 1)], pl.st[2 * (k - 1) + 1]}, xk, xnk);
            if (k != M - k) out[k] = xk;
            out[M - k] = xnk;
        }
    }
    __syncthreads();
    X = out;
}
