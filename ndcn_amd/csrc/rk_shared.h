// Device helpers shared by the solver panel kernels of rk.hip and adams_vc.hip: 16-byte panel accesses, the error ratio of
// misc.py:151-156 and the deterministic two-pass fp64 reduction (per-workgroup partials, one fixed-order finish).  One definition, so
// that a sum formed by either file is the same sequence of additions.
//
// Both files round every product and every sum on its own; the arithmetic below must not be contracted either.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace ndcn {

constexpr int kRedBlocks = 2048;       // partial sums per reduction (deterministic two-pass)

__device__ __forceinline__ float4 ld4(const float *p, int64_t i) { return reinterpret_cast<const float4 *>(p)[i]; }
__device__ __forceinline__ void st4(float *p, int64_t i, float4 v) { reinterpret_cast<float4 *>(p)[i] = v; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// block-level sum of two doubles; result valid in thread 0
__device__ __forceinline__ void block_sum2(double &a, double &b) {
    __shared__ double sa[4], sb[4];
    a = wave_sum(a);
    b = wave_sum(b);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sa[w] = a; sb[w] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = ((sa[0] + sa[1]) + sa[2]) + sa[3];
        b = ((sb[0] + sb[1]) + sb[2]) + sb[3];
    }
}

__device__ __forceinline__ float err_ratio_sq(float e, float a, float b, float rtol, float atol) {
    // misc.py:151-156: tol = atol + rtol * max(|y0|, |y1|); r = err / tol; r * r
    const float tol = atol + rtol * max_nan(fabsf(a), fabsf(b));
    const float r = e / tol;
    return r * r;
}

// fixed-order final sum of the per-block partials (pairs {partial[2 i], partial[2 i + 1]}), by ONE workgroup of 256 threads
__device__ __forceinline__ void reduce_finish(const double *__restrict__ partial, int n_partial, double *__restrict__ out, int accum) {
    double s = 0.0, bad = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += 256) { s += partial[2 * i]; bad += partial[2 * i + 1]; }
    block_sum2(s, bad);
    if (threadIdx.x == 0) { out[0] = accum ? out[0] + s : s; out[1] = accum ? out[1] + bad : bad; }
}

// grid of a reduction pass: at most kRedBlocks workgroups, grid-stride the rest
inline int red_grid(int64_t items) {
    int g = stream_grid(items, 256);
    return g > kRedBlocks ? kRedBlocks : g;
}

}  // namespace ndcn
