// K *= m in place: the dropout factor of csrc/dropout.h as a streaming pass behind the launches that have no dropout epilogue
// (every route of ndcn_rhs_f32 / ndcn_rhs_rk_f32 but the narrow-panel one).  The mask depends on the flat element index alone, so
// the pass is one-dimensional: any n, any H, panels over 2^31 elements.
//   VEC   the panel is 16-byte aligned: a lane owns elements 4 q .. 4 q + 3 - ONE Philox call, one 16-byte load, one 16-byte store;
//         the n & 3 elements behind the last whole group take the scalar expression
//   else  a misaligned view: an element per lane (its own Philox call, word i & 3)
#include "kernels.h"

#pragma clang fp contract(off)

namespace ndcn {

typedef float dr_f32x4 __attribute__((ext_vector_type(4)));

template <bool VEC>
__global__ __launch_bounds__(256) void dropout_apply_kernel(float *__restrict__ K, int64_t n, DropArgs d) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int64_t n4 = n >> 2;
        dr_f32x4 *K4 = reinterpret_cast<dr_f32x4 *>(K);
        for (int64_t q = t0; q < n4; q += stride) {
            const Philox4 o = drop_words(d, q);
            dr_f32x4 v = K4[q];
            v.x = v.x * (o.w[0] >= d.thresh ? d.s : 0.f);
            v.y = v.y * (o.w[1] >= d.thresh ? d.s : 0.f);
            v.z = v.z * (o.w[2] >= d.thresh ? d.s : 0.f);
            v.w = v.w * (o.w[3] >= d.thresh ? d.s : 0.f);
            K4[q] = v;
        }
        for (int64_t i = 4 * n4 + t0; i < n; i += stride) K[i] = K[i] * drop_factor(d, i);
    } else {
        for (int64_t i = t0; i < n; i += stride) K[i] = K[i] * drop_factor(d, i);
    }
}

int drop_args(const ndcn_dropout *desc, DropArgs *out) {
    const float p = desc->p;
    if (!(p > 0.f && p < 1.f)) { set_error("dropout: p = %g outside (0, 1)", (double)p); return NDCN_EINVAL; }
    out->s = 1.0f / (1.0f - p);
    out->thresh = (uint32_t)(uint64_t)((double)p * 4294967296.0);          // floor: p < 1 in float32 keeps it below 2^32
    out->k0 = (uint32_t)(desc->seed & 0xffffffffu);
    out->k1 = (uint32_t)(desc->seed >> 32);
    out->e0 = (uint32_t)(desc->evaluation & 0xffffffffu);
    out->e1 = (uint32_t)(desc->evaluation >> 32);
    return NDCN_OK;
}

int dropout_apply_f32(float *K, int64_t n, const DropArgs &d, hipStream_t st) {
    if (n == 0) return NDCN_OK;
    ProfScope prof(PROF_STAGE, st, 8.0 * (double)n, 1.0 * (double)n);
    if (aligned16(K))
        hipLaunchKernelGGL(dropout_apply_kernel<true>, dim3(stream_grid_full((n + 3) / 4, 256)), dim3(256), 0, st, K, n, d);
    else
        hipLaunchKernelGGL(dropout_apply_kernel<false>, dim3(stream_grid_full(n, 256)), dim3(256), 0, st, K, n, d);
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

}  // namespace ndcn
