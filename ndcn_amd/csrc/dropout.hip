// K *= m in place: the dropout factor of csrc/dropout.h as a streaming pass behind the launches that have no dropout epilogue
// (every route of ndcn_rhs_f32 / ndcn_rhs_rk_f32 but the narrow-panel one).  The mask depends on the flat element index alone, so
// the pass is one-dimensional: any n, any H, panels over 2^31 elements.
//   VEC   the panel is 16-byte aligned: a lane owns elements 4 q .. 4 q + 3 - ONE Philox call, one 16-byte load, one 16-byte store;
//         the n & 3 elements behind the last whole group take the scalar expression
//   else  a misaligned view: an element per lane (its own Philox call, word i & 3)
//
// dropout_combine_kernel: that pass and the un-fused stage sum behind it (rk.hip combine_kernel) as ONE pass - the masked K' is
// stored and, still in registers, enters out = y0 + sum_j c_j k_j as its LAST term: (n_prev + 2) panel reads and two writes where
// the two kernels read (n_prev + 3) and launch twice.  Same products, same sums, same order (contraction is off): the same bits.
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

// the earlier stage derivatives of the sum and every coefficient: c[n] belongs to the masked K
struct DropTerms {
    const float *k[5];
    float c[6];
    int n;
};

__device__ __forceinline__ float drop_keep(uint32_t u, const DropArgs &d) { return u >= d.thresh ? d.s : 0.f; }

// sum_j c_j k_j[i] + c_n kd, left to right from +0, every product and sum rounded on its own (rk.hip wsum1 with kd as the last term)
__device__ __forceinline__ float drop_wsum1(const DropTerms &t, int64_t i, float kd) {
    if (t.n == 0) return 0.f + t.c[0] * kd;
    float acc = 0.f + t.c[0] * t.k[0][i];
#pragma unroll
    for (int j = 1; j < 5; ++j)
        if (j < t.n) acc = acc + t.c[j] * t.k[j][i];
    return acc + t.c[t.n] * kd;
}

// K[i] = K[i] * m(i), stored; out[i] = y0[i] + (((0 + c_0 k_0[i]) + ...) + c_n K'[i])  (y0 null: the sum alone).  out, y0 and the k_j
// must not overlap K; VEC: every pointer is 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void dropout_combine_kernel(float *K, int64_t n, DropArgs d, float *__restrict__ out,
                                                              const float *__restrict__ y0, DropTerms t) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t tail = t0;
    if (VEC) {
        const int64_t n4 = n >> 2;
        dr_f32x4 *K4 = reinterpret_cast<dr_f32x4 *>(K);
        for (int64_t q = t0; q < n4; q += stride) {
            const Philox4 o = drop_words(d, q);
            dr_f32x4 v = K4[q];
            v.x = v.x * drop_keep(o.w[0], d);
            v.y = v.y * drop_keep(o.w[1], d);
            v.z = v.z * drop_keep(o.w[2], d);
            v.w = v.w * drop_keep(o.w[3], d);
            K4[q] = v;
            dr_f32x4 acc;
            if (t.n == 0) {
                acc = 0.f + t.c[0] * v;
            } else {
                acc = 0.f + t.c[0] * reinterpret_cast<const dr_f32x4 *>(t.k[0])[q];
#pragma unroll
                for (int j = 1; j < 5; ++j)
                    if (j < t.n) acc = acc + t.c[j] * reinterpret_cast<const dr_f32x4 *>(t.k[j])[q];
                acc = acc + t.c[t.n] * v;
            }
            if (y0) acc = reinterpret_cast<const dr_f32x4 *>(y0)[q] + acc;
            reinterpret_cast<dr_f32x4 *>(out)[q] = acc;
        }
        tail = 4 * n4 + t0;
    }
    for (int64_t i = tail; i < n; i += stride) {
        const float kd = K[i] * drop_factor(d, i);
        K[i] = kd;
        const float s = drop_wsum1(t, i, kd);
        out[i] = y0 ? y0[i] + s : s;
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

int dropout_combine_f32(float *K, int64_t n, const DropArgs &d, float *out, const float *y0, const float *const *h_kprev, const float *h_c,
                        int n_prev, hipStream_t st) {
    if (n_prev < 0 || n_prev > 5 || !h_c || (n_prev > 0 && !h_kprev)) { set_error("dropout_combine: n_prev must be 0..5, with its panels and coefficients"); return NDCN_EINVAL; }
    if (n == 0) return NDCN_OK;
    DropTerms t;
    t.n = n_prev;
    bool vec = aligned16(K) && aligned16(out) && (!y0 || aligned16(y0));
    for (int j = 0; j < 5; ++j) {
        t.k[j] = j < n_prev ? h_kprev[j] : K;
        if (j < n_prev) {
            if (!h_kprev[j]) { set_error("dropout_combine: null stage panel"); return NDCN_EINVAL; }
            vec = vec && aligned16(h_kprev[j]);
        }
    }
    for (int j = 0; j < 6; ++j) t.c[j] = j <= n_prev ? h_c[j] : 0.f;
    ProfScope prof(PROF_STAGE, st, 4.0 * (double)n * (n_prev + 3 + (y0 ? 1 : 0)), (2.0 * n_prev + 4.0) * (double)n);
    if (vec)
        hipLaunchKernelGGL(dropout_combine_kernel<true>, dim3(stream_grid_full((n + 3) / 4, 256)), dim3(256), 0, st, K, n, d, out, y0, t);
    else
        hipLaunchKernelGGL(dropout_combine_kernel<false>, dim3(stream_grid_full(n, 256)), dim3(256), 0, st, K, n, d, out, y0, t);
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

}  // namespace ndcn
