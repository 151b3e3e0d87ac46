// The pointwise half of one step of the variable-coefficient Adams-Bashforth-Moulton method (adams.py:62-170) as three streaming
// passes: predictor, corrector + error sums, and the phi update of an accepted step.  Composed from the per-operation kernels of
// rk.hip the same step is k - 1 ndcn_scale_f32, 2 k + 3 ndcn_rk_combine_f32 and up to four ndcn_rk_error_f32 calls at order k, every
// link of a phi chain written by one launch and read back by the next.  Here a chain lives in registers.
//
// The bits are the composed ones.  FP contraction is OFF for this translation unit as in rk.hip; every product and every sum below
// is the single instruction the composed kernels execute for it, in their order:
//   e_j  = beta_j * phi_j  (j >= 1; e_0 = phi_0)                  scale_kernel:    w * x            - re-formed here, never stored
//   s    = ((0 + c_0 e_0) + c_1 e_1) + ...  ;  y + s              combine_kernel:  wsum4 / wsum1, then y0 + s
//   a - b = a + (0 + (-1) * b)                                    combine_kernel with the single coefficient -1 that core.Adams.step
//                                                                 passes: -0 - (+0) is therefore +0, as composed
//   coef * ip = 0 + coef * ip  ->  err_ratio_sq                   rk_error_kernel with one term
// The -1 arrives as a kernel argument like every other coefficient, so the product is a real multiplication, as in combine_kernel -
// a literal would let the compiler negate instead, which moves the sign of a NaN.
//
// The order is a template parameter: all panel loads of an element group are issued before the first dependent operation (at order 12
// the corrector has 15 float4 loads per lane in flight), and nothing is indexed at run time.
#include "common.h"

#pragma clang fp contract(off)

#include "rk_shared.h"

namespace ndcn {

constexpr int kAdamsMaxOrder = 12;

template <bool VEC> struct Lane;
template <> struct Lane<true> {
    typedef float4 T;
    static __device__ __forceinline__ float4 ld(const float *p, int64_t i) { return ld4(p, i); }
    static __device__ __forceinline__ void st(float *p, int64_t i, float4 v) { st4(p, i, v); }
};
template <> struct Lane<false> {
    typedef float T;
    static __device__ __forceinline__ float ld(const float *p, int64_t i) { return p[i]; }
    static __device__ __forceinline__ void st(float *p, int64_t i, float v) { p[i] = v; }
};

__device__ __forceinline__ float mul1(float c, float v) { return c * v; }
__device__ __forceinline__ float4 mul1(float c, float4 v) { return make_float4(c * v.x, c * v.y, c * v.z, c * v.w); }
__device__ __forceinline__ float add1(float a, float b) { return a + b; }
__device__ __forceinline__ float4 add1(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
// 0 + c v: the first (or only) term of Python's sum(), which starts from +0
__device__ __forceinline__ float term0(float c, float v) { return 0.f + c * v; }
__device__ __forceinline__ float4 term0(float c, float4 v) { return make_float4(0.f + c * v.x, 0.f + c * v.y, 0.f + c * v.z, 0.f + c * v.w); }
// a - b as ops.combine(a, [b], [-1]) forms it
template <class T> __device__ __forceinline__ T minus(T a, T b, float neg1) { return add1(a, term0(neg1, b)); }

// phi_0 .. phi_{order-1} and the float32 beta_j that turn them into explicit phi (beta[0] is not read)
struct AdamsPhi {
    const float *phi[kAdamsMaxOrder];
    float beta[kAdamsMaxOrder];
};

// -------------------------------------------------------------------------------- predictor
// p_next = y + ((0 + c_0 e_0) + c_1 e_1 + ... + c_{M-1} e_{M-1})     adams.py:44-50
struct PredictArgs {
    AdamsPhi p;
    float c[kAdamsMaxOrder];
    const float *y;
    float *out;
};

template <int M, bool VEC>
__global__ __launch_bounds__(256) void adams_predict_kernel(PredictArgs a, int64_t n_items) {
    typedef typename Lane<VEC>::T T;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * blockDim.x) {
        T v[M];
#pragma unroll
        for (int j = 0; j < M; ++j) v[j] = Lane<VEC>::ld(a.p.phi[j], i);
        const T y = Lane<VEC>::ld(a.y, i);
        T acc = term0(a.c[0], v[0]);
#pragma unroll
        for (int j = 1; j < M; ++j) acc = add1(acc, mul1(a.c[j], mul1(a.p.beta[j], v[j])));
        Lane<VEC>::st(a.out, i, add1(y, acc));
    }
}

// -------------------------------------------------------------------------------- corrector + error sums
// ip_0 = nf, ip_j = ip_{j-1} - e_{j-1} (adams.py:53-59); y_next = p_next + c_corr ip_{order-1} (:129-132); up to four sums of squared
// error ratios against {y0, y_next} (:135-139, :154-165), each the sum ndcn_rk_error_f32 forms for that one term above the ATen-order
// bound: rk_error_kernel's element-to-thread map, grid and per-thread order, block_sum2, reduce_finish.
struct CorrectArgs {
    AdamsPhi p;
    const float *nf, *p_next, *y0;
    float *y_next;
    float c_corr, neg1;
    float coef[4];          // sum 0, 3: times ip_order; sum 1: times ip_{order-1}; sum 2: times ip_{order-2}
    unsigned mask;          // bit q: sum q is formed
    float rtol, atol;
};

__device__ __forceinline__ void ratio_acc(double &s, float coef, float ip, float y0, float y1, float rtol, float atol) {
    s += (double)err_ratio_sq(0.f + coef * ip, y0, y1, rtol, atol);
}
__device__ __forceinline__ void ratio_acc(double &s, float coef, float4 ip, float4 y0, float4 y1, float rtol, float atol) {
    ratio_acc(s, coef, ip.x, y0.x, y1.x, rtol, atol);
    ratio_acc(s, coef, ip.y, y0.y, y1.y, rtol, atol);
    ratio_acc(s, coef, ip.z, y0.z, y1.z, rtol, atol);
    ratio_acc(s, coef, ip.w, y0.w, y1.w, rtol, atol);
}

template <int ORDER, bool VEC>
__global__ __launch_bounds__(256) void adams_correct_kernel(CorrectArgs a, int64_t n_items, double *__restrict__ partial) {
    typedef typename Lane<VEC>::T T;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * blockDim.x) {
        T v[ORDER];
#pragma unroll
        for (int j = 0; j < ORDER; ++j) v[j] = Lane<VEC>::ld(a.p.phi[j], i);
        const T nf = Lane<VEC>::ld(a.nf, i), pn = Lane<VEC>::ld(a.p_next, i), y0 = Lane<VEC>::ld(a.y0, i);
        // the chain; only its last three links stay live: lo2 = ip_{ORDER-2}, lo1 = ip_{ORDER-1}, top = ip_ORDER
        T lo2 = nf, lo1 = nf, top = nf;
#pragma unroll
        for (int j = 1; j <= ORDER; ++j) {
            lo2 = lo1;
            lo1 = top;
            top = minus(top, j == 1 ? v[0] : mul1(a.p.beta[j - 1], v[j - 1]), a.neg1);
        }
        const T y1 = add1(pn, term0(a.c_corr, lo1));
        Lane<VEC>::st(a.y_next, i, y1);
        if (a.mask & 1u) ratio_acc(s0, a.coef[0], top, y0, y1, a.rtol, a.atol);
        if (a.mask & 2u) ratio_acc(s1, a.coef[1], lo1, y0, y1, a.rtol, a.atol);
        if (ORDER >= 2 && (a.mask & 4u)) ratio_acc(s2, a.coef[2], lo2, y0, y1, a.rtol, a.atol);
        if (a.mask & 8u) ratio_acc(s3, a.coef[3], top, y0, y1, a.rtol, a.atol);
    }
    block_sum2(s0, s1);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = s0; partial[2 * blockIdx.x + 1] = s1; }
    __syncthreads();
    block_sum2(s2, s3);
    double *partial2 = partial + 2 * kRedBlocks;
    if (threadIdx.x == 0) { partial2[2 * blockIdx.x] = s2; partial2[2 * blockIdx.x + 1] = s3; }
}

// the finish of both pairs in one launch: out4 = {sum 0, sum 1, sum 2, sum 3}
__global__ __launch_bounds__(256) void adams_finish_kernel(const double *__restrict__ partial, int n_partial, double *__restrict__ out4) {
    reduce_finish(partial, n_partial, out4, 0);
    __syncthreads();
    reduce_finish(partial + 2 * kRedBlocks, n_partial, out4 + 2, 0);
}

// -------------------------------------------------------------------------------- phi update of an accepted step
// new_phi_0 = nf2 (the caller's panel, not copied); new_phi_j = new_phi_{j-1} - e_{j-1}, j = 1 .. NOUT - 1     adams.py:53-59 at :142
struct UpdateArgs {
    AdamsPhi p;
    const float *nf2;
    float *out[kAdamsMaxOrder];     // out[j]: new_phi_j, j >= 1 (out[0] is not written)
    float neg1;
};

template <int NOUT, bool VEC>
__global__ __launch_bounds__(256) void adams_update_kernel(UpdateArgs a, int64_t n_items) {
    typedef typename Lane<VEC>::T T;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * blockDim.x) {
        T v[NOUT - 1];
#pragma unroll
        for (int j = 0; j < NOUT - 1; ++j) v[j] = Lane<VEC>::ld(a.p.phi[j], i);
        T cur = Lane<VEC>::ld(a.nf2, i);
#pragma unroll
        for (int j = 1; j < NOUT; ++j) {
            cur = minus(cur, j == 1 ? v[0] : mul1(a.p.beta[j - 1], v[j - 1]), a.neg1);
            Lane<VEC>::st(a.out[j], i, cur);
        }
    }
}

// -------------------------------------------------------------------------------- host wrappers
static bool overlap(const float *a, const float *b, int64_t n) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b), len = (uintptr_t)n * sizeof(float);
    return x < y + len && y < x + len;
}

// fills p from the first n_phi entries of the host tables; vec: cleared when a panel is not 16-byte aligned
static bool fill_phi(AdamsPhi &p, const float *const *h_phi, const float *h_beta, int n_phi, bool &vec) {
    for (int j = 0; j < kAdamsMaxOrder; ++j) {
        const int u = j < n_phi ? j : 0;
        if (!h_phi[u]) return false;
        p.phi[j] = h_phi[u];
        p.beta[j] = (j >= 1 && j < n_phi) ? h_beta[j] : 0.f;
        vec = vec && aligned16(h_phi[u]);
    }
    return true;
}

#define NDCN_ADAMS_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)

int adams_predict_f32(float *p_next, const float *y, const float *const *h_phi, const float *h_beta, const float *h_c, int order,
                      int64_t n, hipStream_t st) {
    if (order < 1 || order > kAdamsMaxOrder) { set_error("adams_predict: order %d outside 1..%d", order, kAdamsMaxOrder); return NDCN_EINVAL; }
    if (n < 1) { set_error("adams_predict: needs at least one element"); return NDCN_EINVAL; }
    if (!p_next || !y || !h_phi || !h_beta || !h_c) { set_error("adams_predict: null panel"); return NDCN_EINVAL; }
    const int m = order > 1 ? order - 1 : 1;
    PredictArgs a;
    bool vec = (n % 4 == 0) && aligned16(p_next) && aligned16(y);
    if (!fill_phi(a.p, h_phi, h_beta, m, vec)) { set_error("adams_predict: null panel"); return NDCN_EINVAL; }
    bool alias = overlap(p_next, y, n);
    for (int j = 0; j < m; ++j) alias = alias || overlap(p_next, h_phi[j], n);
    if (alias) { set_error("adams_predict: the output aliases an input"); return NDCN_EINVAL; }
    for (int j = 0; j < kAdamsMaxOrder; ++j) a.c[j] = j < m ? h_c[j] : 0.f;
    a.y = y;
    a.out = p_next;
    ProfScope prof(PROF_COMBINE, st, 4.0 * n * (m + 2), 1.0 * n * (3 * m));
    const int64_t items = vec ? n / 4 : n;
    const int g = stream_grid_full(items, 256);
    switch (m) {
#define X(M_)                                                                                                              \
    case M_:                                                                                                               \
        if (vec) hipLaunchKernelGGL((adams_predict_kernel<M_, true>), dim3(g), dim3(256), 0, st, a, items);                \
        else hipLaunchKernelGGL((adams_predict_kernel<M_, false>), dim3(g), dim3(256), 0, st, a, items);                   \
        break;
        NDCN_ADAMS_CASES(X)
#undef X
    }
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

int64_t adams_correct_ws_bytes() { return (int64_t)2 * kRedBlocks * 2 * sizeof(double); }     // two arrays of pairs

int adams_correct_f32(float *y_next, const float *nf, const float *const *h_phi, const float *h_beta, int order, const float *p_next,
                      const float *y0, float c_corr, const float *h_coef4, unsigned mask, float rtol, float atol, int64_t n,
                      double *d_out4, void *d_ws, int64_t ws_bytes, hipStream_t st) {
    if (order < 1 || order > kAdamsMaxOrder) { set_error("adams_correct: order %d outside 1..%d", order, kAdamsMaxOrder); return NDCN_EINVAL; }
    if (n < 1) { set_error("adams_correct: needs at least one element"); return NDCN_EINVAL; }
    if (!y_next || !nf || !h_phi || !h_beta || !p_next || !y0 || !h_coef4 || !d_out4 || !d_ws) { set_error("adams_correct: null panel"); return NDCN_EINVAL; }
    if (mask > 15u || ((mask & 4u) && order < 2)) { set_error("adams_correct: sum mask %u names a link order %d does not have", mask, order); return NDCN_EINVAL; }
    if (ws_bytes < adams_correct_ws_bytes()) {
        set_error("adams_correct: scratch of %lld bytes, ndcn_adams_correct_ws_bytes() = %lld", (long long)ws_bytes, (long long)adams_correct_ws_bytes());
        return NDCN_EINVAL;
    }
    CorrectArgs a;
    bool vec = (n % 4 == 0) && aligned16(y_next) && aligned16(nf) && aligned16(p_next) && aligned16(y0);
    if (!fill_phi(a.p, h_phi, h_beta, order, vec)) { set_error("adams_correct: null panel"); return NDCN_EINVAL; }
    bool alias = overlap(y_next, nf, n) || overlap(y_next, p_next, n) || overlap(y_next, y0, n);
    for (int j = 0; j < order; ++j) alias = alias || overlap(y_next, h_phi[j], n);
    if (alias) { set_error("adams_correct: the output aliases an input"); return NDCN_EINVAL; }
    a.nf = nf; a.p_next = p_next; a.y0 = y0; a.y_next = y_next;
    a.c_corr = c_corr; a.neg1 = -1.f;
    for (int q = 0; q < 4; ++q) a.coef[q] = h_coef4[q];
    a.mask = mask; a.rtol = rtol; a.atol = atol;
    int n_sums = 0;
    for (int q = 0; q < 4; ++q) n_sums += (mask >> q) & 1u;
    ProfScope prof(PROF_ERROR, st, 4.0 * n * (order + 4), 1.0 * n * (4 * order + 2 + 8 * n_sums));
    const int64_t items = vec ? n / 4 : n;
    const int g = red_grid(items);
    double *partial = static_cast<double *>(d_ws);
    switch (order) {
#define X(K_)                                                                                                              \
    case K_:                                                                                                               \
        if (vec) hipLaunchKernelGGL((adams_correct_kernel<K_, true>), dim3(g), dim3(256), 0, st, a, items, partial);       \
        else hipLaunchKernelGGL((adams_correct_kernel<K_, false>), dim3(g), dim3(256), 0, st, a, items, partial);          \
        break;
        NDCN_ADAMS_CASES(X)
#undef X
    }
    hipLaunchKernelGGL(adams_finish_kernel, dim3(1), dim3(256), 0, st, partial, g, d_out4);
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

int adams_update_f32(float *const *h_out, const float *nf2, const float *const *h_phi, const float *h_beta, int order, int n_out,
                     int64_t n, hipStream_t st) {
    if (order < 1 || order > kAdamsMaxOrder) { set_error("adams_update: order %d outside 1..%d", order, kAdamsMaxOrder); return NDCN_EINVAL; }
    if (n_out < 1 || n_out > order + 1 || n_out > kAdamsMaxOrder) { set_error("adams_update: %d new phi at order %d (1..min(order + 1, %d))", n_out, order, kAdamsMaxOrder); return NDCN_EINVAL; }
    if (n < 1) { set_error("adams_update: needs at least one element"); return NDCN_EINVAL; }
    if (!nf2 || !h_phi || !h_beta || (n_out > 1 && !h_out)) { set_error("adams_update: null panel"); return NDCN_EINVAL; }
    if (n_out == 1) return NDCN_OK;                             // new_phi_0 is nf2 itself: nothing to write
    UpdateArgs a;
    bool vec = (n % 4 == 0) && aligned16(nf2);
    if (!fill_phi(a.p, h_phi, h_beta, n_out - 1, vec)) { set_error("adams_update: null panel"); return NDCN_EINVAL; }
    for (int j = 1; j < n_out; ++j)
        if (!h_out[j]) { set_error("adams_update: null panel"); return NDCN_EINVAL; }
    bool alias = false;
    for (int j = 1; j < n_out; ++j) {
        alias = alias || overlap(h_out[j], nf2, n);
        for (int q = 0; q < n_out - 1; ++q) alias = alias || overlap(h_out[j], h_phi[q], n);
        for (int q = 1; q < j; ++q) alias = alias || overlap(h_out[j], h_out[q], n);
    }
    if (alias) { set_error("adams_update: an output aliases an input or another output"); return NDCN_EINVAL; }
    for (int j = 0; j < kAdamsMaxOrder; ++j) {
        a.out[j] = h_out[(j >= 1 && j < n_out) ? j : 1];
        vec = vec && aligned16(a.out[j]);
    }
    a.nf2 = nf2;
    a.neg1 = -1.f;
    ProfScope prof(PROF_COMBINE, st, 4.0 * n * (2 * n_out - 1), 1.0 * n * (4 * (n_out - 1)));
    const int64_t items = vec ? n / 4 : n;
    const int g = stream_grid_full(items, 256);
    switch (n_out) {
#define X(N_)                                                                                                              \
    case N_ + 1:                                                                                                           \
        if (vec) hipLaunchKernelGGL((adams_update_kernel<N_ + 1, true>), dim3(g), dim3(256), 0, st, a, items);             \
        else hipLaunchKernelGGL((adams_update_kernel<N_ + 1, false>), dim3(g), dim3(256), 0, st, a, items);                \
        break;
        X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11)
#undef X
    }
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

#undef NDCN_ADAMS_CASES

}  // namespace ndcn
