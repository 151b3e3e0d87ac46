// fixed_adams: the predictor / corrector passes of the reference's AdamsBashforthMoulton (torchdiffeq/_impl/fixed_adams.py:179-200) - the
// fixed-grid Adams-Bashforth step of adams.hip corrected by the Adams-Moulton formula over the same history, iterated until every element
// of the step has settled.
//
//   abm_predict_f32     dy = dt * sum a_i f_i, delta = dt * sum m_i f_i, u = y + dy: ONE streaming pass over the n = 3..11 history panels
//                       (the reference reads them twice: :182 and :188)
//   abm_correct_f32     dy' = c0 * f + delta, u = y + dy' and the number of elements that fail |dy - dy'| < atol + rtol * max(|dy|, |dy'|):
//                       an integer per workgroup, added to a device counter with one integer atomic per workgroup - whatever the order
//                       of the workgroups, the same number
//
// Rounding follows the reference term by term as in adams.hip (misc.py:22-25,33-37): every product and every sum rounded on its own, so
// FP contraction is switched OFF for this translation unit and the arithmetic is written with plain operators.
#include <stdint.h>

#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace ndcn {

namespace {

constexpr int kMinTerms = 3;           // fixed_adams.py:146,174: below three evaluations the step is RK4
constexpr int kMaxTerms = 11;          // :147,163

struct AbmArgs {
    const float *f[kMaxTerms];         // newest first
    float a[kMaxTerms];                // Adams-Bashforth weights of order n
    float m[kMaxTerms];                // Adams-Moulton weights of the history (the formula over n + 1 points without its leading one)
    const float *y;
    float *dy, *delta, *u;
    float dt;
};

__device__ __forceinline__ float dot1(const float *f, const float *w, int n, float dt) {
    float s = 0.f + w[0] * f[0];                            // Python's sum() starts from 0: a lone -0 product becomes +0
#pragma unroll
    for (int j = 1; j < n; ++j) s = s + w[j] * f[j];
    return dt * s;
}

// The lanes of ab_step_kernel (adams.hip): elements [head, head + 4 n4) by 16 bytes per lane, the <= 3 in front and the <= 3 behind by
// single lanes (n4 = 0: everything); a grid-stride loop on a grid sized from the compute units; the N + 1 loads of an item are issued
// before the first use.  The three outputs are written once and not read again by this launch.
template <int N>
__global__ __launch_bounds__(256) void abm_predict_kernel(AbmArgs p, int64_t head, int64_t n4, int64_t n) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < n4; i += stride) {
        const int64_t e = head + 4 * i;
        const float4 y = *reinterpret_cast<const float4 *>(p.y + e);          // first: the compiler keeps the loads in this order
        float4 v[N];
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = *reinterpret_cast<const float4 *>(p.f[j] + e);
        // ... but would sink the last of them below the first products (seen in the ISA at N = 6..10).  Loads do not cross the empty
        // statement with a memory clobber, and every value passes through one behind it (volatile statements keep their order): no use
        // comes before the N + 1 loads have been issued.  No instruction is emitted for either.
        asm volatile("" ::: "memory");
        float fx[N], fy[N], fz[N], fw[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            fx[j] = v[j].x; fy[j] = v[j].y; fz[j] = v[j].z; fw[j] = v[j].w;
            asm volatile("" : "+v"(fx[j]), "+v"(fy[j]), "+v"(fz[j]), "+v"(fw[j]));
        }
        float4 dy, dl, u;
        dy.x = dot1(fx, p.a, N, p.dt); dy.y = dot1(fy, p.a, N, p.dt); dy.z = dot1(fz, p.a, N, p.dt); dy.w = dot1(fw, p.a, N, p.dt);
        dl.x = dot1(fx, p.m, N, p.dt); dl.y = dot1(fy, p.m, N, p.dt); dl.z = dot1(fz, p.m, N, p.dt); dl.w = dot1(fw, p.m, N, p.dt);
        u.x = y.x + dy.x; u.y = y.y + dy.y; u.z = y.z + dy.z; u.w = y.w + dy.w;
        *reinterpret_cast<float4 *>(p.dy + e) = dy;
        *reinterpret_cast<float4 *>(p.delta + e) = dl;
        *reinterpret_cast<float4 *>(p.u + e) = u;
    }
    const int64_t rest = n - 4 * n4;
    for (int64_t r = tid; r < rest; r += stride) {
        const int64_t e = r < head ? r : r + 4 * n4;
        float f[N];
#pragma unroll
        for (int j = 0; j < N; ++j) f[j] = p.f[j][e];
        const float y = p.y[e];
        const float dy = dot1(f, p.a, N, p.dt);
        p.dy[e] = dy;
        p.delta[e] = dot1(f, p.m, N, p.dt);
        p.u[e] = y + dy;
    }
}

struct AbmcArgs {
    const float *f, *delta, *y;
    float *dy, *u;
    unsigned long long *count;
    float c0, rtol, atol;
};

// one element of the corrector pass: the new increment, and 1 where the pair (old, new) fails misc.py:33-37 - a strict `<`, so a NaN
// on either side (err is NaN then) and err == tol both fail
__device__ __forceinline__ float corr1(float f, float delta, float old, float c0, float rtol, float atol, unsigned &bad) {
    const float dy = c0 * f + delta;
    const float tol = atol + rtol * fmaxf(fabsf(old), fabsf(dy));
    const float err = fabsf(old - dy);
    bad += (err < tol) ? 0u : 1u;
    return dy;
}

__global__ __launch_bounds__(256) void abm_correct_kernel(AbmcArgs p, int64_t head, int64_t n4, int64_t n) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    unsigned bad = 0;
    for (int64_t i = tid; i < n4; i += stride) {
        const int64_t e = head + 4 * i;
        const float4 f = *reinterpret_cast<const float4 *>(p.f + e);
        const float4 dl = *reinterpret_cast<const float4 *>(p.delta + e);
        const float4 y = *reinterpret_cast<const float4 *>(p.y + e);
        const float4 old = *reinterpret_cast<const float4 *>(p.dy + e);
        float4 dy, u;
        dy.x = corr1(f.x, dl.x, old.x, p.c0, p.rtol, p.atol, bad);
        dy.y = corr1(f.y, dl.y, old.y, p.c0, p.rtol, p.atol, bad);
        dy.z = corr1(f.z, dl.z, old.z, p.c0, p.rtol, p.atol, bad);
        dy.w = corr1(f.w, dl.w, old.w, p.c0, p.rtol, p.atol, bad);
        u.x = y.x + dy.x; u.y = y.y + dy.y; u.z = y.z + dy.z; u.w = y.w + dy.w;
        *reinterpret_cast<float4 *>(p.dy + e) = dy;
        *reinterpret_cast<float4 *>(p.u + e) = u;
    }
    const int64_t rest = n - 4 * n4;
    for (int64_t r = tid; r < rest; r += stride) {
        const int64_t e = r < head ? r : r + 4 * n4;
        const float y = p.y[e];
        const float dy = corr1(p.f[e], p.delta[e], p.dy[e], p.c0, p.rtol, p.atol, bad);
        p.dy[e] = dy;
        p.u[e] = y + dy;
    }
    // the workgroup's count: integers, so the order of the additions does not matter
    __shared__ unsigned part[256 / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = part[0] + part[1] + part[2] + part[3];
        if (total) atomicAdd(p.count, (unsigned long long)total);
    }
}

template <int N>
void predict_launch(const AbmArgs &p, int64_t head, int64_t n4, int64_t n, hipStream_t st) {
    const int64_t rest = n - 4 * n4;
    hipLaunchKernelGGL(abm_predict_kernel<N>, dim3(ab_grid(n4 > rest ? n4 : rest)), dim3(256), 0, st, p, head, n4, n);
}

inline uintptr_t off16(const void *p) { return reinterpret_cast<uintptr_t>(p) & 15u; }

// the split of n elements into head / 16-byte body / tail when every panel sits `off` bytes behind a 16-byte boundary (same: they do)
inline void lanes(bool same, uintptr_t off, int64_t n, int64_t &head, int64_t &n4) {
    head = 0;
    n4 = 0;
    if (same) {
        head = (int64_t)((16u - off) & 15u) / 4;
        if (head > n) head = n;
        n4 = (n - head) / 4;
    }
    if (n4 == 0) head = 0;
}

}  // namespace

int abm_predict_f32(float *dy, float *delta, float *u, const float *y, const float *const *h_f, const float *h_a, const float *h_m,
                    int n_terms, float dt, int64_t n, hipStream_t st) {
    if (n_terms < kMinTerms || n_terms > kMaxTerms) { set_error("abm_predict: %d terms, the orders are %d..%d", n_terms, kMinTerms, kMaxTerms); return NDCN_EINVAL; }
    if (!dy || !delta || !u || !y || !h_f || !h_a || !h_m || n < 0) { set_error("abm_predict: null argument"); return NDCN_EINVAL; }
    if (dy == delta || dy == u || delta == u || dy == y || delta == y) { set_error("abm_predict: the outputs alias each other or the state (only u may be y)"); return NDCN_EINVAL; }
    AbmArgs p;
    p.y = y; p.dy = dy; p.delta = delta; p.u = u; p.dt = dt;
    const uintptr_t off = off16(u);
    bool same = (off & 3u) == 0 && off16(y) == off && off16(dy) == off && off16(delta) == off;
    for (int j = 0; j < kMaxTerms; ++j) {
        p.f[j] = h_f[j < n_terms ? j : 0];
        p.a[j] = j < n_terms ? h_a[j] : 0.f;
        p.m[j] = j < n_terms ? h_m[j] : 0.f;
        if (j >= n_terms) continue;
        if (!h_f[j]) { set_error("abm_predict: term %d is null", j); return NDCN_EINVAL; }
        if (h_f[j] == dy || h_f[j] == delta || h_f[j] == u) { set_error("abm_predict: an output aliases history panel %d", j); return NDCN_EINVAL; }
        same = same && off16(h_f[j]) == off;
    }
    if (n == 0) return NDCN_OK;
    int64_t head, n4;
    lanes(same, off, n, head, n4);
    ProfScope prof(PROF_COMBINE, st, 4.0 * n * (n_terms + 4), 1.0 * n * (4 * n_terms + 3));
    switch (n_terms) {
        case 3: predict_launch<3>(p, head, n4, n, st); break;
        case 4: predict_launch<4>(p, head, n4, n, st); break;
        case 5: predict_launch<5>(p, head, n4, n, st); break;
        case 6: predict_launch<6>(p, head, n4, n, st); break;
        case 7: predict_launch<7>(p, head, n4, n, st); break;
        case 8: predict_launch<8>(p, head, n4, n, st); break;
        case 9: predict_launch<9>(p, head, n4, n, st); break;
        case 10: predict_launch<10>(p, head, n4, n, st); break;
        default: predict_launch<11>(p, head, n4, n, st); break;
    }
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

int abm_correct_f32(float *dy, float *u, const float *f, const float *delta, const float *y, float c0, float rtol, float atol, int64_t n,
                    unsigned long long *d_count, hipStream_t st) {
    if (!dy || !u || !f || !delta || !y || !d_count || n < 0) { set_error("abm_correct: null argument"); return NDCN_EINVAL; }
    if ((reinterpret_cast<uintptr_t>(d_count) & 7u) != 0) { set_error("abm_correct: the counter must be 8-byte aligned"); return NDCN_EINVAL; }
    if (u == f || u == delta || u == y || u == dy || dy == f || dy == delta || dy == y) {
        set_error("abm_correct: u or dy aliases an input (dy is updated in place, nothing else may overlap)");
        return NDCN_EINVAL;
    }
    NDCN_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
    if (n == 0) return NDCN_OK;
    AbmcArgs p;
    p.f = f; p.delta = delta; p.y = y; p.dy = dy; p.u = u; p.count = d_count;
    p.c0 = c0; p.rtol = rtol; p.atol = atol;
    const uintptr_t off = off16(u);
    const bool same = (off & 3u) == 0 && off16(f) == off && off16(delta) == off && off16(y) == off && off16(dy) == off;
    int64_t head, n4;
    lanes(same, off, n, head, n4);
    const int64_t rest = n - 4 * n4;
    ProfScope prof(PROF_ERROR, st, 4.0 * n * 6, 1.0 * n * 9);
    hipLaunchKernelGGL(abm_correct_kernel, dim3(ab_grid(n4 > rest ? n4 : rest)), dim3(256), 0, st, p, head, n4, n);
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

}  // namespace ndcn

using namespace ndcn;

extern "C" {

int ndcn_abm_predict_f32(float *dy, float *delta, float *u, const float *y, const float *const *h_f, const float *h_a, const float *h_m,
                         int n, float dt, int64_t n_elem, void *stream) {
    return abm_predict_f32(dy, delta, u, y, h_f, h_a, h_m, n, dt, n_elem, static_cast<hipStream_t>(stream));
}

int ndcn_abm_correct_f32(float *dy, float *u, const float *f, const float *delta, const float *y, float c0, float rtol, float atol,
                         int64_t n_elem, uint64_t *d_count, void *stream) {
    return abm_correct_f32(dy, u, f, delta, y, c0, rtol, atol, n_elem, reinterpret_cast<unsigned long long *>(d_count),
                           static_cast<hipStream_t>(stream));
}

}  // extern "C"
