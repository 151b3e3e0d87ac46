// explicit_adams under a gradient: the part of the reverse sweep that is specific to a linear multistep method.  The evaluation f_i
// of grid step i is a term of up to eleven later Adams-Bashforth steps, so its gradient GATHERS from the adjoints of their states:
//
//   ab_adjoint_f32     out = [base +] (((0 + c_0 g_0) + c_1 g_1) + ... + c_{n-1} g_{n-1}), n = 1..11: one streaming pass that reads the
//                      n adjoint panels (and the base) and writes one - the scatter form would be 2n read-modify-write passes
//
//   abm_adjoint_f32    the same gather for fixed_adams, whose evaluation is a term of the predictor (adjoint P) AND of the explicit part
//                      of the corrector (adjoint D) of every later step that holds it: out = [base +] ((((0 + cp_0 P_0) + cd_0 D_0) +
//                      cp_1 P_1) + cd_1 D_1 ...), n = 1..11 pairs - up to 22 panels and the base read in one pass
//
// c_q = fl32(dt * a_q) is formed on the host (core.ab_adjoint_terms; the pairs: core.abm_adjoint_terms).  Every product and sum is rounded on its own and the base is
// added last: FP contraction is switched OFF for this translation unit and the arithmetic is written with plain operators, as in
// adams.hip (whose ab_step_kernel this kernel has the shape of; it is no special case of it: ab_step needs a state, starts at three
// terms and multiplies the sum by dt).
#include <stdint.h>

#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace ndcn {

namespace {

constexpr int kAdjMaxTerms = 11;       // an evaluation is held for max_order - 1 <= 11 steps

struct AbAdjArgs {
    const float *g[kAdjMaxTerms];
    float c[kAdjMaxTerms];
    const float *base;                 // read only where BASE
    float *out;
};

template <int N, bool BASE>
__device__ __forceinline__ float adj1(const float *g, const float *c, float base) {
    float s = 0.f + c[0] * g[0];                            // the sum starts from an exact zero: a lone -0 product becomes +0
#pragma unroll
    for (int j = 1; j < N; ++j) s = s + c[j] * g[j];
    return BASE ? base + s : s;
}

// Elements [head, head + 4 n4) by 16 bytes per lane - every panel is 16-byte aligned at element `head` -, the <= 3 elements in front and
// the <= 3 behind by single lanes (n4 = 0: everything, panels that do not share an offset).  A grid-stride loop on a grid sized from
// the compute units.  The N (+ 1) loads of an item are issued before the first use; default cache policy - the gather of the step
// before reads N - 1 of the panels again.
template <int N, bool BASE>
__global__ __launch_bounds__(256) void ab_adjoint_kernel(AbAdjArgs p, int64_t head, int64_t n4, int64_t n) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < n4; i += stride) {
        const int64_t e = head + 4 * i;
        float4 v[N];
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = *reinterpret_cast<const float4 *>(p.g[j] + e);
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (BASE) b = *reinterpret_cast<const float4 *>(p.base + e);
        float gx[N], gy[N], gz[N], gw[N];
#pragma unroll
        for (int j = 0; j < N; ++j) { gx[j] = v[j].x; gy[j] = v[j].y; gz[j] = v[j].z; gw[j] = v[j].w; }
        float4 o;
        o.x = adj1<N, BASE>(gx, p.c, b.x);
        o.y = adj1<N, BASE>(gy, p.c, b.y);
        o.z = adj1<N, BASE>(gz, p.c, b.z);
        o.w = adj1<N, BASE>(gw, p.c, b.w);
        *reinterpret_cast<float4 *>(p.out + e) = o;
    }
    const int64_t rest = n - 4 * n4;
    for (int64_t r = tid; r < rest; r += stride) {
        const int64_t e = r < head ? r : r + 4 * n4;
        float g[N];
#pragma unroll
        for (int j = 0; j < N; ++j) g[j] = p.g[j][e];
        const float b = BASE ? p.base[e] : 0.f;
        p.out[e] = adj1<N, BASE>(g, p.c, b);
    }
}

template <int N>
void adj_launch(const AbAdjArgs &p, int64_t head, int64_t n4, int64_t n, hipStream_t st) {
    const int64_t rest = n - 4 * n4;
    const dim3 grid(ab_grid(n4 > rest ? n4 : rest));
    if (p.base)
        hipLaunchKernelGGL((ab_adjoint_kernel<N, true>), grid, dim3(256), 0, st, p, head, n4, n);
    else
        hipLaunchKernelGGL((ab_adjoint_kernel<N, false>), grid, dim3(256), 0, st, p, head, n4, n);
}

// ---- fixed_adams: pairs of adjoints.  The chain over the 2 N interleaved panels P_0, D_0, P_1, D_1, .. is the chain of ab_adjoint_kernel
// over 2 N terms; what differs is the number of loads in flight.  ALL 2 N (+ 1) 16-byte loads of an item are issued before the first use
// (N = 11: 92 data registers, under the 128 that keep four waves per SIMD - a two-half form would fit 64 registers and eight waves but
// wait twice per item; a streaming pass with 22 loads per lane in flight has no use for more waves).  The compiler would sink the
// later loads below the first products: loads do not cross the empty statement with a memory clobber, and every value passes through
// one behind it, as in abm_predict_kernel (adams_pc.hip).  No instruction is emitted for either.
constexpr int kPairMaxTerms = 2 * kAdjMaxTerms;

struct AbmAdjArgs {
    const float *g[kPairMaxTerms];     // P_0, D_0, P_1, D_1, ..
    float c[kPairMaxTerms];            // cp_0, cd_0, cp_1, cd_1, ..
    const float *base;                 // read only where BASE
    float *out;
};

template <int N, bool BASE>
__global__ __launch_bounds__(256) void abm_adjoint_kernel(AbmAdjArgs p, int64_t head, int64_t n4, int64_t n) {
    constexpr int M = 2 * N;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < n4; i += stride) {
        const int64_t e = head + 4 * i;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (BASE) b = *reinterpret_cast<const float4 *>(p.base + e);
        float4 v[M];
#pragma unroll
        for (int j = 0; j < M; ++j) v[j] = *reinterpret_cast<const float4 *>(p.g[j] + e);
        asm volatile("" ::: "memory");
        float gx[M], gy[M], gz[M], gw[M];
#pragma unroll
        for (int j = 0; j < M; ++j) {
            gx[j] = v[j].x; gy[j] = v[j].y; gz[j] = v[j].z; gw[j] = v[j].w;
            asm volatile("" : "+v"(gx[j]), "+v"(gy[j]), "+v"(gz[j]), "+v"(gw[j]));
        }
        float4 o;
        o.x = adj1<M, BASE>(gx, p.c, b.x);
        o.y = adj1<M, BASE>(gy, p.c, b.y);
        o.z = adj1<M, BASE>(gz, p.c, b.z);
        o.w = adj1<M, BASE>(gw, p.c, b.w);
        *reinterpret_cast<float4 *>(p.out + e) = o;
    }
    const int64_t rest = n - 4 * n4;
    for (int64_t r = tid; r < rest; r += stride) {
        const int64_t e = r < head ? r : r + 4 * n4;
        float g[M];
#pragma unroll
        for (int j = 0; j < M; ++j) g[j] = p.g[j][e];
        const float b = BASE ? p.base[e] : 0.f;
        p.out[e] = adj1<M, BASE>(g, p.c, b);
    }
}

template <int N>
void pair_launch(const AbmAdjArgs &p, int64_t head, int64_t n4, int64_t n, hipStream_t st) {
    const int64_t rest = n - 4 * n4;
    const dim3 grid(ab_grid(n4 > rest ? n4 : rest));
    if (p.base)
        hipLaunchKernelGGL((abm_adjoint_kernel<N, true>), grid, dim3(256), 0, st, p, head, n4, n);
    else
        hipLaunchKernelGGL((abm_adjoint_kernel<N, false>), grid, dim3(256), 0, st, p, head, n4, n);
}

}  // namespace

int ab_adjoint_f32(float *out, const float *base, const float *const *h_g, const float *h_c, int n_terms, int64_t n, hipStream_t st) {
    if (n_terms < 1 || n_terms > kAdjMaxTerms) { set_error("ab_adjoint: %d terms, 1..%d are taken", n_terms, kAdjMaxTerms); return NDCN_EINVAL; }
    if (!out || !h_g || !h_c || n < 0) { set_error("ab_adjoint: null argument"); return NDCN_EINVAL; }
    AbAdjArgs p;
    p.base = base; p.out = out;
    const uintptr_t off = reinterpret_cast<uintptr_t>(out) & 15u;
    bool same_offset = (off & 3u) == 0 && (!base || (reinterpret_cast<uintptr_t>(base) & 15u) == off);
    for (int j = 0; j < kAdjMaxTerms; ++j) {
        p.g[j] = h_g[j < n_terms ? j : 0];
        p.c[j] = j < n_terms ? h_c[j] : 0.f;
        if (j >= n_terms) continue;
        if (!h_g[j]) { set_error("ab_adjoint: term %d is null", j); return NDCN_EINVAL; }
        if (h_g[j] == out) { set_error("ab_adjoint: out aliases term %d (only the base may be updated in place)", j); return NDCN_EINVAL; }
        same_offset = same_offset && (reinterpret_cast<uintptr_t>(h_g[j]) & 15u) == off;
    }
    if (n == 0) return NDCN_OK;
    int64_t head = 0, n4 = 0;
    if (same_offset) {
        head = (int64_t)((16u - off) & 15u) / 4;
        if (head > n) head = n;
        n4 = (n - head) / 4;
    }
    if (n4 == 0) head = 0;
    const int reads = n_terms + (base ? 1 : 0);
    ProfScope prof(PROF_COMBINE, st, 4.0 * n * (reads + 1), 2.0 * n * reads);
    switch (n_terms) {
        case 1: adj_launch<1>(p, head, n4, n, st); break;
        case 2: adj_launch<2>(p, head, n4, n, st); break;
        case 3: adj_launch<3>(p, head, n4, n, st); break;
        case 4: adj_launch<4>(p, head, n4, n, st); break;
        case 5: adj_launch<5>(p, head, n4, n, st); break;
        case 6: adj_launch<6>(p, head, n4, n, st); break;
        case 7: adj_launch<7>(p, head, n4, n, st); break;
        case 8: adj_launch<8>(p, head, n4, n, st); break;
        case 9: adj_launch<9>(p, head, n4, n, st); break;
        case 10: adj_launch<10>(p, head, n4, n, st); break;
        default: adj_launch<11>(p, head, n4, n, st); break;
    }
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

int abm_adjoint_f32(float *out, const float *base, const float *const *h_p, const float *h_cp, const float *const *h_d, const float *h_cd,
                    int n_pairs, int64_t n, hipStream_t st) {
    if (n_pairs < 1 || n_pairs > kAdjMaxTerms) { set_error("abm_adjoint: %d pairs, 1..%d are taken", n_pairs, kAdjMaxTerms); return NDCN_EINVAL; }
    if (!out || !h_p || !h_cp || !h_d || !h_cd || n < 0) { set_error("abm_adjoint: null argument"); return NDCN_EINVAL; }
    AbmAdjArgs p;
    p.base = base; p.out = out;
    const uintptr_t off = reinterpret_cast<uintptr_t>(out) & 15u;
    bool same_offset = (off & 3u) == 0 && (!base || (reinterpret_cast<uintptr_t>(base) & 15u) == off);
    for (int j = 0; j < kAdjMaxTerms; ++j) {
        const int q = j < n_pairs ? j : 0;
        p.g[2 * j] = h_p[q]; p.g[2 * j + 1] = h_d[q];
        p.c[2 * j] = j < n_pairs ? h_cp[j] : 0.f;
        p.c[2 * j + 1] = j < n_pairs ? h_cd[j] : 0.f;
        if (j >= n_pairs) continue;
        if (!h_p[j] || !h_d[j]) { set_error("abm_adjoint: pair %d has a null panel", j); return NDCN_EINVAL; }
        if (h_p[j] == out || h_d[j] == out) { set_error("abm_adjoint: out aliases a panel of pair %d (only the base may be updated in place)", j); return NDCN_EINVAL; }
        same_offset = same_offset && (reinterpret_cast<uintptr_t>(h_p[j]) & 15u) == off && (reinterpret_cast<uintptr_t>(h_d[j]) & 15u) == off;
    }
    if (n == 0) return NDCN_OK;
    int64_t head = 0, n4 = 0;
    if (same_offset) {
        head = (int64_t)((16u - off) & 15u) / 4;
        if (head > n) head = n;
        n4 = (n - head) / 4;
    }
    if (n4 == 0) head = 0;
    const int reads = 2 * n_pairs + (base ? 1 : 0);
    ProfScope prof(PROF_COMBINE, st, 4.0 * n * (reads + 1), 2.0 * n * reads);
    switch (n_pairs) {
        case 1: pair_launch<1>(p, head, n4, n, st); break;
        case 2: pair_launch<2>(p, head, n4, n, st); break;
        case 3: pair_launch<3>(p, head, n4, n, st); break;
        case 4: pair_launch<4>(p, head, n4, n, st); break;
        case 5: pair_launch<5>(p, head, n4, n, st); break;
        case 6: pair_launch<6>(p, head, n4, n, st); break;
        case 7: pair_launch<7>(p, head, n4, n, st); break;
        case 8: pair_launch<8>(p, head, n4, n, st); break;
        case 9: pair_launch<9>(p, head, n4, n, st); break;
        case 10: pair_launch<10>(p, head, n4, n, st); break;
        default: pair_launch<11>(p, head, n4, n, st); break;
    }
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

}  // namespace ndcn

using namespace ndcn;

extern "C" {

int ndcn_ab_adjoint_f32(float *out, const float *base, const float *const *h_g, const float *h_c, int n, int64_t n_elem, void *stream) {
    return ab_adjoint_f32(out, base, h_g, h_c, n, n_elem, static_cast<hipStream_t>(stream));
}

int ndcn_abm_adjoint_f32(float *out, const float *base, const float *const *h_p, const float *h_cp, const float *const *h_d,
                         const float *h_cd, int n, int64_t n_elem, void *stream) {
    return abm_adjoint_f32(out, base, h_p, h_cp, h_d, h_cd, n, n_elem, static_cast<hipStream_t>(stream));
}

}  // extern "C"
