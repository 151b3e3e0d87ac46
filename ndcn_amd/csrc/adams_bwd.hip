// explicit_adams under a gradient: the part of the reverse sweep that is specific to a linear multistep method.  The evaluation f_i
// of grid step i is a term of up to eleven later Adams-Bashforth steps, so its gradient GATHERS from the adjoints of their states:
//
//   ab_adjoint_f32     out = [base +] (((0 + c_0 g_0) + c_1 g_1) + ... + c_{n-1} g_{n-1}), n = 1..11: one streaming pass that reads the
//                      n adjoint panels (and the base) and writes one - the scatter form would be 2n read-modify-write passes
//
// c_q = fl32(dt * a_q) is formed on the host (core.ab_adjoint_terms).  Every product and sum is rounded on its own and the base is
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

}  // namespace ndcn

using namespace ndcn;

extern "C" {

int ndcn_ab_adjoint_f32(float *out, const float *base, const float *const *h_g, const float *h_c, int n, int64_t n_elem, void *stream) {
    return ab_adjoint_f32(out, base, h_g, h_c, n, n_elem, static_cast<hipStream_t>(stream));
}

}  // extern "C"
