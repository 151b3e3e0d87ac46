// The decoder's backward inside the fixed-grid reverse sweep (training with odeint's `readout`): one streaming pass per tick that
//   - forms the tick's gradient from the (N, C) slice,  gi[n,h] = fma chain over c of gd[n,c] * Wd[c,h]  from +0  (what
//     the two-step form reads back from a materialised (T, N, H) tensor: g_dec . W_dec),
//   - adds it where the sweep adds g_out[i]:  out = a + ((((0 + p_0) + p_1) + ...) + gi)  - rk_combine_f32's order for the
//     unit-coefficient call lincomb(a_new, a, {gu..., gi}, {1, ...}) (rk.hip combine_kernel / wsum1: the sum starts from +0, the
//     base panel is added LAST; a product with 1.f is the value itself, so none is formed), so a sweep through this kernel keeps
//     the bits of the sweep over the materialised tensor.  Without a base panel and without addends out = gi (the last tick's seed),
//   - and accumulates the decoder's own gradients  g_Wd[c,h] += sum_n gd[n,c] y[n,h],  g_bd[c] += sum_n gd[n,c]  in fp64: every
//     product of two floats is exact in fp64; a thread adds its rows in ascending order, the block adds its threads' sums in thread
//     order through LDS and writes ONE partial per (c, h); a second small launch adds the blocks' partials in block order into the
//     caller's fp64 accumulator (C H + C doubles, converted to fp32 once after the last tick).  No float atomics: same inputs, same bits.
// Streams 3 + k panels (y, a, out, k addends): HBM-bound.  Wd lives in registers (C x 4 floats per lane).
// FP contraction is off as in rk.hip: the only fused operations are the explicit fmaf of the chain.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace ndcn {

namespace {

constexpr int kMaxAdd = 5;
constexpr int kMaxC = 15;
constexpr int kMaxBlocks = 1024;

struct RbArgs {
    float *out;
    const float *a;                 // nullable
    const float *add[kMaxAdd];
    int n_add;
    const float *gd, *Wd, *y;
    double *partial;                // nullable: no decoder gradients wanted;  [block][C H + C]
    int64_t n_rows;
    int H;
    int L;                          // lanes per row: H / 4 (16-byte lanes) or H
    int Lp;                         // lanes of a row served at once: min(L, 256)
    int G;                          // rows in flight per block: 256 / Lp (threads >= G * Lp idle)
    int64_t rpb;                    // rows per block, a multiple of G
};

template <int W> struct Vec;
template <> struct Vec<4> {
    static __device__ __forceinline__ void ld(const float *p, int64_t i, float (&v)[4]) {
        const float4 q = reinterpret_cast<const float4 *>(p)[i];
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    static __device__ __forceinline__ void st(float *p, int64_t i, const float (&v)[4]) {
        reinterpret_cast<float4 *>(p)[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
};
template <> struct Vec<1> {
    static __device__ __forceinline__ void ld(const float *p, int64_t i, float (&v)[1]) { v[0] = p[i]; }
    static __device__ __forceinline__ void st(float *p, int64_t i, const float (&v)[1]) { p[i] = v[0]; }
};

template <int C, int W>
__global__ __launch_bounds__(256) void readout_bwd_kernel(RbArgs p) {
    __shared__ double red[256 * W];
    __shared__ double redb[256];
    const int t = threadIdx.x, sub = t / p.Lp, lp = t - sub * p.Lp;
    const int64_t r0 = (int64_t)blockIdx.x * p.rpb, r1 = r0 + p.rpb < p.n_rows ? r0 + p.rpb : p.n_rows;
    const int64_t m = (int64_t)C * p.H + C;
    for (int l0 = 0; l0 < p.L; l0 += p.Lp) {          // (one pass unless a row has more than 256 lanes)
        const int lane = l0 + lp;
        const bool on = sub < p.G && lane < p.L;
        float w[C][W];
        double acc[C][W], accb[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            accb[c] = 0.0;
#pragma unroll
            for (int k = 0; k < W; ++k) { w[c][k] = 0.f; acc[c][k] = 0.0; }
            if (on) Vec<W>::ld(p.Wd, ((int64_t)c * p.H) / W + lane, w[c]);
        }
        if (on) {
            for (int64_t r = r0 + sub; r < r1; r += p.G) {
                const int64_t i = r * p.L + lane;
                float g[C], gi[W], s[W], v[W];
#pragma unroll
                for (int c = 0; c < C; ++c) g[c] = p.gd[r * C + c];
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    float x = 0.f;
#pragma unroll
                    for (int c = 0; c < C; ++c) x = fmaf(g[c], w[c][k], x);
                    gi[k] = x;
                }
                if (p.n_add > 0 || p.a) {
                    if (p.n_add > 0) {
                        Vec<W>::ld(p.add[0], i, v);
#pragma unroll
                        for (int k = 0; k < W; ++k) s[k] = 0.f + v[k];
#pragma unroll
                        for (int j = 1; j < kMaxAdd; ++j)
                            if (j < p.n_add) {
                                Vec<W>::ld(p.add[j], i, v);
#pragma unroll
                                for (int k = 0; k < W; ++k) s[k] = s[k] + v[k];
                            }
#pragma unroll
                        for (int k = 0; k < W; ++k) s[k] = s[k] + gi[k];
                    } else {
#pragma unroll
                        for (int k = 0; k < W; ++k) s[k] = 0.f + gi[k];
                    }
                    if (p.a) {
                        Vec<W>::ld(p.a, i, v);
#pragma unroll
                        for (int k = 0; k < W; ++k) s[k] = v[k] + s[k];
                    }
                    Vec<W>::st(p.out, i, s);
                } else {
                    Vec<W>::st(p.out, i, gi);
                }
                if (p.partial) {
                    Vec<W>::ld(p.y, i, v);
#pragma unroll
                    for (int c = 0; c < C; ++c) {
#pragma unroll
                        for (int k = 0; k < W; ++k) acc[c][k] += (double)g[c] * (double)v[k];
                        if (lane == 0) accb[c] += (double)g[c];
                    }
                }
            }
        }
        if (!p.partial) continue;
        double *dst = p.partial + (int64_t)blockIdx.x * m;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < W; ++k) red[t * W + k] = acc[c][k];
            if (lp == 0) redb[sub] = accb[c];
            __syncthreads();
            if (sub == 0 && lane < p.L) {
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    double x = acc[c][k];
                    for (int q = 1; q < p.G; ++q) x += red[(q * p.Lp + lp) * W + k];
                    dst[(int64_t)c * p.H + (int64_t)lane * W + k] = x;
                }
            }
            if (t == 0 && l0 == 0) {
                double x = accb[c];
                for (int q = 1; q < p.G; ++q) x += redb[q];
                dst[(int64_t)C * p.H + c] = x;
            }
        }
    }
}

// acc[j] += partial[0][j] + partial[1][j] + ...  (block order)
__global__ __launch_bounds__(256) void readout_bwd_sum_kernel(const double *__restrict__ partial, int nb, int64_t m, double *__restrict__ acc) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    double s = partial[j];
#pragma unroll 8
    for (int b = 1; b < nb; ++b) s += partial[(int64_t)b * m + j];
    acc[j] = acc[j] + s;
}

__global__ __launch_bounds__(256) void readout_bwd_finish_kernel(const double *__restrict__ acc, float *__restrict__ g_Wd, float *__restrict__ g_bd,
                                                                 int64_t ch, int C) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < ch) g_Wd[j] = (float)acc[j];
    else if (j < ch + C && g_bd) g_bd[j - ch] = (float)acc[j];
}

struct Shape {
    int W, L, Lp, G, nb;
    int64_t rpb;
};

Shape shape_of(int64_t n_rows, int H, bool vec) {
    Shape s;
    s.W = vec ? 4 : 1;
    s.L = H / s.W;
    s.Lp = s.L < 256 ? s.L : 256;
    s.G = 256 / s.Lp;
    int64_t want = (n_rows + s.G - 1) / s.G;
    if (want > kMaxBlocks) want = kMaxBlocks;
    if (want < 1) want = 1;
    int64_t rpb = (n_rows + want - 1) / want;
    rpb = (rpb + s.G - 1) / s.G * s.G;
    if (rpb < s.G) rpb = s.G;
    s.rpb = rpb;
    s.nb = (int)((n_rows + rpb - 1) / rpb);
    if (s.nb < 1) s.nb = 1;
    return s;
}

template <int C>
void launch(const RbArgs &p, int W, int nb, hipStream_t st) {
    if (W == 4) hipLaunchKernelGGL((readout_bwd_kernel<C, 4>), dim3(nb), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((readout_bwd_kernel<C, 1>), dim3(nb), dim3(256), 0, st, p);
}

}  // namespace

int readout_bwd_supported(int H, int C) { return H >= 1 && C >= 1 && C <= kMaxC; }

// the partials of one call: the scalar shape never has fewer blocks x entries than the 16-byte one
int64_t readout_bwd_ws_bytes(int64_t n_rows, int H, int C) {
    if (!readout_bwd_supported(H, C) || n_rows < 1) return 0;
    const Shape a = shape_of(n_rows, H, false);
    int nb = a.nb;
    if (H % 4 == 0) {
        const Shape b = shape_of(n_rows, H, true);
        if (b.nb > nb) nb = b.nb;
    }
    return (int64_t)nb * ((int64_t)C * H + C) * (int64_t)sizeof(double);
}

int readout_bwd_f32(float *out, const float *a, const float *const *h_add, int n_add, const float *gd, const float *Wd, const float *y,
                    int64_t n_rows, int H, int C, double *acc, void *ws, hipStream_t st) {
    if (!readout_bwd_supported(H, C)) { set_error("readout_bwd: H >= 1 and 1 <= C <= %d are supported (H = %d, C = %d)", kMaxC, H, C); return NDCN_EINVAL; }
    NDCN_CHECK_ARG(out && gd && Wd && n_rows >= 0 && n_add >= 0 && n_add <= kMaxAdd && (n_add == 0 || h_add), "bad argument");
    NDCN_CHECK_ARG(!acc || (y && ws), "the decoder gradients need the tick's state and the partials' scratch");
    if (n_rows == 0) return NDCN_OK;
    RbArgs p = {};
    bool vec = H % 4 == 0 && aligned16(out) && aligned16(Wd) && (!a || aligned16(a)) && (!acc || aligned16(y));
    for (int j = 0; j < kMaxAdd; ++j) {
        p.add[j] = j < n_add ? h_add[j] : nullptr;
        if (j < n_add) {
            NDCN_CHECK_ARG(h_add[j], "null addend");
            vec = vec && aligned16(h_add[j]);
        }
    }
    const Shape s = shape_of(n_rows, H, vec);
    p.out = out; p.a = a; p.n_add = n_add; p.gd = gd; p.Wd = Wd; p.y = y;
    p.partial = acc ? static_cast<double *>(ws) : nullptr;
    p.n_rows = n_rows; p.H = H; p.L = s.L; p.Lp = s.Lp; p.G = s.G; p.rpb = s.rpb;
    const double panels = 2.0 + (a ? 1 : 0) + n_add;
    ProfScope prof(PROF_COMBINE, st, 4.0 * n_rows * H * panels, 2.0 * n_rows * H * (C + n_add + (acc ? C : 0)));
    switch (C) {
#define NDCN_RB_CASE(c) case c: launch<c>(p, s.W, s.nb, st); break;
        NDCN_RB_CASE(1) NDCN_RB_CASE(2) NDCN_RB_CASE(3) NDCN_RB_CASE(4) NDCN_RB_CASE(5) NDCN_RB_CASE(6) NDCN_RB_CASE(7) NDCN_RB_CASE(8)
        NDCN_RB_CASE(9) NDCN_RB_CASE(10) NDCN_RB_CASE(11) NDCN_RB_CASE(12) NDCN_RB_CASE(13) NDCN_RB_CASE(14) NDCN_RB_CASE(15)
#undef NDCN_RB_CASE
    }
    NDCN_LAUNCH_CHECK();
    if (acc) {
        const int64_t m = (int64_t)C * H + C;
        hipLaunchKernelGGL(readout_bwd_sum_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, p.partial, s.nb, m, acc);
        NDCN_LAUNCH_CHECK();
    }
    return NDCN_OK;
}

int readout_bwd_finish_f32(const double *acc, float *g_Wd, float *g_bd, int H, int C, hipStream_t st) {
    NDCN_CHECK_ARG(acc && g_Wd && readout_bwd_supported(H, C), "bad argument");
    const int64_t ch = (int64_t)C * H;
    hipLaunchKernelGGL(readout_bwd_finish_kernel, dim3((unsigned)((ch + C + 255) / 256)), dim3(256), 0, st, acc, g_Wd, g_bd, ch, C);
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

}  // namespace ndcn
