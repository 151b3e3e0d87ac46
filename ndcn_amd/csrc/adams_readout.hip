// explicit_adams / fixed_adams inference: the Adams-Bashforth step that decodes its new state in the same launch.
//
//   ab_step_readout_f32     out = y + dt * sum_{i<n} a_i f_i as ab_step_f32 forms it (adams_step.h: ab1) AND dec[t] = Wd * s_t + bd for the
//                           <= 8 ticks the step reports - s_t the new state, or tick_emit_f32's expression of it for a tick strictly
//                           inside the step - while the row sits in registers / LDS: the hidden tick panels are never written
//
// Two kernels on the row layouts of the dense-output readout kernels (rk.hip: interp_readout_kernel, readout_narrow_kernel), which are
// the layouts of the decoder's two routes (linear.hip: linear_rowdot_kernel, linear_small_kernel), so that dec is bit for bit linear_f32
// of the panel.  FP contraction is OFF for this translation unit (the step's products and sums are rounded on their own); the decoder's
// chains are written with fmaf, as in rk.hip.  The kernels live apart from adams.hip, whose device code holds no fused multiply-add at
// all (tests/test_explicit_adams_host.py reads its ISA).
#include <stdint.h>

#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "adams_step.h"

namespace ndcn {

namespace {

// ------------------------------------------------------------------------------------------------ the step with the decoder
// ab_step_kernel's arithmetic on the row layouts of the two readout kernels of rk.hip, so that the new state is decoded by the
// Linear(H, C) while it sits in registers / LDS: dec[t] is bit for bit linear_f32 of the panel the step stores (tm[t] == 0) or of
// tick_emit_f32 of it (a tick strictly inside the step: tm[t] = t - t0 != 0).  The stored state is never transformed.
constexpr int kDecTileRows = 64;       // readout_narrow_kernel's tile

struct AbDecArgs {
    AbArgs s;
    float *dec[kDecMaxTicks];          // n_rows x C each
    float tm[kDecMaxTicks];
    int nt;
};

// solvers.py:103-108 after y0 was overwritten with y1 (rk.hip: emit1) - three roundings, -0 becomes +0 and Inf becomes NaN
__device__ __forceinline__ float ab_emit1(float v, float dt, float tm) { return v + ((v - v) / dt) * tm; }

// 64 <= H <= 512, the decoder's row-dot route.  A wave per row, lane l holds the elements l + 64 v (interp_readout_kernel): the
// N NV + NV loads of a row are issued before the first use; fmaf chain over v, xor butterfly, bias by lane 0 are linear_rowdot_kernel's.
template <int N, int NV>          // NV = ceil(H / 64) <= 8
__global__ __launch_bounds__(256) void ab_step_readout_kernel(AbDecArgs p, const float *__restrict__ Wd, const float *__restrict__ bd,
                                                              int64_t n_rows, int H, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave0; r < n_rows; r += n_waves) {
        float f[NV][N], y[NV], x[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int k = lane + 64 * v;                            // (only the last v has surplus lanes)
            const int64_t i = r * H + ((v < NV - 1 || k < H) ? k : H - 1);   // unconditional request; the surplus lanes are zeroed below
#pragma unroll
            for (int j = 0; j < N; ++j) f[v][j] = p.s.f[j][i];
            y[v] = p.s.y[i];
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int k = lane + 64 * v;
            x[v] = ab1(y[v], f[v], p.s.a, N, p.s.dt);
            if (v < NV - 1 || k < H) p.s.out[r * H + k] = x[v];
        }
        // (a run-time loop, as in interp_readout_kernel)
#pragma unroll 1
        for (int t = 0; t < p.nt; ++t) {
            const float tm = p.tm[t];
            float h[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                h[v] = tm != 0.f ? ab_emit1(x[v], p.s.dt, tm) : x[v];
                h[v] = (v < NV - 1 || lane + 64 * v < H) ? h[v] : 0.f;
            }
            for (int o = 0; o < C; ++o) {
                float acc = 0.f;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const int k = lane + 64 * v;
                    acc = fmaf(h[v], Wd[(int64_t)o * H + ((v < NV - 1 || k < H) ? k : H - 1)], acc);
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
                if (lane == 0) {
                    if (bd) acc += bd[o];
                    p.dec[t][r * C + o] = acc;
                }
            }
        }
    }
}

template <bool VEC>
__device__ __forceinline__ float4 ab_ldq(const float *p, int64_t q) {
    return VEC ? *reinterpret_cast<const float4 *>(p + 4 * q) : make_float4(p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]);
}

// H = 16, 20, .. 60, the decoder's small route: ONE in-order fma chain per (row, output).  readout_narrow_kernel's layout - a workgroup
// per tile of 64 rows, thread x holds the quads x + 256 j of the tile's contiguous span (coalesced 16-byte loads, the N + 1 of a quad
// issued before the first use), the new state goes to memory from registers and into an LDS tile [64][H + 1] per tick (two tiles
// alternate: one barrier per tick), lane l of wave w runs row l's chains for the outputs o = w, w + 4, w + 8, w + 12 < C with the
// decoder's rows read from LDS.  Rows past n_rows are neither read nor written.
template <int N, int NQ, bool VEC>          // NQ = ceil(H / 16) <= 4; VEC: every panel is 16-byte aligned
__global__ __launch_bounds__(256) void ab_step_readout_narrow_kernel(AbDecArgs p, const float *__restrict__ Wd,
                                                                     const float *__restrict__ bd, int64_t n_rows, int H, int C) {
    extern __shared__ float4 ab_narrow_smem[];                      // Wd [C][H] | bd [16] | two tiles [64][H + 1]
    float *Wl = reinterpret_cast<float *>(ab_narrow_smem);
    float *bl = Wl + C * H;
    float *tiles = bl + 16;
    const int tid = threadIdx.x, LD = H + 1, H4 = H / 4;
    const int row = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < C * H; i += 256) Wl[i] = Wd[i];
    if (tid < 16) bl[tid] = (bd && tid < C) ? bd[tid] : 0.f;
    const int64_t row0 = (int64_t)blockIdx.x * kDecTileRows;
    const int live = (int)(n_rows - row0 < kDecTileRows ? n_rows - row0 : kDecTileRows);
    const int nq_live = live * H4;                              // quads of the tile's live rows (<= 16 H)
    const int64_t q0 = row0 * H4;
    int lofs[NQ];                                                   // where quad j of this thread starts in a tile
    float4 x[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int e = 4 * (tid + 256 * j), r = e / H;
        lofs[j] = r * LD + (e - r * H);
        x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid + 256 * j < nq_live) {
            const int64_t q = q0 + tid + 256 * j;
            float4 v[N];
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] = ab_ldq<VEC>(p.s.f[i], q);
            const float4 y = ab_ldq<VEC>(p.s.y, q);
            float fx[N], fy[N], fz[N], fw[N];
#pragma unroll
            for (int i = 0; i < N; ++i) { fx[i] = v[i].x; fy[i] = v[i].y; fz[i] = v[i].z; fw[i] = v[i].w; }
            x[j].x = ab1(y.x, fx, p.s.a, N, p.s.dt);
            x[j].y = ab1(y.y, fy, p.s.a, N, p.s.dt);
            x[j].z = ab1(y.z, fz, p.s.a, N, p.s.dt);
            x[j].w = ab1(y.w, fw, p.s.a, N, p.s.dt);
            if (VEC) {
                *reinterpret_cast<float4 *>(p.s.out + 4 * q) = x[j];
            } else {
                p.s.out[4 * q] = x[j].x; p.s.out[4 * q + 1] = x[j].y; p.s.out[4 * q + 2] = x[j].z; p.s.out[4 * q + 3] = x[j].w;
            }
        }
    }
    // (the decoder's image is read behind the first tick's barrier)
#pragma unroll 1
    for (int t = 0; t < p.nt; ++t) {
        const float tm = p.tm[t], dt = p.s.dt;
        float *buf = tiles + (t & 1) * (kDecTileRows * LD);
#pragma unroll
        for (int j = 0; j < NQ; ++j)
            if (tid + 256 * j < nq_live) {
                float *h = buf + lofs[j];
                h[0] = tm != 0.f ? ab_emit1(x[j].x, dt, tm) : x[j].x;
                h[1] = tm != 0.f ? ab_emit1(x[j].y, dt, tm) : x[j].y;
                h[2] = tm != 0.f ? ab_emit1(x[j].z, dt, tm) : x[j].z;
                h[3] = tm != 0.f ? ab_emit1(x[j].w, dt, tm) : x[j].w;
            }
        __syncthreads();
        if (row < live && wv < C) {
            const float *s = buf + row * LD;
            const float4 *W4 = reinterpret_cast<const float4 *>(Wl);
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k4 = 0; k4 < H4; ++k4) {
                const float s0 = s[4 * k4], s1 = s[4 * k4 + 1], s2 = s[4 * k4 + 2], s3 = s[4 * k4 + 3];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int o = wv + 4 * j;                   // (wave-uniform)
                    if (o < C) {
                        const float4 w = W4[o * H4 + k4];
                        acc[j] = fmaf(s0, w.x, acc[j]);
                        acc[j] = fmaf(s1, w.y, acc[j]);
                        acc[j] = fmaf(s2, w.z, acc[j]);
                        acc[j] = fmaf(s3, w.w, acc[j]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = wv + 4 * j;
                if (o < C) {
                    float r = acc[j];
                    if (bd) r += bl[o];
                    p.dec[t][(row0 + row) * C + o] = r;
                }
            }
        }
    }
}

}  // namespace

namespace {

template <int N>
void ab_dec_launch_wide(const AbDecArgs &p, const float *Wd, const float *bd, int64_t n_rows, int H, int C, hipStream_t st) {
    const int g = stream_grid(n_rows * 64, 256);
#define NDCN_ABD(NV_) hipLaunchKernelGGL((ab_step_readout_kernel<N, NV_>), dim3(g), dim3(256), 0, st, p, Wd, bd, n_rows, H, C)
    switch ((H + 63) / 64) {
        case 1: NDCN_ABD(1); break;
        case 2: NDCN_ABD(2); break;
        case 3: NDCN_ABD(3); break;
        case 4: NDCN_ABD(4); break;
        case 5: NDCN_ABD(5); break;
        case 6: NDCN_ABD(6); break;
        case 7: NDCN_ABD(7); break;
        default: NDCN_ABD(8); break;
    }
#undef NDCN_ABD
}

template <int N>
void ab_dec_launch_narrow(const AbDecArgs &p, bool vec, const float *Wd, const float *bd, int64_t n_rows, int H, int C, hipStream_t st) {
    const int gn = (int)((n_rows + kDecTileRows - 1) / kDecTileRows);
    const size_t lds = ((size_t)C * H + 16 + 2 * (size_t)kDecTileRows * (H + 1)) * sizeof(float);         // <= 34.9 KB
#define NDCN_ABN(NQ_)                                                                                                                  \
    do {                                                                                                                               \
        if (vec) hipLaunchKernelGGL((ab_step_readout_narrow_kernel<N, NQ_, true>), dim3(gn), dim3(256), lds, st, p, Wd, bd, n_rows, H, C);  \
        else hipLaunchKernelGGL((ab_step_readout_narrow_kernel<N, NQ_, false>), dim3(gn), dim3(256), lds, st, p, Wd, bd, n_rows, H, C);     \
    } while (0)
    switch ((H + 15) / 16) {
        case 1: NDCN_ABN(1); break;
        case 2: NDCN_ABN(2); break;
        case 3: NDCN_ABN(3); break;
        default: NDCN_ABN(4); break;
    }
#undef NDCN_ABN
}

}  // namespace

// ab_step_f32 that also writes h_dec[t] = Wd * (the new state, through tick_emit_f32's expression where h_tm[t] != 0) + bd, t < nt <= 8,
// in the same pass: bit for bit linear_f32 of the panel.  H and C as interp_readout_supported; out may be y.
int ab_step_readout_f32(float *out, const float *y, const float *const *h_f, const float *h_a, int n_terms, float dt, int64_t n_rows, int H,
                        const float *Wd, const float *bd, int C, float *const *h_dec, const float *h_tm, int nt, hipStream_t st) {
    if (!interp_readout_supported(H, C)) {
        set_error("ab_step_readout: 64 <= H <= 512 or 16 <= H <= 60 in fours, and 1 <= C <= 15, got H = %d, C = %d", H, C);
        return NDCN_EINVAL;
    }
    if (n_terms < kAbMinTerms || n_terms > kAbMaxTerms) { set_error("ab_step_readout: %d terms, the orders are %d..%d", n_terms, kAbMinTerms, kAbMaxTerms); return NDCN_EINVAL; }
    if (!out || !y || !h_f || !h_a || !Wd || !h_dec || !h_tm || n_rows < 0) { set_error("ab_step_readout: null argument"); return NDCN_EINVAL; }
    if (nt < 1 || nt > kDecMaxTicks) { set_error("ab_step_readout: 1..%d ticks per launch", kDecMaxTicks); return NDCN_EINVAL; }
    AbDecArgs p;
    p.s.y = y; p.s.out = out; p.s.dt = dt;
    bool vec = aligned16(out) && aligned16(y);
    for (int j = 0; j < kAbMaxTerms; ++j) {
        p.s.f[j] = h_f[j < n_terms ? j : 0];
        p.s.a[j] = j < n_terms ? h_a[j] : 0.f;
        if (j >= n_terms) continue;
        if (!h_f[j]) { set_error("ab_step_readout: term %d is null", j); return NDCN_EINVAL; }
        if (h_f[j] == out) { set_error("ab_step_readout: out aliases history panel %d (only y may be updated in place)", j); return NDCN_EINVAL; }
        vec = vec && aligned16(h_f[j]);
    }
    p.nt = nt;
    for (int t = 0; t < kDecMaxTicks; ++t) {
        p.dec[t] = h_dec[t < nt ? t : 0];
        p.tm[t] = h_tm[t < nt ? t : 0];
        if (!p.dec[t] || p.dec[t] == out || p.dec[t] == y) { set_error("ab_step_readout: a decoded panel is null or aliases the state"); return NDCN_EINVAL; }
    }
    if (n_rows == 0) return NDCN_OK;
    if (H < 64 && (n_rows + kDecTileRows - 1) / kDecTileRows > 0x7fffffffll) {
        set_error("ab_step_readout: %lld rows are more tiles than one launch holds", (long long)n_rows);
        return NDCN_EINVAL;
    }
    const double P = (double)n_rows * H;
    ProfScope prof(PROF_COMBINE, st, 4.0 * P * (n_terms + 2) + 4.0 * nt * (double)n_rows * C, 2.0 * P * (n_terms + 1 + (3 + C) * nt));
#define NDCN_ABR(N_)                                                                        \
    do {                                                                                    \
        if (H < 64) ab_dec_launch_narrow<N_>(p, vec, Wd, bd, n_rows, H, C, st);             \
        else ab_dec_launch_wide<N_>(p, Wd, bd, n_rows, H, C, st);                           \
    } while (0)
    switch (n_terms) {
        case 3: NDCN_ABR(3); break;
        case 4: NDCN_ABR(4); break;
        case 5: NDCN_ABR(5); break;
        case 6: NDCN_ABR(6); break;
        case 7: NDCN_ABR(7); break;
        case 8: NDCN_ABR(8); break;
        case 9: NDCN_ABR(9); break;
        case 10: NDCN_ABR(10); break;
        default: NDCN_ABR(11); break;
    }
#undef NDCN_ABR
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

}  // namespace ndcn
