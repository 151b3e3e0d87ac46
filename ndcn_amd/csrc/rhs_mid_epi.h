// The tile constants and the per-lane epilogue that the one-launch right-hand sides for hidden widths 16..128 share: rhs_mid.hip
// (K = relu(W (A X) + b)) and rhs_abl.hip (the no_control and no_graph ablations).  A lane holds four consecutive elements of K,
// idx = row * H + 4 q: it applies the dropout factor (DROP; csrc/dropout.h, idx >> 2 is one Philox group), stores K, reads the
// row-local panels at idx and writes y_next / y_aux with the stage algebra of the STAND-ALONE kernels (rk.hip: wsum1 from +0, stage1)
// - the composed form of rhs.hip, bit for bit.
#pragma once
#include "dropout.h"

#pragma clang fp contract(off)

namespace ndcn {

constexpr int kMidTile = 64;          // rows per tile: two 32-row MFMA tiles
constexpr int kMidThreads = 512;
constexpr int kMidMaxPrev = 5;
constexpr int kMidMinH = 16, kMidMaxH = 128;
constexpr int kLdsPerCu = 160 * 1024;
enum { MID_PLAIN = 0, MID_COMBINE = 1, MID_RK4 = 3 };

struct MidEpi {
    const float *y0;
    const float *kprev[kMidMaxPrev];
    float *y_next;
    float *y_aux;                     // COMBINE, nullable: second linear combination (no y0)
    float c[kMidMaxPrev + 1];
    float c2[kMidMaxPrev + 1];
    int n_prev;
};

__device__ __forceinline__ float4 mid_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void mid_st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ void mid_fma4(float4 &a, float v, const float4 &x) {
    a.x = fmaf(v, x.x, a.x); a.y = fmaf(v, x.y, a.y); a.z = fmaf(v, x.z, a.z); a.w = fmaf(v, x.w, a.w);
}

// rk.hip wsum1 over {km[0..np), kn}: (0 + c_0 k_0) + c_1 k_1 + ..., the new stage last, every product rounded on its own
__device__ __forceinline__ float mid_wsum(const float *c, const float (&km)[kMidMaxPrev], float kn, int np) {
    float acc = 0.f + c[0] * (np > 0 ? km[0] : kn);
#pragma unroll
    for (int m = 1; m < kMidMaxPrev; ++m)
        if (m < np) acc = acc + c[m] * km[m];
    if (np > 0) acc = acc + c[np] * kn;
    return acc;
}

// rk.hip stage1<2..5> with the new stage as the last of {km[0..np), kn}  (rk_common.py:75-78).  Stage 1: fixed_stage_kernel<3, true> is
// compiled as k2 - k1 / 3 for stage1<3>'s k1 / -3 + k2 - every bit the same except the sign of a NaN that k1 carries through.  The
// quotient is pinned in a register here so that the subtraction stays one and even that sign agrees.
__device__ __forceinline__ float mid_rk4(float y, const float (&km)[kMidMaxPrev], float kn, int np, float dt) {
    if (np == 0) return y + dt * kn / 3.f;
    if (np == 1) {
        float q = km[0] / 3.f;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(q));
#endif
        return y + dt * (kn - q);
    }
    if (np == 2) return y + dt * (km[0] - km[1] + kn);
    return y + (km[0] + 3.f * km[1] + 3.f * km[2] + kn) * (dt / 8.f);
}

// CDEV - a replayed adaptive step (solver.hip), whose step size lives in device memory: the coefficients come from `c_dev` instead of
// MidEpi::c, with the meaning rhs_small_f32 / spmm_rec_f32 give that argument - COMBINE reads c_dev[m], m <= n_prev, the fl(dt * beta) image
// that the graph's first kernel writes; never together with y_aux.  (COMBINE only: no step replays an RK4 launch - the fixed grids pass
// dt by value -, so that form is not instantiated until it has a caller.)  The address is the same for every lane and
// the loads stand at the kernel's entry, before its first store: scalar loads into SGPRs, once per workgroup, and the new stage's
// coefficient c[n_prev] is picked there too - the epilogue loop holds no more vector registers than the by-value form, which indexes
// its kernel argument.  The arithmetic behind the fetch is mid_wsum's / mid_rk4's.
struct MidCoef {
    float c[kMidMaxPrev + 1];
    float cn;                         // c[n_prev]
};

__device__ __forceinline__ MidCoef mid_coef_dev(const float *c_dev, int np) {
    MidCoef k;
#pragma unroll
    for (int m = 0; m <= kMidMaxPrev; ++m) k.c[m] = m <= np ? c_dev[m] : 0.f;
    k.cn = c_dev[np];            // (a load of its own: a select chain over c[] would run on the vector unit)
    return k;
}

// mid_wsum with the coefficients of MidCoef: the same products and sums in the same order
__device__ __forceinline__ float mid_wsum_dev(const MidCoef &k, const float (&km)[kMidMaxPrev], float kn, int np) {
    float acc = 0.f + k.c[0] * (np > 0 ? km[0] : kn);
#pragma unroll
    for (int m = 1; m < kMidMaxPrev; ++m)
        if (m < np) acc = acc + k.c[m] * km[m];
    if (np > 0) acc = acc + k.cn * kn;
    return acc;
}

// One lane's share of the epilogue: kn = K[idx .. idx + 4) as the launch formed it (behind the ReLU).  The statements of
// rhs_mid_kernel's epilogue loop, which keeps its own copy (see there); rhs_abl.hip's kernels call this one.  kc: read under CDEV only.
template <int MODE, bool DROP, bool CDEV = false>
__device__ __forceinline__ void mid_epi_lane(float4 kn, size_t idx, float *K, const MidEpi &e, const DropArgs &d, const MidCoef &kc) {
    if (DROP) {                                          // K' = K * m: stored, and the K of everything below
        const Philox4 o = drop_words<true>(d, (int64_t)(idx >> 2));
        kn.x = kn.x * (o.w[0] >= d.thresh ? d.s : 0.f);
        kn.y = kn.y * (o.w[1] >= d.thresh ? d.s : 0.f);
        kn.z = kn.z * (o.w[2] >= d.thresh ? d.s : 0.f);
        kn.w = kn.w * (o.w[3] >= d.thresh ? d.s : 0.f);
    }
    mid_st4(K + idx, kn);
    if (MODE == MID_PLAIN) return;
    const int np = e.n_prev;
    const float4 y = mid_ld4(e.y0 + idx);
    float kx[kMidMaxPrev], ky[kMidMaxPrev], kz[kMidMaxPrev], kw[kMidMaxPrev];
#pragma unroll
    for (int m = 0; m < kMidMaxPrev; ++m) {
        const float4 v = m < np ? mid_ld4(e.kprev[m] + idx) : make_float4(0.f, 0.f, 0.f, 0.f);
        kx[m] = v.x; ky[m] = v.y; kz[m] = v.z; kw[m] = v.w;
    }
    if (MODE == MID_RK4) {
        const float dt = e.c[0];
        mid_st4(e.y_next + idx, make_float4(mid_rk4(y.x, kx, kn.x, np, dt), mid_rk4(y.y, ky, kn.y, np, dt),
                                            mid_rk4(y.z, kz, kn.z, np, dt), mid_rk4(y.w, kw, kn.w, np, dt)));
        return;
    }
    if (CDEV) {
        mid_st4(e.y_next + idx, make_float4(y.x + mid_wsum_dev(kc, kx, kn.x, np), y.y + mid_wsum_dev(kc, ky, kn.y, np),
                                            y.z + mid_wsum_dev(kc, kz, kn.z, np), y.w + mid_wsum_dev(kc, kw, kn.w, np)));
        return;
    }
    mid_st4(e.y_next + idx, make_float4(y.x + mid_wsum(e.c, kx, kn.x, np), y.y + mid_wsum(e.c, ky, kn.y, np),
                                        y.z + mid_wsum(e.c, kz, kn.z, np), y.w + mid_wsum(e.c, kw, kn.w, np)));
    if (e.y_aux)
        mid_st4(e.y_aux + idx, make_float4(mid_wsum(e.c2, kx, kn.x, np), mid_wsum(e.c2, ky, kn.y, np),
                                           mid_wsum(e.c2, kz, kn.z, np), mid_wsum(e.c2, kw, kn.w, np)));
}

// the host side of MidEpi: the stage arguments of rhs_rk_f32 (mode != MID_PLAIN).  Under c_dev the launch reads neither c nor c2 (h_c then
// holds the bare tableau entries of the replayed step)
inline void mid_epi_fill(MidEpi &e, int mode, const float *y0, const float *const *h_kprev, const float *h_c, int n_prev, float *y_next,
                         float *y_aux, const float *c_aux) {
    e.y0 = y0; e.y_next = y_next; e.n_prev = n_prev;
    e.y_aux = (mode == MID_COMBINE && y_aux && c_aux) ? y_aux : nullptr;
    for (int m = 0; m < n_prev; ++m) e.kprev[m] = h_kprev[m];
    if (mode == MID_RK4) e.c[0] = h_c[0];
    else for (int m = 0; m <= n_prev; ++m) { e.c[m] = h_c[m]; e.c2[m] = e.y_aux ? c_aux[m] : 0.f; }
}

}  // namespace ndcn
