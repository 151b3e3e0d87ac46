// K = relu(W (A X) + b)  (neural_dynamics.py:27-36) plus the Runge-Kutta algebra that consumes K, in ONE launch, for hidden widths
// 16 <= H <= 128 (H a multiple of 4) at ANY number of rows - the widths between the narrow-panel kernel (rhs_small.hip: n H <= 2^18)
// and the H = 256 kernels, which otherwise run composed: row SpMM into a scratch panel S, MFMA Linear reading S and writing K, a
// stand-alone stage kernel reading K again (rhs.hip).  Here S never leaves the CU and K is consumed where it is formed: a COMBINE
// launch with j earlier stages moves about (j + 4) panels instead of (j + 7).
//
//   workgroup = 8 waves, persistent over a contiguous run of 64-row tiles; W (H x H fp32 <= 64 KiB) is staged into LDS once per
//   workgroup - zero-padded to P = ceil32(H) in both dimensions - and stays there.  Per tile, all 8 waves in every phase but the second:
//     gather   P / 4 (rounded up to a power of two) lanes per row, each 4 columns wide: S[r, c] as ONE fma per stored entry in stored
//              order from +0 - the chain of spmm_csr_kernel (tests/_fma_chain.py) - four entries' loads in flight at a time; the S
//              tile (64 x P, columns beyond H zero) goes to LDS
//     linear   wave w < 2 (P / 32) owns the 32 x 32 output tile (rows 32 (w & 1), columns 32 (w >> 1)): v_mfma_f32_32x32x2_f32 over
//              k = 0, 2, .. P - 2 from a zero accumulator - the instruction sequence of linear_mfma_kernel, whose k chunks are
//              zero-padded to 32 in the same way - then + b and the NaN-passing ReLU; the K tile replaces the S tile in LDS
//     epilogue 16 bytes per lane over the tile: K is stored, the row-local panels (y0, earlier stages) are read and y_next / y_aux
//              written with the stage algebra of the STAND-ALONE kernels (rk.hip: wsum1 from +0, stage1): the composed form
//   => every panel the launch writes equals the composed path's bit for bit, signs of zero and NaN positions included; the switch
//   (ndcn_set_rhs_mid / NDCN_RHS_MID, off by default) is invisible in the results.
//
// Dropout (DROP; the contract is csrc/dropout.h): a lane of the epilogue owns the four consecutive elements idx = gr H + 4 q, and H is a
// multiple of 4, so idx >> 2 is exactly one Philox group - ONE drop_words call per lane (the rolled form: the round keys are formed as
// the loop goes, not held in registers), both counter words from the 64-bit index.  K' = K * (w >= T ? s : 0), one rounded product per
// element behind the ReLU (NaN * 0 and Inf * 0 stay NaN), is what the launch stores as K and what the unchanged stage algebra - y_aux
// included - consumes: the bits of the composed launches followed by dropout_apply_f32 / dropout_combine_f32 and the stand-alone stage
// kernel.  The DROP = false instantiations are the kernels they were.  A switch of its own (ndcn_set_rhs_mid_drop /
// NDCN_RHS_MID_DROP, off by default) lets the dropout calls take the route where the mode above takes the shape.
//
// The error record is not formed here: an ERROR launch is this kernel in PLAIN mode followed by rk_error_f32 (rhs.hip), which keeps
// the record's summation order.  No halo panel, none of the RkOpt fields of the H = 256 launches: rhs.hip declines those.
#include <atomic>

#include "kernels.h"
#include "rhs_mid_epi.h"

#pragma clang fp contract(off)

namespace ndcn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Mode 1 stops here.  Beyond it P = 128: 99 072 bytes of LDS, ONE workgroup per CU, so a tile's gather, MFMA and epilogue phases run
// one after the other with nothing to overlap them - measured slower than the composed path (tools/micro/rhs_mid_time.py, 99 856 rows,
// H = 128: plain 0.107 ms against 0.080 ms, COMBINE 5 0.185 against 0.160).  Mode 2 still takes those widths.  The dropout form follows
// the same bound: with --dropout 0.5 there H = 128 ran plain 0.119 ms against 0.095 composed and COMBINE 5 0.188 against 0.164, while
// H = 96 was not slower (plain 0.076 against 0.076, COMBINE 5 0.120 against 0.131).
constexpr int kMidMode1MaxH = 96;

struct MidArgs {
    const int *rowptr, *colidx;
    const float *val;
    const float *X;
    const float *W, *bias;
    float *K;
    int n_rows, H, relu;
    int lsh;                          // log2 of the lanes that gather one row
};

// The tile constants, MidEpi, mid_wsum and mid_rk4 are rhs_mid_epi.h's, shared with rhs_abl.hip.  The epilogue below stays written out
// in this kernel: calling the header's mid_epi_lane instead - the same statements - made the compiler schedule and allocate the six
// instantiations differently, and they are to stay the kernels that were measured.
template <int MODE, bool DROP, bool CDEV = false>
__global__ __launch_bounds__(kMidThreads) void rhs_mid_kernel(MidArgs a, MidEpi e, DropArgs d, const float *c_dev) {
    extern __shared__ __align__(16) float mid_lds[];
    const int H = a.H, n = a.n_rows;
    const int P = (H + 31) & ~31;                            // H padded to the MFMA tile: k steps and output columns
    const int ld = P + 1;                                    // odd leading dimension: the column-ish operand reads are conflict-free
    const int H4 = H >> 2;
    float *s_W = mid_lds;                                    // [P][ld]  s_W[o * ld + k] = W[o][k], zero beyond H
    float *s_T = mid_lds + P * ld;                           // [64][ld] the S tile; then [64][P] the K tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < P * P; i += kMidThreads) {
        const int o = i / P, k = i - o * P;
        s_W[o * ld + k] = (o < H && k < H) ? a.W[o * H + k] : 0.f;
    }
    // the workgroup's run of tiles: n_tiles split evenly, the first `rem` workgroups one more
    const int n_tiles = (n + kMidTile - 1) / kMidTile;
    const int base = n_tiles / (int)gridDim.x, rem = n_tiles % (int)gridDim.x;
    const int b = blockIdx.x;
    const int t0 = b * base + (b < rem ? b : rem), t1 = t0 + base + (b < rem ? 1 : 0);
    // gather roles
    const int lsh = a.lsh;
    const int g = tid >> lsh, c4 = (tid & ((1 << lsh) - 1)) * 4, rows_per_pass = kMidThreads >> lsh;
    const bool act = c4 < H, pad = c4 < P;
    // linear roles
    const int n_jobs = 2 * (P >> 5);
    const int wm = wave & 1, tn = wave >> 1;
    const int on = tn * 32 + (lane & 31);
    const float bv = (wave < n_jobs && a.bias && on < H) ? a.bias[on] : 0.f;
    const int np = e.n_prev;
    MidCoef kc = {};                                         // CDEV: the coefficients, scalar loads at the kernel's entry (rhs_mid_epi.h)
    if (CDEV) kc = mid_coef_dev(c_dev, np);
    for (int t = t0; t < t1; ++t) {
        const int r0 = t * kMidTile;
        // ---- gather: S = (A X)[r0 .. r0 + 64, :]
        for (int row = g; row < kMidTile; row += rows_per_pass) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            const int gr = r0 + row;
            if (gr < n && act) {
                int j = a.rowptr[gr];
                const int j1 = a.rowptr[gr + 1];
                const float *xc = a.X + c4;
                for (; j + 4 <= j1; j += 4) {
                    const int q0 = a.colidx[j], q1 = a.colidx[j + 1], q2 = a.colidx[j + 2], q3 = a.colidx[j + 3];
                    const float v0 = a.val[j], v1 = a.val[j + 1], v2 = a.val[j + 2], v3 = a.val[j + 3];
                    const float4 x0 = mid_ld4(xc + (size_t)q0 * H), x1 = mid_ld4(xc + (size_t)q1 * H);
                    const float4 x2 = mid_ld4(xc + (size_t)q2 * H), x3 = mid_ld4(xc + (size_t)q3 * H);
                    mid_fma4(s, v0, x0); mid_fma4(s, v1, x1); mid_fma4(s, v2, x2); mid_fma4(s, v3, x3);
                }
                for (; j < j1; ++j) mid_fma4(s, a.val[j], mid_ld4(xc + (size_t)a.colidx[j] * H));
            }
            if (pad) {
                float *d = s_T + row * ld + c4;
                d[0] = s.x; d[1] = s.y; d[2] = s.z; d[3] = s.w;
            }
        }
        __syncthreads();
        // ---- linear: one 32 x 32 output tile per wave, k ascending from a zero accumulator
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        if (wave < n_jobs) {
            const float *pa = s_T + (wm * 32 + (lane & 31)) * ld + (lane >> 5);
            const float *pb = s_W + on * ld + (lane >> 5);
            for (int k0 = 0; k0 < P; k0 += 32)
#pragma unroll
                for (int k = 0; k < 32; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[k0 + k], pb[k0 + k], acc, 0, 0, 0);
        }
        __syncthreads();                                     // every wave has read its S rows: the K tile takes their place
        if (wave < n_jobs) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                float v = acc[r] + bv;
                if (a.relu) v = relu_nan(v);
                s_T[m * P + on] = v;
            }
        }
        __syncthreads();
        // ---- epilogue: 4 columns per lane
        for (int i = tid; i < kMidTile * H4; i += kMidThreads) {
            const int row = i / H4, q = i - row * H4;
            const int gr = r0 + row;
            if (gr >= n) continue;
            float4 kn = mid_ld4(s_T + row * P + 4 * q);
            const size_t idx = (size_t)gr * H + 4 * q;
            if (DROP) {                                      // K' = K * m: stored, and the K of everything below
                const Philox4 o = drop_words<true>(d, (int64_t)(idx >> 2));
                kn.x = kn.x * (o.w[0] >= d.thresh ? d.s : 0.f);
                kn.y = kn.y * (o.w[1] >= d.thresh ? d.s : 0.f);
                kn.z = kn.z * (o.w[2] >= d.thresh ? d.s : 0.f);
                kn.w = kn.w * (o.w[3] >= d.thresh ? d.s : 0.f);
            }
            mid_st4(a.K + idx, kn);
            if (MODE == MID_PLAIN) continue;
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
                continue;
            }
            if (CDEV) {
                mid_st4(e.y_next + idx, make_float4(y.x + mid_wsum_dev(kc, kx, kn.x, np), y.y + mid_wsum_dev(kc, ky, kn.y, np),
                                                    y.z + mid_wsum_dev(kc, kz, kn.z, np), y.w + mid_wsum_dev(kc, kw, kn.w, np)));
                continue;
            }
            mid_st4(e.y_next + idx, make_float4(y.x + mid_wsum(e.c, kx, kn.x, np), y.y + mid_wsum(e.c, ky, kn.y, np),
                                                y.z + mid_wsum(e.c, kz, kn.z, np), y.w + mid_wsum(e.c, kw, kn.w, np)));
            if (e.y_aux)
                mid_st4(e.y_aux + idx, make_float4(mid_wsum(e.c2, kx, kn.x, np), mid_wsum(e.c2, ky, kn.y, np),
                                                   mid_wsum(e.c2, kz, kn.z, np), mid_wsum(e.c2, kw, kn.w, np)));
        }
        __syncthreads();                                     // the next tile's gather overwrites the K tile
    }
}

// ---------------------------------------------------------------------------------------------------- the switch
static std::atomic<int> g_mid_override{-1};                // ndcn_set_rhs_mid: -1 = the environment's mode
static int clamp_mode(int m) { return m < 0 ? 0 : (m > 2 ? 2 : m); }

int rhs_mid_mode() {
    const int ov = g_mid_override.load(std::memory_order_relaxed);
    if (ov >= 0) return ov;
    static const int env_mode = clamp_mode(env_int("NDCN_RHS_MID", 0));
    return env_mode;
}

int set_rhs_mid(int mode) {
    const int prev = rhs_mid_mode();
    g_mid_override.store(mode < 0 ? -1 : clamp_mode(mode), std::memory_order_relaxed);
    return prev;
}

// the dropout form's own switch (ndcn_set_rhs_mid_drop / NDCN_RHS_MID_DROP): effective only where rhs_mid_mode() takes the shape
static std::atomic<int> g_mid_drop_override{-1};           // -1 = the environment's value

int rhs_mid_drop_on() {
    const int ov = g_mid_drop_override.load(std::memory_order_relaxed);
    if (ov >= 0) return ov;
    static const int env_on_ = env_int("NDCN_RHS_MID_DROP", 0) > 0 ? 1 : 0;
    return env_on_;
}

int set_rhs_mid_drop(int on) {
    const int prev = rhs_mid_drop_on();
    g_mid_drop_override.store(on < 0 ? -1 : (on ? 1 : 0), std::memory_order_relaxed);
    return prev;
}

// From the sizes alone.  Mode 1 leaves to rhs_small.hip what that kernel takes and to the composed path the widths above
// kMidMode1MaxH; mode 2 takes every supported shape.
int rhs_mid_supported(int64_t n_rows, int H, uint32_t flags, int mode) {
    if (mode != 1 && mode != 2) return 0;
    if (n_rows < 1 || n_rows >= ((int64_t)1 << 31) - kMidTile || H < kMidMinH || H > kMidMaxH || (H & 3)) return 0;
    if (flags & (NDCN_F_NO_GRAPH | NDCN_F_NO_CONTROL)) return 0;
    if (mode == 1 && (H > kMidMode1MaxH || rhs_small_wanted(n_rows, H, flags))) return 0;
    return 1;
}

static size_t mid_lds_bytes(int H) {
    const size_t P = (size_t)((H + 31) & ~31);
    return (P + kMidTile) * (P + 1) * sizeof(float);
}

int rhs_mid_f32(const ndcn_csr *A, const float *X, const float *W, const float *b, float *K, int H, uint32_t flags, int mode,
                const float *y0, const float *const *h_kprev, const float *h_c, int n_prev, float *y_next, hipStream_t st,
                const RkOpt *opt, const DropArgs *drop, const float *c_dev) {
    const int n_rows = (int)A->n_rows;
    if (n_rows == 0) return NDCN_OK;
    if (H < kMidMinH || H > kMidMaxH || (H & 3)) { set_error("rhs_mid: H must be a multiple of 4 in 16..128"); return NDCN_EINVAL; }
    if (mode != MID_PLAIN && mode != MID_COMBINE && mode != MID_RK4) { set_error("rhs_mid: bad mode"); return NDCN_EINVAL; }
    if (n_prev < 0 || n_prev > kMidMaxPrev || (mode == MID_RK4 && n_prev > 3)) { set_error("rhs_mid: bad stage count"); return NDCN_EINVAL; }
    if (drop && !(flags & NDCN_F_RELU)) { set_error("rhs_mid: dropout without the ReLU"); return NDCN_EINVAL; }
    if (c_dev && (mode != MID_COMBINE || drop || (opt && opt->y_aux))) { set_error("rhs_mid: c_dev goes with COMBINE, without dropout or y_aux"); return NDCN_EINVAL; }
    MidArgs a;
    a.rowptr = A->rowptr; a.colidx = A->colidx; a.val = A->val; a.X = X; a.W = W; a.bias = b; a.K = K;
    a.n_rows = n_rows; a.H = H; a.relu = (flags & NDCN_F_RELU) ? 1 : 0;
    const int P = (H + 31) & ~31;
    a.lsh = P <= 32 ? 3 : (P <= 64 ? 4 : 5);
    MidEpi e = {};
    if (mode != MID_PLAIN) mid_epi_fill(e, mode, y0, h_kprev, h_c, n_prev, y_next, opt ? opt->y_aux : nullptr, opt ? opt->c_aux : nullptr);
    const size_t lds = mid_lds_bytes(H);
    int per_cu = (int)(kLdsPerCu / lds);                   // H = 128: 1, H = 64: 4
    if (per_cu > 4) per_cu = 4;                            // 2048 threads per CU
    const int n_tiles = (n_rows + kMidTile - 1) / kMidTile;
    const int grid = n_tiles < kCus * per_cu ? n_tiles : kCus * per_cu;
    const double Pn = 4.0 * H * (double)n_rows;
    double bytes = 8.0 * A->nnz + 4.0 * (n_rows + 1) + 4.0 * H * (double)(A->n_rows + A->n_cols) + 4.0 * H * H;
    if (mode != MID_PLAIN) bytes += Pn * (n_prev + 2 + (e.y_aux ? 1 : 0));
    ProfScope prof(PROF_RHS_FUSED, st, bytes, 2.0 * A->nnz * H + 2.0 * (double)n_rows * H * H);
    const DropArgs dv = drop ? *drop : DropArgs{};
#define NDCN_MID(MODE_, DROP_, CDEV_)                                                                                          \
    do {                                                                                                                  \
        auto kern = rhs_mid_kernel<MODE_, DROP_, CDEV_>;                                                                  \
        static std::atomic<unsigned long long> attr_seen{0};                                                              \
        if (once_per_device(attr_seen))                                                                                   \
            NDCN_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mid_lds_bytes(kMidMaxH))); \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kMidThreads), lds, st, a, e, dv, c_dev);                                \
    } while (0)
    if (drop) {
        if (mode == MID_PLAIN) NDCN_MID(MID_PLAIN, true, false);
        else if (mode == MID_COMBINE) NDCN_MID(MID_COMBINE, true, false);
        else NDCN_MID(MID_RK4, true, false);
    } else if (c_dev) {                                      // a replayed adaptive step: coefficients from device memory (rhs_mid_epi.h)
        NDCN_MID(MID_COMBINE, false, true);
    } else if (mode == MID_PLAIN) NDCN_MID(MID_PLAIN, false, false);
    else if (mode == MID_COMBINE) NDCN_MID(MID_COMBINE, false, false);
    else NDCN_MID(MID_RK4, false, false);
#undef NDCN_MID
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

}  // namespace ndcn
