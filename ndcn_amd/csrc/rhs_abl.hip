// The paper's two ablations of ODEFunc (neural_dynamics.py:27-36) plus the Runge-Kutta algebra that consumes K, in ONE launch, for hidden
// widths 16 <= H <= 128 (H a multiple of 4) at any number of rows:
//   no_control   K = relu(A X)            otherwise spmm_f32 (row SpMM with the ReLU), then a stand-alone stage kernel reading K again
//   no_graph     K = relu(X W^T + b)      otherwise linear_f32 (MFMA Linear), then the same stage kernel
// and, under dropout, a third launch for the mask (rhs.hip: Rhs::Composed).  Here K is consumed where it is formed: a COMBINE launch with
// j earlier stages moves about (j + 4) panels plus the gather instead of (j + 5) - the byte model of rhs_mid.hip's header.  Both kernels
// work on 64-row tiles in persistent workgroups of 8 waves and end in the per-lane epilogue of rhs_mid.hip (rhs_mid_epi.h: 16 bytes per
// lane, dropout factor, the stage algebra of the STAND-ALONE kernels), so every panel they write - K, y_next, y_aux - equals the
// composed path's bit for bit, signs of zero and NaN positions included; the switch (ndcn_set_rhs_abl / NDCN_RHS_ABL, off by default)
// is invisible in the results.
//
//   no_control   P / 4 (rounded up to a power of two; P = ceil32(H)) lanes per row, each 4 columns wide: S[r, c] as ONE fma per stored
//                entry in stored order from +0 - the gather phase of rhs_mid_kernel, the chain of spmm_csr_kernel (tests/_fma_chain.py) -
//                four entries' loads in flight at a time.  No weight, no LDS, no barrier: the lane that gathered four columns runs
//                the ReLU and the epilogue on them in registers.
//   no_graph     W (H x H fp32) is staged into LDS once per workgroup, zero-padded to P in both dimensions; per tile the 64 rows of X
//                are loaded straight into the LDS tile that rhs_mid_kernel gathers into (columns beyond H and rows beyond n zero),
//                then wave w < 2 (P / 32) runs v_mfma_f32_32x32x2_f32 over k = 0, 2, .. P - 2 from a zero accumulator - the sequence
//                of linear_mfma_kernel, whose k chunks are zero-padded to 32 in the same way -, + b, the NaN-passing ReLU; the K tile
//                replaces the X tile in LDS and the epilogue reads it from there.
//
// Which chain the composed SpMM runs.  spmm_f32 leaves the plain stored-order chain for three plans: the column sweep (H = 256
// only), the group records (H = 256 only) and the long-row plan, whose hub rows are summed by segments - taken when the plan was built
// for this very width (ndcn_csr::hub_H == H).  csr_create_plans builds plans for H = 256 alone, so none of them exists at these
// widths; rhs_abl_takes still declines an operator that carries a long-row plan for H, which keeps the bits the composed path's
// whatever a later plan builder does.  (rhs_mid.hip runs its plain chain against the same spmm_f32 on the same grounds.)
//
// The error record is not formed here: an ERROR launch is this kernel in PLAIN mode followed by rk_error_f32 (rhs.hip), which keeps
// the record's summation order.  No halo panel, none of the RkOpt fields of the H = 256 launches: rhs.hip declines those.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, over each form's six instantiations): graph 42 - 46
// VGPRs, 42 - 94 SGPRs, no LDS; dense 46 - 64 VGPRs, 49 - 99 SGPRs, (P + 64)(P + 1) 4 bytes of LDS (99 072 at P = 128: one workgroup per
// CU); no instantiation uses scratch.
//
// Measured slower than the composed path (tools/micro/rhs_abl_time.py, 99 856 rows, medians in us): no_graph at
// H = 128 in every mode - plain 59.7 against 52.1, COMBINE 5 141.1 against 127.9, RK4 stage 3 131.9 against 107.8, and 1.03 - 1.07 x with
// p = 0.5 - the one-workgroup-per-CU width of rhs_mid.hip's kMidMode1MaxH; no_control in PLAIN mode without a mask, where the composed
// path is one launch too, at H = 64 / 96 / 128 (20.3 against 18.6, 31.7 against 24.0, 36.1 against 26.3).  Every other (form, width,
// mode) at H <= 96, and every launch with an epilogue or a mask of no_control, measured 0.60 - 0.99 x.  The switch has no mode-1 bound
// yet: the step that turns it on by default can leave those cells out.
#include <atomic>

#include "kernels.h"
#include "rhs_mid_epi.h"

#pragma clang fp contract(off)

namespace ndcn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct AblArgs {
    const int *rowptr, *colidx;       // no_control
    const float *val;
    const float *X;
    const float *W, *bias;            // no_graph
    float *K;
    int n_rows, H, relu;
    int lsh;                          // no_control: log2 of the lanes that gather one row
};

// the workgroup's run of tiles: n_tiles split evenly, the first `rem` workgroups one more (rhs_mid_kernel's split)
__device__ __forceinline__ void abl_tiles(int n, int &t0, int &t1) {
    const int n_tiles = (n + kMidTile - 1) / kMidTile;
    const int base = n_tiles / (int)gridDim.x, rem = n_tiles % (int)gridDim.x;
    const int b = blockIdx.x;
    t0 = b * base + (b < rem ? b : rem);
    t1 = t0 + base + (b < rem ? 1 : 0);
}

template <int MODE, bool DROP, bool CDEV = false>
__global__ __launch_bounds__(kMidThreads) void rhs_abl_graph_kernel(AblArgs a, MidEpi e, DropArgs d, const float *c_dev) {
    const int H = a.H, n = a.n_rows;
    int t0, t1;
    abl_tiles(n, t0, t1);
    const int tid = threadIdx.x, lsh = a.lsh;
    const int g = tid >> lsh, c4 = (tid & ((1 << lsh) - 1)) * 4, rows_per_pass = kMidThreads >> lsh;
    if (c4 >= H) return;                                     // (no barrier anywhere below)
    MidCoef kc = {};
    if (CDEV) kc = mid_coef_dev(c_dev, e.n_prev);
    const float *xc = a.X + c4;
    for (int t = t0; t < t1; ++t) {
        const int r0 = t * kMidTile;
        for (int row = g; row < kMidTile; row += rows_per_pass) {
            const int gr = r0 + row;
            if (gr >= n) break;
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            int j = a.rowptr[gr];
            const int j1 = a.rowptr[gr + 1];
            for (; j + 4 <= j1; j += 4) {
                const int q0 = a.colidx[j], q1 = a.colidx[j + 1], q2 = a.colidx[j + 2], q3 = a.colidx[j + 3];
                const float v0 = a.val[j], v1 = a.val[j + 1], v2 = a.val[j + 2], v3 = a.val[j + 3];
                const float4 x0 = mid_ld4(xc + (size_t)q0 * H), x1 = mid_ld4(xc + (size_t)q1 * H);
                const float4 x2 = mid_ld4(xc + (size_t)q2 * H), x3 = mid_ld4(xc + (size_t)q3 * H);
                mid_fma4(s, v0, x0); mid_fma4(s, v1, x1); mid_fma4(s, v2, x2); mid_fma4(s, v3, x3);
            }
            for (; j < j1; ++j) mid_fma4(s, a.val[j], mid_ld4(xc + (size_t)a.colidx[j] * H));
            if (a.relu) { s.x = relu_nan(s.x); s.y = relu_nan(s.y); s.z = relu_nan(s.z); s.w = relu_nan(s.w); }
            mid_epi_lane<MODE, DROP, CDEV>(s, (size_t)gr * H + c4, a.K, e, d, kc);
        }
    }
}

template <int MODE, bool DROP, bool CDEV = false>
__global__ __launch_bounds__(kMidThreads) void rhs_abl_dense_kernel(AblArgs a, MidEpi e, DropArgs d, const float *c_dev) {
    extern __shared__ __align__(16) float abl_lds[];
    const int H = a.H, n = a.n_rows;
    const int P = (H + 31) & ~31;                            // H padded to the MFMA tile: k steps and output columns
    const int ld = P + 1;                                    // odd leading dimension: the column-ish operand reads are conflict-free
    const int H4 = H >> 2, P4 = P >> 2;
    float *s_W = abl_lds;                                    // [P][ld]  s_W[o * ld + k] = W[o][k], zero beyond H
    float *s_T = abl_lds + P * ld;                           // [64][ld] the X tile; then [64][P] the K tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < P * P; i += kMidThreads) {
        const int o = i / P, k = i - o * P;
        s_W[o * ld + k] = (o < H && k < H) ? a.W[o * H + k] : 0.f;
    }
    int t0, t1;
    abl_tiles(n, t0, t1);
    const int n_jobs = 2 * (P >> 5);
    const int wm = wave & 1, tn = wave >> 1;
    const int on = tn * 32 + (lane & 31);
    const float bv = (wave < n_jobs && a.bias && on < H) ? a.bias[on] : 0.f;
    MidCoef kc = {};
    if (CDEV) kc = mid_coef_dev(c_dev, e.n_prev);
    for (int t = t0; t < t1; ++t) {
        const int r0 = t * kMidTile;
        // ---- the X tile, 16 bytes per lane
        for (int i = tid; i < kMidTile * P4; i += kMidThreads) {
            const int row = i / P4, q = i - row * P4;
            const int gr = r0 + row;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gr < n && q < H4) v = mid_ld4(a.X + (size_t)gr * H + 4 * q);
            float *dst = s_T + row * ld + 4 * q;
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        }
        __syncthreads();                                     // (the first tile: s_W too)
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
        __syncthreads();                                     // every wave has read its X rows: the K tile takes their place
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
            mid_epi_lane<MODE, DROP, CDEV>(mid_ld4(s_T + row * P + 4 * q), (size_t)gr * H + 4 * q, a.K, e, d, kc);
        }
        __syncthreads();                                     // the next tile's load overwrites the K tile
    }
}

// ---------------------------------------------------------------------------------------------------- the switch
static std::atomic<int> g_abl_override{-1};                // ndcn_set_rhs_abl: -1 = the environment's value

int rhs_abl_on() {
    const int ov = g_abl_override.load(std::memory_order_relaxed);
    if (ov >= 0) return ov;
    static const int env_on_ = env_int("NDCN_RHS_ABL", 0) > 0 ? 1 : 0;
    return env_on_;
}

int set_rhs_abl(int on) {
    const int prev = rhs_abl_on();
    g_abl_override.store(on < 0 ? -1 : (on ? 1 : 0), std::memory_order_relaxed);
    return prev;
}

// From the sizes alone: exactly one of the two ablation flags, H a multiple of 4 in 16..128, at least one row
int rhs_abl_supported(int64_t n_rows, int H, uint32_t flags) {
    const bool no_graph = flags & NDCN_F_NO_GRAPH, no_control = flags & NDCN_F_NO_CONTROL;
    if (no_graph == no_control) return 0;
    if (n_rows < 1 || n_rows >= ((int64_t)1 << 31) - kMidTile || H < kMidMinH || H > kMidMaxH || (H & 3)) return 0;
    return 1;
}

// ... and the operator: a long-row plan built for this width would make spmm_f32 sum the hub rows by segments (header)
int rhs_abl_takes(const ndcn_csr *A, int H, uint32_t flags) {
    if (!rhs_abl_supported(A->n_rows, H, flags)) return 0;
    if (!(flags & NDCN_F_NO_GRAPH) && A->hub_n > 0 && A->hub_H == H) return 0;
    return 1;
}

static size_t abl_lds_bytes(int H) {
    const size_t P = (size_t)((H + 31) & ~31);
    return (P + kMidTile) * (P + 1) * sizeof(float);
}

int rhs_abl_f32(const ndcn_csr *A, const float *X, const float *W, const float *b, float *K, int H, uint32_t flags, int mode,
                const float *y0, const float *const *h_kprev, const float *h_c, int n_prev, float *y_next, hipStream_t st,
                const RkOpt *opt, const DropArgs *drop, const float *c_dev) {
    const int n_rows = (int)A->n_rows;
    if (!rhs_abl_takes(A, H, flags)) { set_error("rhs_abl: one of no_graph / no_control, H a multiple of 4 in 16..128"); return NDCN_EINVAL; }
    if (mode != MID_PLAIN && mode != MID_COMBINE && mode != MID_RK4) { set_error("rhs_abl: bad mode"); return NDCN_EINVAL; }
    if (n_prev < 0 || n_prev > kMidMaxPrev || (mode == MID_RK4 && n_prev > 3)) { set_error("rhs_abl: bad stage count"); return NDCN_EINVAL; }
    if (drop && !(flags & NDCN_F_RELU)) { set_error("rhs_abl: dropout without the ReLU"); return NDCN_EINVAL; }
    if (c_dev && (mode != MID_COMBINE || drop || (opt && opt->y_aux))) { set_error("rhs_abl: c_dev goes with COMBINE, without dropout or y_aux"); return NDCN_EINVAL; }
    const bool dense = flags & NDCN_F_NO_GRAPH;
    AblArgs a = {};
    a.X = X; a.K = K; a.n_rows = n_rows; a.H = H; a.relu = (flags & NDCN_F_RELU) ? 1 : 0;
    const int P = (H + 31) & ~31;
    if (dense) { a.W = W; a.bias = b; }
    else { a.rowptr = A->rowptr; a.colidx = A->colidx; a.val = A->val; a.lsh = P <= 32 ? 3 : (P <= 64 ? 4 : 5); }
    MidEpi e = {};
    if (mode != MID_PLAIN) mid_epi_fill(e, mode, y0, h_kprev, h_c, n_prev, y_next, opt ? opt->y_aux : nullptr, opt ? opt->c_aux : nullptr);
    const size_t lds = dense ? abl_lds_bytes(H) : 0;
    int per_cu = dense ? (int)(kLdsPerCu / lds) : 4;       // no_graph, H = 128: 1, H = 64: 4
    if (per_cu > 4) per_cu = 4;                            // 2048 threads per CU
    const int n_tiles = (n_rows + kMidTile - 1) / kMidTile;
    const int grid = n_tiles < kCus * per_cu ? n_tiles : kCus * per_cu;
    const double Pn = 4.0 * H * (double)n_rows;
    double bytes = dense ? 2.0 * Pn + 4.0 * H * H : 8.0 * A->nnz + 4.0 * (n_rows + 1) + 4.0 * H * (double)(A->n_rows + A->n_cols);
    if (mode != MID_PLAIN) bytes += Pn * (n_prev + 2 + (e.y_aux ? 1 : 0));
    ProfScope prof(PROF_RHS_FUSED, st, bytes, dense ? 2.0 * (double)n_rows * H * H : 2.0 * A->nnz * H);
    const DropArgs dv = drop ? *drop : DropArgs{};
#define NDCN_ABL(MODE_, DROP_, CDEV_)                                                                                          \
    do {                                                                                                                  \
        if (dense) {                                                                                                      \
            auto kern = rhs_abl_dense_kernel<MODE_, DROP_, CDEV_>;                                                        \
            static std::atomic<unsigned long long> attr_seen{0};                                                          \
            if (once_per_device(attr_seen))                                                                               \
                NDCN_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)abl_lds_bytes(kMidMaxH))); \
            hipLaunchKernelGGL(kern, dim3(grid), dim3(kMidThreads), lds, st, a, e, dv, c_dev);                            \
        } else {                                                                                                          \
            hipLaunchKernelGGL((rhs_abl_graph_kernel<MODE_, DROP_, CDEV_>), dim3(grid), dim3(kMidThreads), 0, st, a, e, dv, c_dev); \
        }                                                                                                                 \
    } while (0)
    if (drop) {
        if (mode == MID_PLAIN) NDCN_ABL(MID_PLAIN, true, false);
        else if (mode == MID_COMBINE) NDCN_ABL(MID_COMBINE, true, false);
        else NDCN_ABL(MID_RK4, true, false);
    } else if (c_dev) {                                      // a replayed adaptive step: coefficients from device memory (rhs_mid_epi.h)
        NDCN_ABL(MID_COMBINE, false, true);
    } else if (mode == MID_PLAIN) NDCN_ABL(MID_PLAIN, false, false);
    else if (mode == MID_COMBINE) NDCN_ABL(MID_COMBINE, false, false);
    else NDCN_ABL(MID_RK4, false, false);
#undef NDCN_ABL
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

}  // namespace ndcn
