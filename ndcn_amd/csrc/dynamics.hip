// Ground-truth dynamics of the three drivers on an N x 1 state, edge-wise in O(nnz)  (SURVEY A11).
// The reference evaluates these with torch.sparse.mm / torch.mm on N x 1 (heat, gene) and, for the
// mutualistic model, by materialising a dense N x N interaction matrix (mutualistic_dynamics.py:206-216),
// which cannot exist at 10^6 nodes.  Here 8 lanes share a row, each lane walks every 8th stored edge,
// and the partial sums meet in a 3-step shuffle.
#include "kernels.h"

// Every rounding below is written out: products and sums round on their own, and where one fused multiply-add is meant it is an
// fmaf.  (Left to the compiler's contraction, the same expression came out fused in one kernel and unfused in its neighbour - the
// stand-alone kernels and the ones with the Runge-Kutta epilogue further down must agree bit for bit, and do so by construction.)
#pragma clang fp contract(off)

namespace ndcn {

constexpr int kLanesPerRow = 8;

__device__ __forceinline__ float ipow(float x, float p) {
    // torch's x ** 1 and x ** 2 are exact (x, x*x); anything else goes through powf
    if (p == 1.f) return x;
    if (p == 2.f) return x * x;
    return powf(x, p);
}

// edge(acc, a, xi, xj): the lane's partial sum after one more stored entry; finish(xi, acc): the row's result from the summed lanes
struct GeneOp {
    float b, f, h;
    __device__ __forceinline__ float edge(float acc, float a, float xi, float xj) const {
        const float p = ipow(xj, h);
        return fmaf(a, p / (p + 1.f), acc);                           // gene_dynamics.py:202
    }
    __device__ __forceinline__ float finish(float xi, float acc) const { return fmaf(-b, ipow(xi, f), acc); }
};

struct MutualOp {
    float b, k, c, d, e, h;
    __device__ __forceinline__ float edge(float acc, float a, float xi, float xj) const {
        return fmaf(a, xj * xi / (fmaf(e, xj, d) + h * xi), acc);     // mutualistic_dynamics.py:209-211 as executed
    }
    __device__ __forceinline__ float finish(float xi, float acc) const { return (b + xi * (1.f - xi / k) * (xi / c - 1.f)) + acc; }
};

template <class Op>
__global__ __launch_bounds__(256) void edge_dynamics_kernel(const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                                            const float *__restrict__ val, const float *__restrict__ x,
                                                            float *__restrict__ out, int n_rows, Op op) {
    const int rows_per_block = 256 / kLanesPerRow;
    const int li = threadIdx.x % kLanesPerRow;
    for (int r = blockIdx.x * rows_per_block + threadIdx.x / kLanesPerRow; r < n_rows; r += gridDim.x * rows_per_block) {
        const float xi = x[r];
        float acc = 0.f;
        for (int j = rowptr[r] + li; j < rowptr[r + 1]; j += kLanesPerRow) acc = op.edge(acc, val[j], xi, x[colidx[j]]);
#pragma unroll
        for (int off = kLanesPerRow / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, kLanesPerRow);
        if (li == 0) out[r] = op.finish(xi, acc);
    }
}

template <class Op>
static int launch_edge(const ndcn_csr *A, const float *x, float *out, Op op, hipStream_t st) {
    const int n = (int)A->n_rows;
    if (n == 0) return NDCN_OK;
    ProfScope prof(PROF_DYN, st, 8.0 * A->nnz + 4.0 * (n + 1) + 8.0 * n, 8.0 * A->nnz);
    const int rows_per_block = 256 / kLanesPerRow;
    int g = (n + rows_per_block - 1) / rows_per_block;
    if (g > kCus * 16) g = kCus * 16;
    hipLaunchKernelGGL((edge_dynamics_kernel<Op>), dim3(g), dim3(256), 0, st, A->rowptr, A->colidx, A->val, x, out, n, op);
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

int gene_rhs_f32(const ndcn_csr *A, const float *x, float *out, float b, float f, float h, hipStream_t st) {
    return launch_edge(A, x, out, GeneOp{b, f, h}, st);
}

int mutual_rhs_f32(const ndcn_csr *A, const float *x, float *out, float b, float k, float c, float d, float e, float h,
                   hipStream_t st) {
    return launch_edge(A, x, out, MutualOp{b, k, c, d, e, h}, st);
}

// ---------------------------------------------------------------------------------------------------
// The same right-hand sides with the Runge-Kutta algebra that consumes K in their epilogue: rhs_small_f32's contract at H = 1
// (modes PLAIN / COMBINE / ERROR / RK4, up to five earlier stages, coefficients by value or from device memory for a replayed
// step, RkOpt::y1 and y_aux / c_aux), so that the device solver runs the drivers' truth solves like any ODEFunc solve.
//   K        the bits of the stand-alone entry points: edge_dynamics_kernel's loop, shuffle and finish(xi, acc) for gene and
//            mutual (the same functions); for heat ndcn_spmm_f32 on an N x 1 panel - one lane per row, one fma per stored
//            entry in stored order from +0, then one multiply by alpha = -k
//   after K  the reference's operator order (rhs_small.hip): each product rounded on its own, the stages summed left to
//            right with the new one last; error terms squared and accumulated in double
// The lane that holds K owns the row's element of every row-local panel.
constexpr int kDynMaxPrev = 5;
constexpr int kDynMaxGrid = kCus * 16;        // as launch_edge
constexpr int kDynMaxGridError = 2048;        // ERROR: one {sum, bad} slot per workgroup; reduce_ws_bytes() holds at least 2048
enum { DYN_PLAIN = 0, DYN_COMBINE = 1, DYN_ERROR = 2, DYN_RK4 = 3 };

struct DynEpi {
    const float *y0;
    const float *kprev[kDynMaxPrev];
    float *y_next;
    double *partials;                 // ERROR: [gridDim.x][2]
    float c[kDynMaxPrev + 1];
    int n_prev;
    float rtol, atol;
    const float *c_dev;               // nullable: coefficients in device memory (hipGraph replay)
    const float *y1;                  // ERROR: the state of the error record
    float *y_aux;                     // COMBINE, nullable: second linear combination (no y0), coefficients c2[] (by value only)
    float c2[kDynMaxPrev + 1];
};

template <int MODE>
__device__ __forceinline__ void dyn_epilogue(const DynEpi &e, int idx, float kn, double &err_sum, double &err_bad) {
    const int np = e.n_prev;
    auto coef = [&](int m) { return e.c_dev ? e.c_dev[m] : e.c[m]; };
    const float y0 = e.y0[idx];
    float km[kDynMaxPrev];
#pragma unroll
    for (int m = 0; m < kDynMaxPrev; ++m) km[m] = m < np ? e.kprev[m][idx] : 0.f;
    if (MODE == DYN_RK4) {
        // rk4_alt_step_func (rk_common.py:72-78), same operator order as fixed_stage_kernel ops 2-5
        const float dt = coef(0);
        float sd;
        if (np == 0) sd = (kn * dt) / 3.f;
        else if (np == 1) sd = (km[0] / -3.f + kn) * dt;
        else if (np == 2) sd = ((km[0] - km[1]) + kn) * dt;
        else sd = (((km[0] + km[1] * 3.f) + km[2] * 3.f) + kn) * (dt / 8.f);
        e.y_next[idx] = y0 + sd;
        return;
    }
    // sum of the stages left to right, the new one last (misc.py:22-25), each product rounded on its own
    float sm = kn * coef(np);
    if (np > 0) {
        float uu = km[0] * coef(0);
#pragma unroll
        for (int m = 1; m < kDynMaxPrev; ++m)
            if (m < np) uu = uu + km[m] * coef(m);
        sm = uu + sm;
    }
    if (MODE == DYN_COMBINE) {
        e.y_next[idx] = y0 + sm;
        if (e.y_aux) {
            float w2 = kn * e.c2[np];
            if (np > 0) {
                float u2 = km[0] * e.c2[0];
#pragma unroll
                for (int m = 1; m < kDynMaxPrev; ++m)
                    if (m < np) u2 = u2 + km[m] * e.c2[m];
                w2 = u2 + w2;
            }
            e.y_aux[idx] = w2;
        }
    } else {
        const float y1 = e.y1[idx];
        const float tol = e.atol + e.rtol * max_nan(fabsf(y0), fabsf(y1));
        const float z = sm / tol;
        err_sum += (double)(z * z);
        err_bad += (double)(int)(!(fabsf(y1) <= 3.402823466e38f));
    }
}

// every thread's {sum, bad} -> the workgroup's slot of e.partials (fixed order: wave shuffle, then the four waves in order)
__device__ __forceinline__ void dyn_block_record(const DynEpi &e, double err_sum, double err_bad) {
    __shared__ double s_red[2 * (256 / kWave)];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        err_sum += __shfl_down(err_sum, off, kWave);
        err_bad += __shfl_down(err_bad, off, kWave);
    }
    if (lane == 0) { s_red[2 * wave] = err_sum; s_red[2 * wave + 1] = err_bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_red[0], b = s_red[1];
        for (int w = 1; w < 256 / kWave; ++w) { s += s_red[2 * w]; b += s_red[2 * w + 1]; }
        e.partials[2 * blockIdx.x] = s;
        e.partials[2 * blockIdx.x + 1] = b;
    }
}

template <class Op, int MODE>
__global__ __launch_bounds__(256) void edge_dynamics_rk_kernel(const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                                               const float *__restrict__ val, const float *__restrict__ x,
                                                               float *__restrict__ K, int n_rows, Op op, DynEpi e) {
    const int rows_per_block = 256 / kLanesPerRow;
    const int li = threadIdx.x % kLanesPerRow;
    double err_sum = 0.0, err_bad = 0.0;
    for (int r = blockIdx.x * rows_per_block + threadIdx.x / kLanesPerRow; r < n_rows; r += gridDim.x * rows_per_block) {
        const float xi = x[r];
        float acc = 0.f;
        for (int j = rowptr[r] + li; j < rowptr[r + 1]; j += kLanesPerRow) acc = op.edge(acc, val[j], xi, x[colidx[j]]);
#pragma unroll
        for (int off = kLanesPerRow / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, kLanesPerRow);
        if (li == 0) {
            const float kn = op.finish(xi, acc);
            K[r] = kn;
            if (MODE != DYN_PLAIN) dyn_epilogue<MODE>(e, r, kn, err_sum, err_bad);
        }
    }
    if (MODE == DYN_ERROR) dyn_block_record(e, err_sum, err_bad);
}

// heat: K = alpha (L x), the arithmetic of spmm_csr_kernel<1, 1> (spmm.hip row_gather: four entries requested ahead, consumed in
// stored order)
template <int MODE>
__global__ __launch_bounds__(256) void heat_rk_kernel(const int *__restrict__ rowptr, const int *__restrict__ colidx,
                                                      const float *__restrict__ val, const float *__restrict__ x,
                                                      float *__restrict__ K, int n_rows, float alpha, DynEpi e) {
    double err_sum = 0.0, err_bad = 0.0;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n_rows; r += gridDim.x * 256) {
        const int j1 = rowptr[r + 1];
        int j = rowptr[r];
        float acc = 0.f;
        for (; j + 4 <= j1; j += 4) {
            const float v0 = val[j], v1 = val[j + 1], v2 = val[j + 2], v3 = val[j + 3];
            const float x0 = x[colidx[j]], x1 = x[colidx[j + 1]], x2 = x[colidx[j + 2]], x3 = x[colidx[j + 3]];
            acc = fmaf(v0, x0, acc); acc = fmaf(v1, x1, acc); acc = fmaf(v2, x2, acc); acc = fmaf(v3, x3, acc);
        }
        for (; j < j1; ++j) acc = fmaf(val[j], x[colidx[j]], acc);
        const float kn = acc * alpha;
        K[r] = kn;
        if (MODE != DYN_PLAIN) dyn_epilogue<MODE>(e, r, kn, err_sum, err_bad);
    }
    if (MODE == DYN_ERROR) dyn_block_record(e, err_sum, err_bad);
}

template <class Op>
static void launch_edge_rk(int mode, int grid, hipStream_t st, const ndcn_csr *A, const float *x, float *K, Op op, const DynEpi &e) {
    const int n = (int)A->n_rows;
#define NDCN_DYN_EDGE(MODE_) \
    hipLaunchKernelGGL((edge_dynamics_rk_kernel<Op, MODE_>), dim3(grid), dim3(256), 0, st, A->rowptr, A->colidx, A->val, x, K, n, op, e)
    if (mode == DYN_PLAIN) NDCN_DYN_EDGE(DYN_PLAIN);
    else if (mode == DYN_COMBINE) NDCN_DYN_EDGE(DYN_COMBINE);
    else if (mode == DYN_ERROR) NDCN_DYN_EDGE(DYN_ERROR);
    else NDCN_DYN_EDGE(DYN_RK4);
#undef NDCN_DYN_EDGE
}

int dyn_rk_f32(int kind, const float *p, const ndcn_csr *A, const float *x, float *K, int mode, const float *y0,
               const float *const *h_kprev, const float *h_c, int n_prev, float *y_next, float rtol, float atol, double *d_out,
               void *d_ws, hipStream_t st, const float *c_dev, const RkOpt *opt) {
    if (kind != NDCN_DYN_HEAT && kind != NDCN_DYN_GENE && kind != NDCN_DYN_MUTUAL) { set_error("dyn_rk: unknown dynamics kind %d", kind); return NDCN_EINVAL; }
    if (mode < DYN_PLAIN || mode > DYN_RK4) { set_error("dyn_rk: unknown mode %d", mode); return NDCN_EINVAL; }
    if (n_prev < 0 || n_prev > kDynMaxPrev || (mode == DYN_RK4 && n_prev > 3)) { set_error("dyn_rk: bad stage count"); return NDCN_EINVAL; }
    if (opt && (opt->accum || opt->xadd || opt->xmask || opt->s_out || opt->no_k || opt->c_mid)) {
        set_error("dyn_rk: of the launch options only y1 and y_aux / c_aux are supported");
        return NDCN_EINVAL;
    }
    if (opt && opt->y_aux && (mode != DYN_COMBINE || !opt->c_aux || c_dev)) {
        set_error("dyn_rk: y_aux needs the COMBINE mode and c_aux, with the coefficients by value");
        return NDCN_EINVAL;
    }
    const int n = (int)A->n_rows;
    g_last_rhs_path = NDCN_PATH_DYN;
    if (n == 0) return NDCN_OK;
    DynEpi e = {};
    e.y0 = y0; e.y_next = y_next; e.n_prev = n_prev; e.rtol = rtol; e.atol = atol; e.partials = static_cast<double *>(d_ws);
    e.c_dev = mode != DYN_PLAIN ? c_dev : nullptr;
    e.y1 = (opt && opt->y1) ? opt->y1 : x;
    e.y_aux = (opt && opt->y_aux) ? opt->y_aux : nullptr;
    for (int m = 0; m <= kDynMaxPrev; ++m) e.c2[m] = (e.y_aux && m <= n_prev) ? opt->c_aux[m] : 0.f;
    for (int m = 0; m < kDynMaxPrev; ++m) e.kprev[m] = (m < n_prev && h_kprev) ? h_kprev[m] : nullptr;
    for (int m = 0; m <= kDynMaxPrev; ++m) e.c[m] = (mode != DYN_PLAIN && mode != DYN_RK4 && m <= n_prev && h_c) ? h_c[m] : 0.f;
    if (mode == DYN_RK4 && h_c) e.c[0] = h_c[0];
    double bytes = 8.0 * A->nnz + 4.0 * (n + 1) + 8.0 * n;
    if (mode != DYN_PLAIN) bytes += 4.0 * n * (n_prev + 2 + ((mode == DYN_ERROR && opt && opt->y1) ? 1 : 0) + (e.y_aux ? 1 : 0));
    ProfScope prof(PROF_DYN, st, bytes, (kind == NDCN_DYN_HEAT ? 2.0 : 8.0) * A->nnz);
    const int rows_per_block = kind == NDCN_DYN_HEAT ? 256 : 256 / kLanesPerRow;
    int grid = (n + rows_per_block - 1) / rows_per_block;
    const int max_grid = mode == DYN_ERROR ? kDynMaxGridError : kDynMaxGrid;
    if (grid > max_grid) grid = max_grid;
    if (kind == NDCN_DYN_HEAT) {
        const float alpha = -p[0];
#define NDCN_DYN_HEAT_LAUNCH(MODE_) \
    hipLaunchKernelGGL((heat_rk_kernel<MODE_>), dim3(grid), dim3(256), 0, st, A->rowptr, A->colidx, A->val, x, K, n, alpha, e)
        if (mode == DYN_PLAIN) NDCN_DYN_HEAT_LAUNCH(DYN_PLAIN);
        else if (mode == DYN_COMBINE) NDCN_DYN_HEAT_LAUNCH(DYN_COMBINE);
        else if (mode == DYN_ERROR) NDCN_DYN_HEAT_LAUNCH(DYN_ERROR);
        else NDCN_DYN_HEAT_LAUNCH(DYN_RK4);
#undef NDCN_DYN_HEAT_LAUNCH
    } else if (kind == NDCN_DYN_GENE) {
        launch_edge_rk(mode, grid, st, A, x, K, GeneOp{p[0], p[1], p[2]}, e);
    } else {
        launch_edge_rk(mode, grid, st, A, x, K, MutualOp{p[0], p[1], p[2], p[3], p[4], p[5]}, e);
    }
    NDCN_LAUNCH_CHECK();
    if (mode == DYN_ERROR) return partials_finish(e.partials, grid, d_out, st, 0);
    return NDCN_OK;
}

}  // namespace ndcn
