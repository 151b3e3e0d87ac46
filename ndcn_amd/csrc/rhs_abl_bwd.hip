// The reverse of ONE evaluation of the paper's two ablations (rhs_abl.hip is the forward) for hidden widths 16 <= H <= 128 (H a multiple
// of 4) at any number of rows, behind rhs_vjp_f32 (rhs_mid_bwd.hip) and so behind ndcn_rhs_vjp_f32, the dopri5 tape and the fixed-grid
// sweeps:
//   no_control   K = relu(A X):          gX = alpha A^T (g (.) [K > 0])
//                composed: relu_bwd_f32(g, K) -> tmpG, spmm_f32(At, tmpG) -> gX - two launches, a whole panel written and read again
//                only to carry a mask.
//                here: rhs_abl_vjp_graph_kernel, ONE launch - the mask rides in the transposed gather.
//   no_graph     K = relu(X W^T + b):    gZ = g (.) [K > 0],  gX = alpha gZ W,  gW (+)= s gZ^T X,  gb (+)= s colsum gZ
//                composed: linear_bwd_f32's three launches (gS GEMM, weight-gradient kernel, chunk sum) and a scale_f32 pass whenever
//                alpha does not ride in an SpMM.
//                here: rhs_mid_bwd_kernel with S = X (rhs_mid_bwd.hip: gS and the row-chunk partials of gW / gb in one launch, g, K
//                and X read once), gS stored straight into gX - times alpha exactly when the composed branch would run its scaling
//                pass (rhs_mid_bwd_scaled_kernel) -, then wgrad_chunk_sum: two launches.
//
// rhs_abl_vjp_graph_kernel: the lane layout of rhs_abl_graph_kernel - 64-row tiles in persistent workgroups of 512 threads, P / 4
// (rounded up to a power of two; P = ceil32(H)) lanes per row, each 4 columns wide; no LDS, no barrier.  For row r of At the lane walks
// the stored entries in stored order from +0, four entries' loads in flight; per entry 16 bytes of g and 16 bytes of K at row colidx[j],
// gz = (k <= 0 ? 0 : g) - relu_bwd_kernel's predicate, under which a NaN K passes - and ONE fmaf(val[j], gz, acc) per column: the chain
// of spmm_csr_kernel over the panel relu_bwd_kernel would have written (tests/_fma_chain.py).  acc *= alpha as vfinish of spmm.hip does,
// also when alpha is 1.  => gX holds the raw words of the two composed launches, signs of zero and NaN positions included: a masked NaN
// of g contributes val * 0, a passed one stays a NaN.  Dropout needs nothing new: the stored K' is the mask and s arrives as alpha.
//
// Which chain the composed SpMM runs: rhs_abl.hip's header.  rhs_abl_vjp_takes declines an At that carries a long-row plan for this
// width, as rhs_abl_takes does for A; csr_create_plans builds such plans for H = 256 alone, so none exists at these widths today.
//
// The switch (ndcn_set_rhs_abl_bwd / NDCN_RHS_ABL_BWD, off by default) is invisible in the gradients.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): rhs_abl_vjp_graph_kernel 60 VGPRs, 38 SGPRs, no
// LDS, 8 waves per SIMD; rhs_mid_bwd_scaled_kernel 153 VGPRs, 92 SGPRs (rhs_mid_bwd_kernel: 153 and 90), no static LDS, the dynamic
// (P + 128)(P + 1) 4 bytes of rhs_mid_bwd.hip; neither uses scratch.
//
// Measured slower than the composed launches (tools/micro/rhs_abl_bwd_time.py, one ndcn_rhs_vjp_f32 call at 99 856 rows, medians in us;
// DESIGN.md section 0.1): no_control at H = 96 and 128 - 51.0 against 44.7 (1.14 x) and 66.9 against 54.2 (1.23 x), the same with alpha = 2 -
// where the doubled gather (two row loads per stored entry) costs more than the panel write and re-read it saves.  Every other cell
// measured faster: no_control 0.73 - 0.96 x at H = 16 .. 64 and 0.57 x on the Pubmed topology at H = 16; no_graph 0.41 - 0.62 x at every
// width (0.74 - 0.78 x on Pubmed).  The switch has no bound yet: the step that turns it on by default can leave those two cells out.
#include <atomic>

#include "kernels.h"

#pragma clang fp contract(off)

namespace ndcn {

constexpr int kAbTile = 64;           // rows per tile (rhs_abl_graph_kernel's)
constexpr int kAbThreads = 512;
constexpr int kAbMinH = 16, kAbMaxH = 128;

struct AblVjpArgs {
    const int *rowptr, *colidx;       // At
    const float *val;
    const float *g, *K;
    float *gX;
    int n_rows, H;
    int lsh;                          // log2 of the lanes that gather one row
    float alpha;
};

__device__ __forceinline__ float4 ab_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float ab_mask(float g, float k) { return k <= 0.f ? 0.f : g; }        // relu_bwd_kernel: a NaN K passes
__device__ __forceinline__ void ab_mfma4(float4 &a, float v, const float4 &g, const float4 &k) {
    a.x = fmaf(v, ab_mask(g.x, k.x), a.x); a.y = fmaf(v, ab_mask(g.y, k.y), a.y);
    a.z = fmaf(v, ab_mask(g.z, k.z), a.z); a.w = fmaf(v, ab_mask(g.w, k.w), a.w);
}

// (8 waves per SIMD = four workgroups per CU, the grid below: uncapped the kernel takes 72 VGPRs and only three fit; capped 60, the
// eight 16-byte loads of a group of four entries still in flight together)
__global__ __launch_bounds__(kAbThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void rhs_abl_vjp_graph_kernel(AblVjpArgs a) {
    const int H = a.H, n = a.n_rows;
    // the workgroup's run of tiles: n_tiles split evenly, the first `rem` workgroups one more (rhs_abl_graph_kernel's split)
    const int n_tiles = (n + kAbTile - 1) / kAbTile;
    const int base = n_tiles / (int)gridDim.x, rem = n_tiles % (int)gridDim.x;
    const int b = blockIdx.x;
    const int t0 = b * base + (b < rem ? b : rem), t1 = t0 + base + (b < rem ? 1 : 0);
    const int tid = threadIdx.x, lsh = a.lsh;
    const int grp = tid >> lsh, c4 = (tid & ((1 << lsh) - 1)) * 4, rows_per_pass = kAbThreads >> lsh;
    if (c4 >= H) return;                                     // (no barrier anywhere below)
    const float *gc = a.g + c4, *kc = a.K + c4;
    const float alpha = a.alpha;
    for (int t = t0; t < t1; ++t) {
        const int r0 = t * kAbTile;
        for (int row = grp; row < kAbTile; row += rows_per_pass) {
            const int gr = r0 + row;
            if (gr >= n) break;
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            int j = a.rowptr[gr];
            const int j1 = a.rowptr[gr + 1];
            for (; j + 4 <= j1; j += 4) {
                const size_t q0 = (size_t)a.colidx[j] * H, q1 = (size_t)a.colidx[j + 1] * H;
                const size_t q2 = (size_t)a.colidx[j + 2] * H, q3 = (size_t)a.colidx[j + 3] * H;
                const float v0 = a.val[j], v1 = a.val[j + 1], v2 = a.val[j + 2], v3 = a.val[j + 3];
                const float4 g0 = ab_ld4(gc + q0), g1 = ab_ld4(gc + q1), g2 = ab_ld4(gc + q2), g3 = ab_ld4(gc + q3);
                const float4 k0 = ab_ld4(kc + q0), k1 = ab_ld4(kc + q1), k2 = ab_ld4(kc + q2), k3 = ab_ld4(kc + q3);
                ab_mfma4(s, v0, g0, k0); ab_mfma4(s, v1, g1, k1); ab_mfma4(s, v2, g2, k2); ab_mfma4(s, v3, g3, k3);
            }
            for (; j < j1; ++j) {
                const size_t q = (size_t)a.colidx[j] * H;
                ab_mfma4(s, a.val[j], ab_ld4(gc + q), ab_ld4(kc + q));
            }
            s.x *= alpha; s.y *= alpha; s.z *= alpha; s.w *= alpha;          // spmm.hip vfinish: also when alpha is 1
            *reinterpret_cast<float4 *>(a.gX + (size_t)gr * H + c4) = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- the switch
static std::atomic<int> g_ab_override{-1};                 // ndcn_set_rhs_abl_bwd: -1 = the environment's value

int rhs_abl_bwd_on() {
    const int ov = g_ab_override.load(std::memory_order_relaxed);
    if (ov >= 0) return ov;
    static const int env_on_ = env_int("NDCN_RHS_ABL_BWD", 0) > 0 ? 1 : 0;
    return env_on_;
}

int set_rhs_abl_bwd(int on) {
    const int prev = rhs_abl_bwd_on();
    g_ab_override.store(on < 0 ? -1 : (on ? 1 : 0), std::memory_order_relaxed);
    return prev;
}

// From the sizes alone: exactly one of the two ablation flags, H a multiple of 4 in 16..128, 1 <= n_rows < 2^31 - 64
int rhs_abl_bwd_supported(int64_t n_rows, int H, uint32_t flags) {
    const bool no_graph = flags & NDCN_F_NO_GRAPH, no_control = flags & NDCN_F_NO_CONTROL;
    if (no_graph == no_control) return 0;
    if (n_rows < 1 || n_rows >= ((int64_t)1 << 31) - kAbTile || H < kAbMinH || H > kAbMaxH || (H & 3)) return 0;
    return 1;
}

// ... and the transposed operator of a no_control call: square, and no long-row plan for this width (spmm_f32 would sum the hub rows
// by segments)
int rhs_abl_vjp_takes(const ndcn_csr *At, int64_t n_rows, int H) {
    if (At->n_rows != n_rows || At->n_cols != n_rows) return 0;
    if (At->hub_n > 0 && At->hub_H == H) return 0;
    return 1;
}

// gX = alpha At (g (.) [K > 0]) in one launch; the caller checked rhs_abl_bwd_supported, rhs_abl_vjp_takes and the 16-byte alignment
int rhs_abl_vjp_graph_f32(const ndcn_csr *At, const float *g, const float *K, float *gX, int H, float alpha, hipStream_t st) {
    AblVjpArgs a;
    a.rowptr = At->rowptr; a.colidx = At->colidx; a.val = At->val; a.g = g; a.K = K; a.gX = gX;
    a.n_rows = (int)At->n_rows; a.H = H; a.alpha = alpha;
    const int P = (H + 31) & ~31;
    a.lsh = P <= 32 ? 3 : (P <= 64 ? 4 : 5);
    const int n_tiles = (a.n_rows + kAbTile - 1) / kAbTile;
    const int grid = n_tiles < kCus * 4 ? n_tiles : kCus * 4;        // 2048 threads per CU
    const double Pn = 4.0 * H * (double)At->n_rows;
    ProfScope prof(PROF_SPMM, st, 8.0 * At->nnz + 4.0 * (At->n_rows + 1) + 3.0 * Pn, 2.0 * At->nnz * H);
    hipLaunchKernelGGL(rhs_abl_vjp_graph_kernel, dim3(grid), dim3(kAbThreads), 0, st, a);
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

}  // namespace ndcn
