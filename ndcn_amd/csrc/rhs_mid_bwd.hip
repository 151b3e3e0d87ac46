// The reverse of ONE evaluation K = relu(W (A X) + b) for the upstream gradient g (autograd_ops.rhs_vjp, tape.hip):
//   gZ = g (.) [K > 0],  gS = gZ W,  gW (+)= s gZ^T S,  gb (+)= s colsum gZ,  gX = s A^T gS,   S = A X
// rhs_vjp_f32 below is the one implementation every caller shares (the two native tapes, ndcn_rhs_vjp_f32).  Composed it is five launches:
// spmm_f32(A, X) -> S, linear_gs_kernel, linear_wgrad_kernel, chunk_sum2_kernel, spmm_f32(At, gS) - eight panel passes and two gathers.
//
// rhs_mid_bwd_kernel, for hidden widths 16 <= H <= 128 (H a multiple of 4) at ANY number of rows, forms gS and the row-chunk partials of
// gW / gb in ONE launch: three panel passes and one gather, S never leaves the CU and gZ is formed once.  Five launches become three.
//
//   workgroup = 8 waves = ONE row chunk of the weight gradient, exactly the chunks linear_bwd_f32 forms (wgrad_chunking), walked in
//   64-row tiles from the chunk's first row (tiles are not aligned to 64 globally; the last one is partial).  W (H x H fp32 <= 64 KiB)
//   is staged once into LDS, zero-padded to P = ceil32(H) in both dimensions.  Per tile:
//     S tile   the caller's S panel (the tape kept it) by 16-byte loads, or gathered: P / 4 (rounded up to a power of two) lanes per row,
//              ONE fma per stored entry in stored order from +0, four entries' loads in flight - the chain of spmm_csr_kernel and
//              rhs_mid.hip.  Columns beyond H and rows beyond the chunk are zero.
//     gZ tile  g masked by K with the predicate of linear_bwd.hip's masked() (zero where K <= 0, a NaN K passes), or g itself when the
//              caller masked it already; 16-byte loads
//     gS       wave w < 2 (P / 32) owns the 32 x 32 output tile (rows 32 (w & 1), columns 32 (w >> 1)): v_mfma_f32_32x32x2_f32 over
//              k = o = 0, 2, .. P - 2 from a zero accumulator - the operand mapping and chain of linear_gs_kernel, whose k chunks are
//              zero-padded to 32 in the same way - stored straight to global for rows of the chunk and columns below H
//     gW, gb   every (32-wide o-strip, 32-wide i-tile) pair has ONE accumulator that lives across all tiles of the chunk, advanced by one
//              v_mfma_f32_32x32x2_f32 per row pair, pairs ascending from the chunk's first row in whole rounds of 8 rows - the chain of
//              linear_wgrad_kernel (lane kk = lane >> 5 supplies row r + 2 u + kk; rows beyond the chunk are zero operands).  The up to
//              16 pairs are dealt over the 8 waves (pair p and p + 8 to wave p); no accumulator's rows are ever split.  gb: the per-lane
//              fp32 sum of the same A operands in the same order, then the __shfl_xor(.., 32) add.
//   After the last tile the partial block and bias row are written in linear_wgrad_kernel's layout; chunk_sum2_kernel / chunk_sum_kernel
//   (wgrad_chunk_sum) and the transposed SpMM follow as on the composed path.
//   => gS, gW, gb and gX hold the composed launches' raw words - signs of zero and NaN positions included, for every accumulate /
//   acc_scale combination: the switch (ndcn_set_rhs_mid_bwd / NDCN_RHS_MID_BWD, off by default) is invisible in the gradients.
//
// The kernel's body lives in rhs_mid_bwd_body.h and is included twice: rhs_mid_bwd_kernel as it always was, and rhs_mid_bwd_scaled_kernel,
// whose gS store multiplies by alpha - the no_graph ablation's reverse (rhs_abl_bwd.hip: S = X, gS straight into gX), taken at the top of
// rhs_vjp_f32 under ndcn_set_rhs_abl_bwd.
//
// LDS: (P + 64 + 64) (P + 1) 4 bytes - 20.6 KiB at P = 32, 48.8 KiB at 64, 84.0 KiB at 96, 129.0 KiB at 128 (one workgroup per CU).
#include <atomic>

#include "kernels.h"

#pragma clang fp contract(off)

namespace ndcn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMbTile = 64;           // rows per tile: two 32-row MFMA tiles of gS, 32 row pairs of gW
constexpr int kMbThreads = 512;
constexpr int kMbMinH = 16, kMbMaxH = 128;
// Mode 1 stops here: the largest measured width at which the fused reverse is not slower than the composed launches - and that is the
// widest one (tools/micro/rhs_mid_bwd_time.py, 99 856 rows, S re-formed: H = 16 0.067 ms against 0.127, 32 0.072 against 0.128, 64 0.102
// against 0.163, 96 0.171 against 0.237, 128 0.209 against 0.294; the single-wave gW chain at P = 32 does not make the narrow widths
// slower).  Mode 1 and mode 2 therefore take the same shapes today; the cap stays a constant for the measurement that moves it.
constexpr int kMbMode1MaxH = 128;

struct MidBwdArgs {
    const int *rowptr, *colidx;
    const float *val;
    const float *X;                   // the evaluation's input: gathered when S is null
    const float *S;                   // nullable: S = A X as the forward wrote it
    const float *g;
    const float *K;                   // nullable: no mask (g is gZ already, or no ReLU)
    const float *W;
    float *gS;                        // nullable: not wanted
    float *part_w, *part_b;           // part_b nullable
    int n_rows, H;
    int rpc;                          // rows per chunk (a multiple of 8)
    int lsh;                          // log2 of the lanes that gather one row
};

__device__ __forceinline__ float4 mb_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void mb_fma4(float4 &a, float v, const float4 &x) {
    a.x = fmaf(v, x.x, a.x); a.y = fmaf(v, x.y, a.y); a.z = fmaf(v, x.z, a.z); a.w = fmaf(v, x.w, a.w);
}
__device__ __forceinline__ float mb_mask(float g, float k) { return k <= 0.f ? 0.f : g; }       // linear_bwd.hip masked(): NaN passes

__global__ __launch_bounds__(kMbThreads) void rhs_mid_bwd_kernel(MidBwdArgs a) {
#define MB_GS_STORE(v) (v)
#include "rhs_mid_bwd_body.h"
#undef MB_GS_STORE
}

__global__ __launch_bounds__(kMbThreads) void rhs_mid_bwd_scaled_kernel(MidBwdArgs a, float alpha) {
#define MB_GS_STORE(v) (alpha * (v))
#include "rhs_mid_bwd_body.h"
#undef MB_GS_STORE
}

// ---------------------------------------------------------------------------------------------------- the switch
static std::atomic<int> g_mb_override{-1};                 // ndcn_set_rhs_mid_bwd: -1 = the environment's mode
static std::atomic<int> g_last_vjp_path{0};                // ndcn_debug_last_rhs_vjp_path: process-wide (a reverse pass runs on autograd's thread)
static int mb_clamp(int m) { return m < 0 ? 0 : (m > 2 ? 2 : m); }

int rhs_mid_bwd_mode() {
    const int ov = g_mb_override.load(std::memory_order_relaxed);
    if (ov >= 0) return ov;
    static const int env_mode = mb_clamp(env_int("NDCN_RHS_MID_BWD", 0));
    return env_mode;
}

int set_rhs_mid_bwd(int mode) {
    const int prev = rhs_mid_bwd_mode();
    g_mb_override.store(mode < 0 ? -1 : mb_clamp(mode), std::memory_order_relaxed);
    return prev;
}

int last_rhs_vjp_path() { return g_last_vjp_path.load(std::memory_order_relaxed); }

// From the sizes alone.  mode < 0: the switch's current mode.
int rhs_mid_bwd_supported(int64_t n_rows, int H, uint32_t flags, int mode) {
    if (mode < 0) mode = rhs_mid_bwd_mode();
    if (mode != 1 && mode != 2) return 0;
    if (n_rows < 1 || n_rows >= ((int64_t)1 << 31) - kMbTile || H < kMbMinH || H > kMbMaxH || (H & 3)) return 0;
    if (flags & (NDCN_F_NO_GRAPH | NDCN_F_NO_CONTROL)) return 0;
    if (mode == 1 && H > kMbMode1MaxH) return 0;
    return 1;
}

static size_t mb_lds_bytes(int H) {
    const size_t P = (size_t)((H + 31) & ~31);
    return (P + 2 * kMbTile) * (P + 1) * sizeof(float);
}

// gS (nullable) and the chunk partials of gW / gb into `work` (linear_bwd_work_bytes(n_rows, H, H) bytes), then their fixed-order sum.
// scale_gs: gS is stored as alpha * gS (the no_graph ablation, whose S is X: A is read for n_rows alone)
static int rhs_mid_bwd_f32(const ndcn_csr *A, const float *X, const float *S, const float *g, const float *mask, const float *W, float *gS,
                           float *gW, float *gb, void *work, int H, float acc_scale, bool accumulate, hipStream_t st,
                           bool scale_gs = false, float alpha = 1.f) {
    const int64_t n = A->n_rows;
    int64_t rpc, used;
    wgrad_chunking(n, H, H, &rpc, &used);
    MidBwdArgs a;
    a.rowptr = A->rowptr; a.colidx = A->colidx; a.val = A->val; a.X = X; a.S = S; a.g = g; a.K = mask; a.W = W; a.gS = gS;
    a.part_w = static_cast<float *>(work);
    a.part_b = gb ? a.part_w + (size_t)used * H * H : nullptr;
    a.n_rows = (int)n; a.H = H; a.rpc = (int)rpc;
    const int P = (H + 31) & ~31;
    a.lsh = P <= 32 ? 3 : (P <= 64 ? 4 : 5);
    const size_t lds = mb_lds_bytes(H);
    {
        const double Pn = 4.0 * H * (double)n;
        ProfScope prof(PROF_LINEAR_WGRAD, st, Pn * (2 + (mask ? 1 : 0) + (gS ? 1 : 0)) + (S ? 0.0 : 8.0 * A->nnz) + 4.0 * (used + 1) * (double)H * H,
                       (gS ? 4.0 : 2.0) * (double)n * H * H + (S ? 0.0 : 2.0 * A->nnz * H));
        static std::atomic<unsigned long long> attr_seen{0}, attr_seen_scaled{0};
        if (scale_gs) {
            if (once_per_device(attr_seen_scaled))
                NDCN_HIP(hipFuncSetAttribute((const void *)rhs_mid_bwd_scaled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)mb_lds_bytes(kMbMaxH)));
            hipLaunchKernelGGL(rhs_mid_bwd_scaled_kernel, dim3((unsigned)used), dim3(kMbThreads), lds, st, a, alpha);
        } else {
            if (once_per_device(attr_seen))
                NDCN_HIP(hipFuncSetAttribute((const void *)rhs_mid_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mb_lds_bytes(kMbMaxH)));
            hipLaunchKernelGGL(rhs_mid_bwd_kernel, dim3((unsigned)used), dim3(kMbThreads), lds, st, a);
        }
        NDCN_LAUNCH_CHECK();
    }
    return wgrad_chunk_sum(a.part_w, a.part_b, gW, gb, H, H, used, acc_scale, accumulate, st);
}

// ---------------------------------------------------------------------------------------------------- one evaluation's reverse
// gX (nullable: not wanted) = alpha J_X^T g; gW / gb (nullable under NO_CONTROL) = acc_scale * (this evaluation's), added to what they hold
// when `accumulate`.  K: the evaluation's output (the ReLU mask; with dropout the stored K' is the mask and s rides in the two scalars);
// premasked: g already is gZ.  S (nullable): A X as the forward wrote it; tmpS / tmpG: one panel each (S when it is re-formed; gS / gZ);
// bwork: linear_bwd_work_bytes(n_rows, H, H) bytes; packed (nullable): the caller's "planes of W^T are in bwork" state (H = 256).
// direct: without a graph and with alpha = 1 the result is written straight into gX (the dopri5 tape; the fixed-grid sweep always scales).
int rhs_vjp_f32(const ndcn_csr *A, const ndcn_csr *At, const float *X, const float *K, const float *g, const float *W,
                const float *S_kept, float *gx, float *gW, float *gb, float *tmpS, float *tmpG, void *bwork, int H, uint32_t flags,
                bool premasked, float acc_scale, float alpha, bool accumulate, bool direct, bool *packed, hipStream_t st) {
    const bool no_graph = flags & NDCN_F_NO_GRAPH, no_control = flags & NDCN_F_NO_CONTROL;
    const float *mask = ((flags & NDCN_F_RELU) && !premasked) ? K : nullptr;
    const bool rescale = no_graph && !(direct && alpha == 1.f);     // no SpMM to carry alpha: g_X = alpha * g_S by a pass from the scratch panel
    const int64_t n_rows = A->n_rows, n = n_rows * H;
    int rc;
    g_last_vjp_path.store(NDCN_VJP_COMPOSED, std::memory_order_relaxed);
    const float *gS = nullptr;
    // the ablations under their own switch (rhs_abl_bwd.hip): declined calls run the composed branches below
    if (no_graph != no_control && rhs_abl_bwd_on() && rhs_abl_bwd_supported(n_rows, H, flags) && A->n_cols == n_rows && aligned16(X) &&
        aligned16(g) && aligned16(K) && aligned16(W) && aligned16(gx) && !(gx && (gx == g || gx == K || gx == X))) {
        if (no_control) {
            // (without a mask the composed path is one launch already; without gx there is nothing to do)
            if (mask && gx && rhs_abl_vjp_takes(At, n_rows, H)) {
                rc = rhs_abl_vjp_graph_f32(At, g, mask, gx, H, alpha, st);
                if (rc) return rc;
                g_last_vjp_path.store(NDCN_VJP_ABL, std::memory_order_relaxed);
                return NDCN_OK;
            }
        } else if (gW && bwork) {
            // S = X; gS goes straight into gx, times alpha exactly when the composed branch would run its scale_f32 pass
            rc = rhs_mid_bwd_f32(A, X, X, g, mask, W, gx, gW, gb, bwork, H, acc_scale, accumulate, st, gx && rescale, alpha);
            if (rc) return rc;
            g_last_vjp_path.store(NDCN_VJP_ABL, std::memory_order_relaxed);
            return NDCN_OK;
        }
    }
    if (!no_control) {
        const int mode = rhs_mid_bwd_mode();
        if (mode != 0 && rhs_mid_bwd_supported(n_rows, H, flags, mode) && gW && bwork && A->n_cols == n_rows && aligned16(X) &&
            aligned16(g) && aligned16(mask) && aligned16(S_kept) && aligned16(W) && aligned16(tmpG)) {
            float *gs_out = gx ? tmpG : nullptr;
            rc = rhs_mid_bwd_f32(A, X, S_kept, g, mask, W, gs_out, gW, gb, bwork, H, acc_scale, accumulate, st);
            if (rc) return rc;
            g_last_vjp_path.store(NDCN_VJP_MID, std::memory_order_relaxed);
            if (!gx) return NDCN_OK;
            return spmm_f32(At, gs_out, nullptr, At->n_cols, gx, H, alpha, 0, st);
        }
        const float *S = X;
        if (!no_graph && S_kept) {
            S = S_kept;
        } else if (!no_graph) {
            rc = spmm_f32(A, X, nullptr, A->n_cols, tmpS, H, 1.f, 0, st);
            if (rc) return rc;
            S = tmpS;
        }
        float *gs_out = gx ? ((no_graph && !rescale) ? gx : tmpG) : nullptr;
        // g_W / g_b: this evaluation's + what the later evaluations sent (autograd_path._add_carried), in the launch that sums the chunks
        rc = linear_bwd_f32(g, mask, S, W, gs_out, gW, gb, bwork, n_rows, H, H, st, (packed && *packed) ? NDCN_F_PACKED : 0u, acc_scale,
                            accumulate);
        if (rc) return rc;
        if (packed && gs_out && H == 256) *packed = true;
        gS = gs_out;
    } else if (gx) {
        float *gs_out = (no_graph && !rescale) ? gx : tmpG;
        if (mask) {
            rc = relu_bwd_f32(gs_out, g, mask, n, st);
            if (rc) return rc;
            gS = gs_out;
        } else if (no_graph && !rescale) {
            rc = copy_f32(gx, g, n, st);
            if (rc) return rc;
            gS = gx;
        } else {
            gS = g;
        }
    }
    if (gx && !no_graph) return spmm_f32(At, gS, nullptr, At->n_cols, gx, H, alpha, 0, st);
    if (gx && rescale) return scale_f32(gx, gS, alpha, n, st);
    return NDCN_OK;
}

static int64_t mb_a256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// ndcn_rhs_vjp_f32's scratch: [S panel | gS panel | linear_bwd scratch], each 256-byte aligned
int64_t rhs_vjp_work_bytes(int64_t n_rows, int H, uint32_t flags) {
    if (n_rows < 0 || H <= 0) return 0;
    const int64_t panel = mb_a256(n_rows * (int64_t)H * (int64_t)sizeof(float));
    return 2 * panel + ((flags & NDCN_F_NO_CONTROL) ? 0 : mb_a256(linear_bwd_work_bytes(n_rows, H, H)));
}

int64_t rhs_vjp_gs_offset(int64_t n_rows, int H) { return mb_a256(n_rows * (int64_t)H * (int64_t)sizeof(float)); }

}  // namespace ndcn
