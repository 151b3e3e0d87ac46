// ODEFunc.forward as one entry point: Y = relu(W (A X) + b)   (neural_dynamics.py:20-39), with or without the stage algebra of an RK
// step behind it and with or without the dropout factor of csrc/dropout.h on it.  One dispatch serves every caller that is not the device
// solver's own launch kind: pick() decides which launch forms K (the table on enum class Rhs), rhs_rk_f32 switches on it.  The mask is
// an optional argument all the way down: in the epilogue of the narrow-panel launch and, under its own switch, of the rhs_mid.hip
// launch; a streaming pass behind every other route.
#include <stdio.h>

#include <atomic>

#include "kernels.h"
#include "split16.h"

namespace ndcn {

int rhs_fused_supported(int H, uint32_t flags);
int64_t rhs_fused_work_bytes(int H);
int rhs_fused_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, const float *W, const float *b,
                  float *Y, float *work, int H, uint32_t flags, hipStream_t st);
int rhs_fused_packed_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, const float *Wp, const float *b, float *Y,
                         uint32_t flags, hipStream_t st);

__global__ __launch_bounds__(256) void relu_copy_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t n,
                                                        int relu) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = x[i];
        y[i] = relu ? relu_nan(v) : v;
    }
}

// y = relu(y) in place, 16 bytes per lane (n4 float4 items; the panels of the H = 256 kernels are 16-byte aligned multiples of 4)
__global__ __launch_bounds__(256) void relu_inplace4_kernel(float4 *y, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 v = y[i];
    v.x = relu_nan(v.x); v.y = relu_nan(v.y); v.z = relu_nan(v.z); v.w = relu_nan(v.w);
    y[i] = v;
}

int64_t rhs_work_bytes(int64_t n_rows, int H, uint32_t flags) {
    const bool graph = !(flags & NDCN_F_NO_GRAPH), ctl = !(flags & NDCN_F_NO_CONTROL);
    if (!(graph && ctl)) return 0;
    if (rhs_fused_supported(H, flags)) return rhs_fused_work_bytes(H);       // packed weights
    if (rhs_small_wanted(n_rows, H, flags)) return 16;                          // rhs_small.hip needs none (a token size keeps callers' pointers non-null)
    return n_rows * (int64_t)H * (int64_t)sizeof(float);                        // S = A X between the two kernels
}

// Which launch forms K for one call of rhs_rk_f32 (mode 0: rhs_f32), decided once by pick() - the first row that holds, top to bottom:
//   kind      rides in the launch    chosen when                                                              the launch
//   Fused     stage algebra          no mask, mode != 0, graph and control, rhs_fused2_supported (H = 256),   rhs_fused2_f32 / rhs_fused2_exact_f32
//                                    rhs_fused2_variant
//   Mid       stage algebra, mask    `mid` (below), and mode 0, or COMBINE / RK4 with y0, y_next, y_aux and   rhs_mid_f32
//                                    every kprev 16-byte aligned
//   Small     stage algebra, mask    small_takes - unless `mid` holds in ERROR mode (MidPlain keeps it)       rhs_small_f32
//   Abl       stage algebra, mask    `abl` (below), and mode 0, or COMBINE / RK4 with the stage panels aligned  rhs_abl_f32
//             mask                   `abl` - ERROR mode, or a misaligned stage panel - unless mask_combines   rhs_abl_f32 in mode 0, then rk_stage_f32
//   Rec       stage algebra          no mask, mode != 0, no_control, aligned panels, spmm_rec_supported,      spmm_rec_f32
//                                    spmm_rec_variant, rows * 1 KiB < 4 GiB
//   Wide      stage algebra          no mask, mode != 0, no_control, aligned panels, spmm_wide_rk_supported,  spmm_wide_rk_f32
//                                    not a shape of the column sweep (rhs_plain runs it)
//   MidPlain  mask                   `mid` - ERROR mode, or a misaligned stage panel that Small left here -   rhs_mid_f32 in mode 0, then rk_stage_f32
//                                    unless mask_combines
//   Composed  nothing                everything else                                                          rhs_plain, then the mask pass and
//                                                                                                             rk_stage_f32, or (mask_combines)
//                                                                                                             dropout_combine_f32 for both
//   mid: ndcn_set_rhs_mid takes the shape (rhs_mid_supported: graph and control, 16 <= H <= 128 in fours) - with a mask only under
//   ndcn_set_rhs_mid_drop too -, no halo panel, X, W and K 16-byte aligned, none of the RkOpt fields of mid_declines.
//   abl: ndcn_set_rhs_abl is on and rhs_abl_takes the shape (exactly one of no_graph / no_control, 16 <= H <= 128 in fours, no long-row
//   plan for this width), no halo panel, X and K - no_graph: and W - 16-byte aligned, none of the RkOpt fields of mid_declines.
// Mode 0 reads neither stage arguments nor RkOpt, so only Mid, Small, Abl and Composed occur there.  H = 256 under a mask is always Composed.
enum class Rhs { Fused, Mid, Small, Abl, Rec, Wide, MidPlain, Composed };

// the RkOpt fields that exist only inside the H = 256 launches (s_out: and the narrow-panel one); none of them has a dropout form
static bool fused_only(const RkOpt *o) { return o && (o->xadd || o->xmask || o->s_out || o->c_mid); }
// ... and the ones rhs_mid.hip declines
static bool mid_declines(const RkOpt *o) { return fused_only(o) || (o && o->no_k); }

// rhs_small.hip takes the shape.  rhs_small_supported implies graph and control and H <= 128, hence never a shape of the H = 256 kernels
static bool small_takes(const ndcn_csr *A, int H, uint32_t flags) { return rhs_small_supported(A, H, flags) != 0; }

// under a mask, COMBINE without y_aux behind a launch that carries neither: dropout_combine_f32 masks K and forms the sum in ONE pass
// (one launch and one panel read fewer than the mask pass and rk_combine_f32; the same bits)
static bool mask_combines(int mode, const RkOpt *opt) { return mode == NDCN_RK_COMBINE && !(opt && opt->y_aux); }

// COMBINE / RK4: every panel the epilogue of rhs_mid.hip / rhs_abl.hip reads or writes by 16 bytes is aligned (mode 0: none)
static bool stage_aligned(int mode, const float *y0, const float *const *h_kprev, int n_prev, const float *y_next, const RkOpt *opt) {
    if (mode == 0) return true;
    bool epi = aligned16(y0) && aligned16(y_next) && !(opt && opt->y_aux && !aligned16(opt->y_aux));
    for (int m = 0; m < n_prev; ++m) epi = epi && h_kprev && aligned16(h_kprev[m]);
    return epi;
}

// the stage algebra rides in the rhs_abl.hip launch (otherwise that launch runs in mode 0 with rk_stage_f32 behind it)
static bool abl_epilogue(int mode, const float *y0, const float *const *h_kprev, int n_prev, const float *y_next, const RkOpt *opt) {
    return mode != NDCN_RK_ERROR && stage_aligned(mode, y0, h_kprev, n_prev, y_next, opt);
}

static Rhs pick(const ndcn_csr *A, const float *X, const float *Xh, const float *W, const float *K, int H, uint32_t flags, int mode,
                const float *y0, const float *const *h_kprev, int n_prev, const float *y_next, const RkOpt *opt, bool masked) {
    const bool graph_only = !(flags & NDCN_F_NO_GRAPH) && (flags & NDCN_F_NO_CONTROL);
    const bool bare_stage = !masked && mode != 0;       // the H = 256 and the graph-only launches carry the stage algebra only, and no mask
    if (bare_stage && rhs_fused2_supported(A, H, flags) && rhs_fused2_variant(mode, n_prev)) return Rhs::Fused;
    const int mid_mode = rhs_mid_mode();
    const bool mid = mid_mode != 0 && (!masked || rhs_mid_drop_on()) && !Xh && !mid_declines(opt) &&
                     rhs_mid_supported(A->n_rows, H, flags, mid_mode) && aligned16(X) && aligned16(W) && aligned16(K);
    // ERROR: its plain launch and rk_error_f32, which keeps the record's summation
    if (mid && mode != NDCN_RK_ERROR && stage_aligned(mode, y0, h_kprev, n_prev, y_next, opt)) return Rhs::Mid;
    if (!(mid && mode == NDCN_RK_ERROR) && small_takes(A, H, flags)) return Rhs::Small;
    if (rhs_abl_on() && !Xh && !mid_declines(opt) && rhs_abl_takes(A, H, flags) && aligned16(X) && aligned16(K) &&
        (!(flags & NDCN_F_NO_GRAPH) || aligned16(W)) &&
        (abl_epilogue(mode, y0, h_kprev, n_prev, y_next, opt) || !(masked && mask_combines(mode, opt))))
        return Rhs::Abl;
    if (bare_stage && graph_only && aligned16(X) && aligned16(K) && (!Xh || aligned16(Xh))) {
        // relu(A X) with the stage algebra in the epilogue of the group-record SpMM (spmm_rec.hip), or of the wide one on any other graph
        if (spmm_rec_supported(A, H) && spmm_rec_variant(mode, n_prev) && A->n_rows * (int64_t)1024 < (1ll << 32)) return Rhs::Rec;
        const bool swept = !Xh && H == 256 && spmm_sweep_supported(A, H);
        if (!swept && spmm_wide_rk_supported(A, H)) return Rhs::Wide;
    }
    if (mid && !(masked && mask_combines(mode, opt))) return Rhs::MidPlain;
    return Rhs::Composed;
}

// RkOpt::s_out can be honoured: the lattice-plan kernel (rhs_adj_supported), or the narrow-panel one
int rhs_s_out_supported(const ndcn_csr *A, int H, uint32_t flags, int mode, int n_prev) {
    return rhs_adj_supported(A, H, flags, mode, n_prev) || small_takes(A, H, flags);
}

// K by the launches that carry neither stage algebra nor mask (Rhs::Composed)
static int rhs_plain(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, const float *W, const float *b, float *Y,
                     float *work, int H, uint32_t flags, hipStream_t st) {
    const bool graph = !(flags & NDCN_F_NO_GRAPH), ctl = !(flags & NDCN_F_NO_CONTROL);
    const uint32_t act = flags & NDCN_F_RELU;
    const int64_t n = A->n_rows;
    if (graph && ctl) {
        if (rhs_fused_supported(H, flags)) {
            if (rhs_fused2_supported(A, H, flags)) {          // operator carries a row-group union plan
                if (!(aligned16(X) && aligned16(Y) && aligned16(W) && aligned16(work) && (!Xh || aligned16(Xh)))) {
                    set_error("rhs: panels must be 16-byte aligned");
                    return NDCN_EINVAL;
                }
                int rc = (flags & NDCN_F_PACKED) ? NDCN_OK : pack_weight_256(W, work, st);
                if (rc) return rc;
                if (weights_wide_range(work))
                    // range guard (split16.h): weights outside the split product's guarantee take the fp32 matrix cores - the same
                    // kernel with the v_mfma_f32_32x32x2_f32 consumer over the fp32 image of W in the same scratch (rhs_fused2_exact.hip)
                    return rhs_fused2_exact_f32(A, X, Xh, n_own, work, b, Y, flags, 0, nullptr, nullptr, nullptr, 0, nullptr, 0.f, 0.f,
                                                nullptr, nullptr, st);
                return rhs_fused2_f32(A, X, Xh, n_own, work, b, Y, flags, 0, nullptr, nullptr, nullptr, 0, nullptr, 0.f,
                                      0.f, nullptr, nullptr, st);
            }
            return rhs_fused_f32(A, X, Xh, n_own, W, b, Y, work, H, flags, st);
        }
        g_last_rhs_path &= ~NDCN_PATH_MID;                                     // (the report of a plain p = 0 call: rhs_rk_f32)
        int rc = spmm_f32(A, X, Xh, n_own, work, H, 1.f, 0, st);
        if (rc) return rc;
        return linear_f32(work, W, b, Y, n, H, H, act, st);
    }
    if (graph) {                                                                // no_control: relu(A x)
        // operators with a column-sweep plan: S = A X by the sweep straight into Y, the ReLU as a streaming pass in place
        if (act && !Xh && H == 256 && spmm_sweep_supported(A, H) && aligned16(X) && aligned16(Y)) {
            int rc = spmm_sweep_f32(A, X, Y, st);
            if (rc) return rc;
            const int64_t total = n * (int64_t)H;
            hipLaunchKernelGGL(relu_inplace4_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, st, reinterpret_cast<float4 *>(Y), total / 4);
            NDCN_LAUNCH_CHECK();
            return NDCN_OK;
        }
        return spmm_f32(A, X, Xh, n_own, Y, H, 1.f, act, st);
    }
    if (ctl) return linear_f32(X, W, b, Y, n, H, H, act, st);                   // no_graph: relu(W x + b)
    const int64_t total = n * (int64_t)H;                                       // neither: relu(x)
    if (total == 0) return NDCN_OK;
    hipLaunchKernelGGL(relu_copy_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, st, X, Y, total, act ? 1 : 0);
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

int rhs_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, const float *W, const float *b, float *Y,
            float *work, int H, uint32_t flags, hipStream_t st, const DropArgs *drop) {
    return rhs_rk_f32(A, X, Xh, n_own, W, b, Y, work, H, flags, 0, nullptr, nullptr, nullptr, 0, nullptr, 0.f, 0.f, nullptr, nullptr, st,
                      nullptr, drop);
}

// the stage algebra over {kprev..., K} by the un-fused kernels, in the term order of the fused epilogues (K is the last term)
static int rk_stage_f32(int64_t n, const float *X, const float *K, int rk_mode, const float *y0, const float *const *h_kprev, const float *h_c,
                        int n_prev, float *y_next, float rtol, float atol, double *d_out, void *d_ws, hipStream_t st, const RkOpt *opt) {
    const float *kk[6];
    for (int m = 0; m < n_prev; ++m) kk[m] = h_kprev[m];
    kk[n_prev] = K;
    if (rk_mode == 3)
        return fixed_stage_f32(2 + n_prev, y_next, y0, kk[0], n_prev > 0 ? kk[1] : nullptr, n_prev > 1 ? kk[2] : nullptr,
                               n_prev > 2 ? kk[3] : nullptr, h_c[0], n, st, nullptr);
    if (rk_mode == 1) {
        int rc = rk_combine_f32(y_next, y0, kk, h_c, n_prev + 1, n, st);
        if (!rc && opt && opt->y_aux && opt->c_aux) rc = rk_combine_f32(opt->y_aux, nullptr, kk, opt->c_aux, n_prev + 1, n, st);
        return rc;
    }
    return rk_error_f32(y0, (opt && opt->y1) ? opt->y1 : X, kk, h_c, n_prev + 1, rtol, atol, n, d_out, d_ws, st, nullptr,
                        (opt && opt->accum) ? 1 : 0);
}

// drop (nullable): K' = relu(z) * m (csrc/dropout.h), K as stored and as the stage algebra consumes it.  Every route gives the bits of
// Composed: the epilogues keep the term order of rk_stage_f32 on the (masked) K.
// ndcn_debug_last_rhs_path: each launch with a stage epilogue or a mask sets the report outright (the H = 256 kernels their own).  A plain
// p = 0 call owns only the MID bit: below H = 256, with graph and control, it sets or clears that one and leaves the others as the
// thread's last such launch left them; with exactly one of no_graph / no_control it owns the ABL bit in the same way (rhs_abl.hip sets
// the report outright); on any other shape it leaves the report alone.
int rhs_rk_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, const float *W, const float *b, float *K,
               float *work, int H, uint32_t flags, int rk_mode, const float *y0, const float *const *h_kprev,
               const float *h_c, int n_prev, float *y_next, float rtol, float atol, double *d_out, void *d_ws,
               hipStream_t st, const RkOpt *opt, const DropArgs *drop) {
    if (drop && Xh) { set_error("dropout with a halo panel (sharded graphs) is not supported"); return NDCN_EINVAL; }
    if (drop && !(flags & NDCN_F_RELU)) { set_error("dropout without NDCN_F_RELU is not supported"); return NDCN_EINVAL; }
    if (rk_mode == 0) {                                 // reads neither the stage arguments nor RkOpt
        y0 = nullptr; h_kprev = nullptr; h_c = nullptr; n_prev = 0; y_next = nullptr; rtol = atol = 0.f; d_out = nullptr; d_ws = nullptr;
        opt = nullptr;
    }
    if (n_prev < 0 || n_prev > 5) { set_error("rhs_rk: n_prev must be 0..5"); return NDCN_EINVAL; }
    if (drop && fused_only(opt)) { set_error("dropout with x_add / x_mask / s_out is not supported"); return NDCN_EINVAL; }
    const Rhs kind = pick(A, X, Xh, W, K, H, flags, rk_mode, y0, h_kprev, n_prev, y_next, opt, drop != nullptr);
    const bool plain_p0 = rk_mode == 0 && !drop;
    // the scratch of rhs_work_bytes: rhs_plain's launches use it, and a p = 0 call without a stage epilogue asks for it whichever kernel runs
    if (!(flags & (NDCN_F_NO_GRAPH | NDCN_F_NO_CONTROL)) && !work && (kind == Rhs::Composed || plain_p0 || (!drop && kind == Rhs::MidPlain))) {
        set_error("rhs: scratch of ndcn_rhs_work_bytes() bytes required for H=%d", H);
        return NDCN_EINVAL;
    }
    const int drop_epi = drop ? NDCN_PATH_DROP_EPI : 0;
    const int halo = (Xh && A->n_cols > n_own) ? NDCN_PATH_HALO : 0;
    const int64_t n = A->n_rows * (int64_t)H;
    int rc;
    switch (kind) {
    case Rhs::Fused: {
        if (!work) { set_error("rhs_rk: scratch of ndcn_rhs_work_bytes() bytes required"); return NDCN_EINVAL; }
        rc = (flags & NDCN_F_PACKED) ? NDCN_OK : pack_weight_256(W, work, st);
        if (rc) return rc;
        const bool wide = weights_wide_range(work);
        // options that exist only inside the fused launches (input formed on the staged rows, S written on the side) have no composed
        // form: such a launch stays on the split product and says so (NDCN_PATH_RANGE; the solvers switch the options off instead)
        const bool no_fp32_form = opt && (opt->xadd || opt->xmask || opt->s_out);
        if (!wide || no_fp32_form) {
            rc = rhs_fused2_f32(A, X, Xh, n_own, work, b, K, flags, rk_mode, y0, h_kprev, h_c, n_prev, y_next, rtol, atol,
                                d_out, d_ws, st, opt);
            if (wide) {
                g_last_rhs_path |= NDCN_PATH_RANGE;
                static std::atomic<bool> warned{false};
                if (!warned.exchange(true))
                    fprintf(stderr, "[ndcn] weights with an in-row range beyond 2^%d on a fused launch that has no fp32 form (x_add / x_mask / "
                                    "s_out): the split fp16 product's guarantee (csrc/split16.h) does not cover them\n", kS16GuardBits);
            }
            return rc;
        }
        // the same launch - gather, Linear, RK epilogue - with the fp32 matrix cores as its consumer (rhs_fused2_exact.hip)
        return rhs_fused2_exact_f32(A, X, Xh, n_own, work, b, K, flags, rk_mode, y0, h_kprev, h_c, n_prev, y_next, rtol, atol, d_out, d_ws,
                                    st, opt);
    }
    case Rhs::Mid:
        g_last_rhs_path = NDCN_PATH_MID | drop_epi;
        return rhs_mid_f32(A, X, W, b, K, H, flags, rk_mode, y0, h_kprev, h_c, n_prev, y_next, st, opt, drop);
    case Rhs::Small:
        g_last_rhs_path = plain_p0 ? (g_last_rhs_path & ~NDCN_PATH_MID) : (NDCN_PATH_SMALL | drop_epi);
        return rhs_small_f32(A, X, Xh, n_own, W, b, K, H, flags, rk_mode, y0, h_kprev, h_c, n_prev, y_next, rtol, atol, d_out, d_ws, st,
                             nullptr, opt, drop);
    case Rhs::Abl:
        g_last_rhs_path = NDCN_PATH_ABL | drop_epi;
        if (abl_epilogue(rk_mode, y0, h_kprev, n_prev, y_next, opt))
            return rhs_abl_f32(A, X, W, b, K, H, flags, rk_mode, y0, h_kprev, h_c, n_prev, y_next, st, opt, drop);
        if ((rc = rhs_abl_f32(A, X, W, b, K, H, flags, 0, nullptr, nullptr, nullptr, 0, nullptr, st, nullptr, drop))) return rc;
        return rk_stage_f32(n, X, K, rk_mode, y0, h_kprev, h_c, n_prev, y_next, rtol, atol, d_out, d_ws, st, opt);
    case Rhs::Rec:
        g_last_rhs_path = NDCN_PATH_REC | halo;
        return spmm_rec_f32(A, X, Xh, n_own, K, 1.f, flags, rk_mode, y0, h_kprev, h_c, n_prev, y_next, rtol, atol, d_out, d_ws, st,
                            nullptr, opt);
    case Rhs::Wide:
        g_last_rhs_path = NDCN_PATH_WIDE | halo;
        return spmm_wide_rk_f32(A, X, Xh, n_own, K, flags, rk_mode, y0, h_kprev, h_c, n_prev, y_next, rtol, atol, d_out, d_ws, st,
                                nullptr, opt);
    case Rhs::MidPlain:
        g_last_rhs_path = NDCN_PATH_MID | drop_epi;
        if ((rc = rhs_mid_f32(A, X, W, b, K, H, flags, 0, nullptr, nullptr, nullptr, 0, nullptr, st, nullptr, drop))) return rc;
        return rk_stage_f32(n, X, K, rk_mode, y0, h_kprev, h_c, n_prev, y_next, rtol, atol, d_out, d_ws, st, opt);
    case Rhs::Composed:
        break;
    }
    // composition with the same term order: K first, its mask, then the algebra over {kprev..., K}
    if (!plain_p0) g_last_rhs_path = 0;
    else if (flags & (NDCN_F_NO_GRAPH | NDCN_F_NO_CONTROL)) g_last_rhs_path &= ~NDCN_PATH_ABL;       // (a plain p = 0 ablation call owns that bit alone)
    if ((rc = rhs_plain(A, X, Xh, n_own, W, b, K, work, H, flags, st))) return rc;
    if (drop && mask_combines(rk_mode, opt)) return dropout_combine_f32(K, n, *drop, y_next, y0, h_kprev, h_c, n_prev, st);
    if (drop && (rc = dropout_apply_f32(K, n, *drop, st))) return rc;
    if (rk_mode == 0) return NDCN_OK;
    return rk_stage_f32(n, X, K, rk_mode, y0, h_kprev, h_c, n_prev, y_next, rtol, atol, d_out, d_ws, st, opt);
}

}  // namespace ndcn
