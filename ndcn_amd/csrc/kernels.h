// Internal (C++) entry points of the kernels; the extern "C" layer in api.hip validates arguments and
// forwards here.
#pragma once
#include "common.h"
#include "dropout.h"

namespace ndcn {

// Options of an RK-epilogue launch that only the sharded callers use (ndcn_rhs_rk_f32: y1 / NDCN_F_ACCUM):
//   y1     ERROR mode - the state whose error record is formed, by ROW of this launch (NULL: X, the evaluation's input).
//          A launch over a row block of a shard, or the second phase of a two-phase evaluation (whose X is the partial sum
//          A_own X, not y1), passes it explicitly.
//   accum  ERROR mode - add this launch's {sum, bad} to d_out instead of overwriting it (an evaluation split into
//          several launches on one stream; the order of the launches fixes the order of the sum)
//   y_aux  COMBINE mode - a SECOND linear combination of the same stages, without y0:
//            y_aux = sum_{m<n_prev} c_aux[m] kprev[m] + c_aux[n_prev] K          (left to right, products rounded on their own)
//          dopri5 uses it to form E = dt sum_{j<=6} c_err[j] k_j in the launch that produces k6 - where k1, k3, k4, k5
//          are in registers anyway - so that the error launch reads {y0, E, y1} instead of {y0, k1, k3, k4, k5, k6, y1}:
//          3 P less traffic per step for 1 P written, the same sum in the same order (E holds the partial sum exactly).
//   xadd / xadd_c (plain and COMBINE with one earlier stage, operators on the rhs_fused3 path without a halo panel -
//          rhs_xadd_supported()): the evaluation's input is X + xadd_c * xadd, formed on the rows the kernel stages instead of by a
//          combine launch in front (3 panels); same product-then-sum rounding per element.
//   no_k   (a hint; COMBINE / RK4 modes) the caller reads only y_next: a kernel that can skips the store of K - an Euler step's K, the
//          fourth stage of an RK4 step.  Honoured by rhs_fused3 (one panel of HBM writes less); K must still point at a panel.
//   c_mid  (COMBINE with 4 earlier stages and no_k, rhs_dense_supported()) the K panel receives sum_{m<4} c_mid[m] kprev[m] + c_mid[4] K
//          instead of K - dopri5's midpoint sum M, formed by the launch that produces k6 for a step that covers a requested tick.
struct RkOpt { const float *y1; int accum; float *y_aux; const float *c_aux; const float *xadd; float xadd_c;
               const float *xmask; float *s_out; int no_k;      // (xmask, s_out: rhs_adj_supported)
               const float *c_mid; };

int spmm_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, float *Y, int H, float alpha,
             uint32_t flags, hipStream_t st);
int gather_rows_f32(const float *X, const int32_t *idx, int64_t n_idx, int H, float *out, hipStream_t st);
int linear_f32(const float *S, const float *W, const float *b, float *Y, int64_t n, int Hi, int Ho, uint32_t flags,
               hipStream_t st);
int rhs_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, const float *W, const float *b, float *Y,
            float *work, int H, uint32_t flags, hipStream_t st, const DropArgs *drop = nullptr);
int64_t rhs_work_bytes(int64_t n_rows, int H, uint32_t flags);
int linear_bwd_f32(const float *g, const float *Y, const float *S, const float *W, float *gS, float *gW, float *gb, void *work,
                   int64_t n, int Hi, int Ho, hipStream_t st, uint32_t flags = 0, float acc_scale = 1.f, bool accumulate = false);
int64_t linear_bwd_work_bytes(int64_t n, int Hi, int Ho);
int scale_f32(float *out, const float *x, float w, int64_t n, hipStream_t st);
int relu_bwd_f32(float *out, const float *g, const float *y, int64_t n, hipStream_t st);
int copy_f32(float *dst, const float *src, int64_t n, hipStream_t st);
int rhs_rk_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, const float *W, const float *b, float *K,
               float *work, int H, uint32_t flags, int rk_mode, const float *y0, const float *const *h_kprev,
               const float *h_c, int n_prev, float *y_next, float rtol, float atol, double *d_out, void *d_ws,
               hipStream_t st, const RkOpt *opt = nullptr, const DropArgs *drop = nullptr);
int rhs_fused_supported(int H, uint32_t flags);
int pack_weight_256(const float *W, float *Wp, hipStream_t st);
// the image at Wp was packed from weights whose in-row range exceeds the split product's guarantee (split16.h: kS16GuardBits): the
// launches that read it take the fp32 matrix-core route (rhs.hip).  False when NDCN_RANGE_GUARD=0.
bool weights_wide_range(const void *Wp);
int set_range_guard(int on);                  // ndcn_set_range_guard
int pack_weight_256_t16(const float *W, void *Wq, hipStream_t st);   // planes of W^T + per-row unscale factors: kS16Bytes + kS16TailBytes
int rhs_fused2_supported(const ndcn_csr *A, int H, uint32_t flags);
int rhs_fused2_variant(int mode, int n_prev);
int64_t rhs_fused2_partials_bytes();
// rhs_fused2_exact.hip: the same contract with the Linear on the fp32 matrix cores (Wp: the fp32 image at the head of the packed scratch)
int rhs_fused2_exact_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, const float *Wp, const float *b,
                         float *K, uint32_t flags, int mode, const float *y0, const float *const *h_kprev, const float *h_c,
                         int n_prev, float *y_next, float rtol, float atol, double *d_out, void *d_ws, hipStream_t st,
                         const RkOpt *opt = nullptr);
// mode 0: K only; 1: also y_next = y0 + sum c_m kprev_m + c_new K; 2: also the dopri5 error record into d_out
int rhs_fused2_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, const float *Wp, const float *b,
                   float *K, uint32_t flags, int mode, const float *y0, const float *const *h_kprev, const float *h_c,
                   int n_prev, float *y_next, float rtol, float atol, double *d_out, void *d_ws, hipStream_t st,
                   const RkOpt *opt = nullptr);
// fixed-order sum of n {sum, bad} fp64 pairs into d_out[0..1] (one workgroup: deterministic accept / reject)
int partials_finish(const double *partials, int n, double *d_out, hipStream_t st, int accum = 0);
// rhs_fused3.hip: the same contract as rhs_fused2_f32 for operators that carry the 16-row group-record plan (Wq: the
// split weights of pack_weight_256, i.e. Wp + 256 * 256 floats)
int rhs_fused3_supported(const ndcn_csr *A);
int rhs_xadd_supported(const ndcn_csr *A, int H, uint32_t flags, int mode, int n_prev);   // RkOpt::xadd can be honoured
int rhs_adj_supported(const ndcn_csr *A, int H, uint32_t flags, int mode, int n_prev);    // RkOpt::xmask / s_out can be honoured
int rhs_dense_supported(const ndcn_csr *A, int H, uint32_t flags);                         // RkOpt::c_mid can be honoured
// RkOpt::s_out can be honoured by the launch rhs_rk_f32 picks: rhs_adj_supported, or the narrow-panel kernel of rhs_small.hip (rhs.hip)
int rhs_s_out_supported(const ndcn_csr *A, int H, uint32_t flags, int mode, int n_prev);
int rhs_fused3_variant(int mode, int n_prev);
int rhs_fused3_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, const void *Wq, const float *b, float *K,
                   uint32_t flags, int mode, const float *y0, const float *const *h_kprev, const float *h_c, int n_prev,
                   float *y_next, float rtol, float atol, double *d_out, void *d_ws, hipStream_t st, const RkOpt *opt = nullptr);
// spmm_sweep.hip: Y = A X through the column-sweep plan (H = 256, no halo panel, alpha = 1, no activation)
int spmm_sweep_supported(const ndcn_csr *A, int H);
int spmm_sweep_f32(const ndcn_csr *A, const float *X, float *Y, hipStream_t st);
int spmm_rec_supported(const ndcn_csr *A, int H);
int spmm_rec_variant(int mode, int n_prev);
int64_t spmm_rec_partials_bytes();
// mode 0: Y = alpha (A X) [relu]; modes 1-3 (NDCN_RK_*): K = relu(A X) plus the RK algebra, as rhs_fused2_f32
int spmm_rec_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, float *Y, float alpha, uint32_t flags,
                 int mode, const float *y0, const float *const *h_kprev, const float *h_c, int n_prev, float *y_next,
                 float rtol, float atol, double *d_out, void *d_ws, hipStream_t st, const float *c_dev = nullptr,
                 const RkOpt *opt = nullptr);
// out[i] = fl(dt[0] * beta[i]), i < n: the effective coefficients of a replayed adaptive step (device-resident step size)
int scale_coef_f32(float *out, const float *beta, const float *dt, int n, hipStream_t st);
int spmm_wide_rk_supported(const ndcn_csr *A, int H);
int spmm_wide_rk_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, float *K, uint32_t flags, int mode,
                     const float *y0, const float *const *h_kprev, const float *h_c, int n_prev, float *y_next, float rtol,
                     float atol, double *d_out, void *d_ws, hipStream_t st, const float *c_dev = nullptr,
                     const RkOpt *opt = nullptr);
// rhs_small.hip: the whole ODEFunc (+ RK epilogue, modes as rhs_fused2_f32) in one launch for H <= 128
int rhs_small_supported(const ndcn_csr *A, int H, uint32_t flags);
int rhs_small_wanted(int64_t n_rows, int H, uint32_t flags);      // the same decision from the sizes alone (rhs_work_bytes)
int rhs_small_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, const float *W, const float *b, float *K,
                  int H, uint32_t flags, int mode, const float *y0, const float *const *h_kprev, const float *h_c, int n_prev,
                  float *y_next, float rtol, float atol, double *d_out, void *d_ws, hipStream_t st, const float *c_dev = nullptr,
                  const RkOpt *opt = nullptr, const DropArgs *drop = nullptr);     // drop: the factor of csrc/dropout.h in the epilogue
// rhs_mid.hip: the whole ODEFunc in one launch for 16 <= H <= 128 (H % 4 == 0) at any number of rows - mode 0 (plain), NDCN_RK_COMBINE
// (with RkOpt::y_aux / c_aux) or NDCN_RK_RK4; every panel 16-byte aligned, no halo panel; the bits of the composed path.  The switch
// (ndcn_set_rhs_mid / NDCN_RHS_MID): 0 off, 1 wherever rhs_small.hip does not take the shape, 2 every supported shape.  drop: the factor
// of csrc/dropout.h in the epilogue (NDCN_F_RELU required) - K as stored and as consumed by the stage algebra is the masked one; the
// masked calls of rhs.hip come here only under a switch of their own (ndcn_set_rhs_mid_drop / NDCN_RHS_MID_DROP: 0 off, 1 on)
int rhs_mid_mode();
int set_rhs_mid(int mode);                    // ndcn_set_rhs_mid: returns the previous mode; < 0: back to the environment's
int rhs_mid_drop_on();
int set_rhs_mid_drop(int on);                 // ndcn_set_rhs_mid_drop: returns the previous value; < 0: back to the environment's
int rhs_mid_supported(int64_t n_rows, int H, uint32_t flags, int mode);      // from the sizes alone, no device
// c_dev (nullable, device; COMBINE without drop or y_aux): the coefficients as rhs_small_f32 / spmm_rec_f32 define them - c_dev[m],
// m <= n_prev - in place of h_c (a replayed adaptive step: solver.hip).  RK4 has no such form yet: no step replays it (NDCN_EINVAL)
int rhs_mid_f32(const ndcn_csr *A, const float *X, const float *W, const float *b, float *K, int H, uint32_t flags, int mode,
                const float *y0, const float *const *h_kprev, const float *h_c, int n_prev, float *y_next, hipStream_t st,
                const RkOpt *opt = nullptr, const DropArgs *drop = nullptr, const float *c_dev = nullptr);
// rhs_abl.hip: the two ablations - no_control K = relu(A X), no_graph K = relu(X W^T + b) - in one launch for 16 <= H <= 128 (H % 4 == 0)
// at any number of rows, with rhs_mid.hip's epilogue: mode 0, NDCN_RK_COMBINE (RkOpt::y_aux / c_aux) or NDCN_RK_RK4, drop as there; every
// panel 16-byte aligned, no halo panel; the bits of the composed path.  The switch (ndcn_set_rhs_abl / NDCN_RHS_ABL): 0 off, 1 on
int rhs_abl_on();
int set_rhs_abl(int on);                      // ndcn_set_rhs_abl: returns the previous value; < 0: back to the environment's
int rhs_abl_supported(int64_t n_rows, int H, uint32_t flags);                 // from the sizes alone, no device
int rhs_abl_takes(const ndcn_csr *A, int H, uint32_t flags);                  // ... and the operator (no long-row plan for this width)
int rhs_abl_f32(const ndcn_csr *A, const float *X, const float *W, const float *b, float *K, int H, uint32_t flags, int mode,
                const float *y0, const float *const *h_kprev, const float *h_c, int n_prev, float *y_next, hipStream_t st,
                const RkOpt *opt = nullptr, const DropArgs *drop = nullptr, const float *c_dev = nullptr);   // c_dev: as rhs_mid_f32's
// linear_bwd.hip: the row chunks linear_bwd_f32 cuts the weight gradient into (`used` chunks of rpc rows) and the fixed-order sum of
// their partial blocks into gW / gb (one of them nullable)
void wgrad_chunking(int64_t n, int Hi, int Ho, int64_t *rpc, int64_t *used);
int wgrad_chunk_sum(const float *part_w, const float *part_b, float *gW, float *gb, int Hi, int Ho, int64_t used, float acc_scale,
                    bool accumulate, hipStream_t st);
// rhs_mid_bwd.hip: the reverse of one evaluation (autograd_ops.rhs_vjp) - the one implementation behind ndcn_rhs_vjp_f32 and the two
// native tapes - and its one-launch gS / gW / gb kernel for 16 <= H <= 128 (H % 4 == 0) at any number of rows: the bits of the composed
// launches.  The switch (ndcn_set_rhs_mid_bwd / NDCN_RHS_MID_BWD): 0 off, 1 the widths that measured not slower, 2 every supported shape
int rhs_mid_bwd_mode();
int set_rhs_mid_bwd(int mode);                // returns the previous mode; < 0: back to the environment's
int rhs_mid_bwd_supported(int64_t n_rows, int H, uint32_t flags, int mode);      // from the sizes alone; mode < 0: the current mode
int last_rhs_vjp_path();                      // ndcn_debug_last_rhs_vjp_path
int rhs_vjp_f32(const ndcn_csr *A, const ndcn_csr *At, const float *X, const float *K, const float *g, const float *W,
                const float *S_kept, float *gx, float *gW, float *gb, float *tmpS, float *tmpG, void *bwork, int H, uint32_t flags,
                bool premasked, float acc_scale, float alpha, bool accumulate, bool direct, bool *packed, hipStream_t st);
int64_t rhs_vjp_work_bytes(int64_t n_rows, int H, uint32_t flags);
int64_t rhs_vjp_gs_offset(int64_t n_rows, int H);
// rhs_abl_bwd.hip: the reverse of one evaluation of the two ablations for 16 <= H <= 128 (H % 4 == 0) at any number of rows, taken at the
// top of rhs_vjp_f32 - no_control: gX = alpha At (g (.) [K > 0]) in one launch (the mask rides in the transposed gather); no_graph:
// rhs_mid_bwd.hip's kernel with S = X, gS stored straight into gX (times alpha where the composed branch runs its scaling pass), then the
// chunk sum: the bits of the composed launches.  The switch (ndcn_set_rhs_abl_bwd / NDCN_RHS_ABL_BWD): 0 off, 1 on
int rhs_abl_bwd_on();
int set_rhs_abl_bwd(int on);                  // ndcn_set_rhs_abl_bwd: returns the previous value; < 0: back to the environment's
int rhs_abl_bwd_supported(int64_t n_rows, int H, uint32_t flags);             // from the sizes alone, no device
int rhs_abl_vjp_takes(const ndcn_csr *At, int64_t n_rows, int H);             // ... and the transposed operator (square, no long-row plan for H)
int rhs_abl_vjp_graph_f32(const ndcn_csr *At, const float *g, const float *K, float *gX, int H, float alpha, hipStream_t st);
// dropout (csrc/dropout.h): the descriptor in the kernels' form (NDCN_EINVAL unless 0 < p < 1) and the streaming pass K *= m.  rhs_f32 /
// rhs_rk_f32 take the mask as their last argument (NULL: p = 0 or eval mode) and the one dispatch of rhs.hip places it: in the epilogue
// of the narrow-panel launch and (under ndcn_set_rhs_mid_drop) of the rhs_mid.hip launch, by the streaming pass behind every other route
int drop_args(const ndcn_dropout *desc, DropArgs *out);
int dropout_apply_f32(float *K, int64_t n, const DropArgs &d, hipStream_t st);
// dropout_apply_f32(K) and rk_combine_f32(out, y0, {h_kprev..., K}, h_c, n_prev + 1) as one pass (h_c[n_prev]: K's coefficient): the same bits
int dropout_combine_f32(float *K, int64_t n, const DropArgs &d, float *out, const float *y0, const float *const *h_kprev, const float *h_c,
                        int n_prev, hipStream_t st);
// solve_small.hip: a whole fixed-grid solve (all ticks) in ONE launch for states that fit one CU; h_dt: the n_ticks step sizes in
// the state dtype; out: n_ticks panels.  Euler also has the reverse sweep (traj / g_out: n_ticks + 1 panels, y_0 first).
int solve_small_supported(const ndcn_csr *A, int H, uint32_t flags, int method);
int evals_per_step(int method);   // right-hand sides per fixed-grid step: euler 1, midpoint 2, rk4 4 (solver.hip)
int solve_small_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, int method, const float *y0,
                    const float *h_dt, int64_t n_ticks, float *out, hipStream_t st, float *keep = nullptr);
// ... on a grid finer than the ticks: n_steps steps, tick j (n_ticks of them, h_tick_step non-decreasing) is written after step
// h_tick_step[j] - as it is (h_tick_same[j]) or through the reference's expression; y_end (nullable while n_steps <= one chunk): the last state
int solve_small_grid_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, int method, const float *y0,
                         const float *h_dt, int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same, int64_t n_ticks,
                         float *out, float *y_end, hipStream_t st);
int solve_small_keep_supported(const ndcn_csr *A, int H, uint32_t flags);
int last_small_route();                       // ndcn_debug_last_small_route
int solve_small_bwd_supported(const ndcn_csr *A, int H, uint32_t flags, int method);
int solve_small_bwd_f32(const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H, uint32_t flags, int method,
                        const float *traj, const float *g_out, const float *h_dt, int64_t n_ticks, float *g_y0, float *g_W,
                        float *g_b, hipStream_t st, const float *keep = nullptr);
// adjoint.hip: func_eval and the three vector-Jacobian products of the adjoint system's right-hand side for ODEFunc
int64_t adjoint_rhs_work_bytes(int64_t n_rows, int H, uint32_t flags);
int adjoint_rhs_f32(const ndcn_csr *A, const ndcn_csr *At, const float *y, const float *a, const float *W, const float *b, float *K,
                    float *vjp_y, float *vjp_W, float *vjp_b, void *work, int H, uint32_t flags, hipStream_t st);
int rhs_fused_packed_f32(const ndcn_csr *A, const float *X, const float *Xh, int64_t n_own, const float *Wp,
                         const float *b, float *Y, uint32_t flags, hipStream_t st);

// dt_dev (nullable, device): the step size is read from device memory and h_c holds the bare tableau entries - the
// kernel forms fl(dt * c) itself (hipGraph replay of an adaptive step: one captured graph serves every step size)
int rk_combine_f32(float *out, const float *y0, const float *const *h_k, const float *h_c, int n_k, int64_t n,
                   hipStream_t st, const float *dt_dev = nullptr);
int rk_error_f32(const float *y0, const float *y1, const float *const *h_k, const float *h_c, int n_k, float rtol,
                 float atol, int64_t n, double *d_out, void *d_ws, hipStream_t st, const float *dt_dev = nullptr, int accum = 0);
// readout_bwd.hip: the decoder's backward for one tick of a fixed-grid reverse sweep.  gi = fma chain over c of gd[:, c] Wd[c, :] from +0;
// out = a + ((((0 + add_0) + ...) + add_k) + gi) - rk_combine_f32's order for unit coefficients - or gi alone without a and addends;
// acc (nullable; C H + C doubles, zeroed by the caller before the first tick) += {gd^T y, column sums of gd}, deterministic; ws:
// readout_bwd_ws_bytes() bytes.  1 <= C <= 15, any H >= 1 (NDCN_EINVAL otherwise); n_add <= 5.  finish: acc -> fp32 g_Wd / g_bd (nullable)
int readout_bwd_supported(int H, int C);
int64_t readout_bwd_ws_bytes(int64_t n_rows, int H, int C);
int readout_bwd_f32(float *out, const float *a, const float *const *h_add, int n_add, const float *gd, const float *Wd, const float *y,
                    int64_t n_rows, int H, int C, double *acc, void *ws, hipStream_t st);
int readout_bwd_finish_f32(const double *acc, float *g_Wd, float *g_bd, int H, int C, hipStream_t st);
// VJPs of the dopri5 panel operations (rk_bwd.hip); d_dots receives 8 doubles, d_ws: rk_bwd_ws_bytes() bytes
int64_t rk_bwd_ws_bytes();
int rk_pull_f32(float *out, const float *base, const float *const *h_p, const float *h_c, int n_p, const float *mask, const float *ua,
                const float *ub, double *d_dots, void *d_ws, int64_t n, hipStream_t st);      // tape.hip's reverse pass
int rk_dot_diff_f32(const float *g, const float *a, const float *b, double *d_dots, void *d_ws, int64_t n, hipStream_t st);
int rk_combine_bwd_f32(const float *g, const float *const *h_k, const float *h_c, int n_k, float *const *h_gk, const float *const *h_acc,
                       float *gy0, const float *acc_y0, double *d_dots, void *d_ws, int64_t n, hipStream_t st);
int rk_error_bwd_f32(const float *y0, const float *y1, const float *const *h_k, const float *h_c, int n_k, float rtol, float atol,
                     float g_r, double inv_n, float *gy0, float *gy1, float *const *h_gk, const float *acc_y0, const float *acc_y1,
                     const float *const *h_acc, double *d_dots, void *d_ws, int64_t n, hipStream_t st);
int rk_rms_bwd_f32(const float *a, const float *b, const float *y, float rtol, float atol, float coef, float *ga, float *gb,
                   float *gy, int64_t n, hipStream_t st);
int rk_dense_bwd_f32(const float *g, const float *y0, const float *y1, const float *const *h_k, float dt, float x, float *gy0,
                     float *gy1, float *const *h_gk, const float *acc_y0, const float *acc_y1, const float *const *h_acc,
                     double *d_dots, void *d_ws, int64_t n, hipStream_t st);
int rk_dense_bwd_multi_f32(const float *const *h_g, int nt, const float *y0, const float *y1, const float *const *h_k, float dt,
                           const float *h_x, float *gy0, float *gy1, float *const *h_gk, const float *acc_y0, const float *acc_y1,
                           const float *const *h_acc, double *d_dots, void *d_ws, int64_t n, hipStream_t st);
bool prof_pause(bool on);     // returns the previous state
extern thread_local int g_last_linear_path;  // ndcn_debug_last_linear_path (linear.hip)
extern thread_local int g_last_rk_bwd_path;  // ndcn_debug_last_rk_bwd_path (rk_bwd.hip)
extern thread_local int g_last_spmm_path;    // ndcn_debug_last_spmm_path (spmm.hip)
extern thread_local int64_t g_last_rk_path;  // ndcn_debug_last_rk_path (rk.hip)
extern thread_local int g_last_rhs_path;     // ndcn_debug_last_rhs_path     // no launch timing while a stream is being captured
int scaled_sumsq_f32(const float *a, const float *b, const float *y, float rtol, float atol, int64_t n, double *d_out,
                     void *d_ws, hipStream_t st);
int64_t reduce_ws_bytes();
int scaled_sumsq_pair_f32(const float *f, const float *y, float rtol, float atol, int64_t n, double *d_out4, void *d_ws,
                          void *d_ws2, hipStream_t st);
int64_t set_aten_order_max_elems(int64_t v);   // run-time override of the bound below (< 0: back to the environment's); returns the previous override
int64_t aten_order_max_elems();   // rk_error_f32 / scaled_sumsq_f32 reduce panels up to this size in ATen's float32 order (0: disabled)
// adams_vc.hip: one step of method 'adams' in three streaming passes, the bits of the scale / combine / error calls core.Adams.step
// composes it from.  h_phi / h_beta: `order` host entries (beta[0] is not read); the explicit phi beta_j phi_j are re-formed in
// registers.  n >= 1, order 1..12; an output must not overlap an input or another output (NDCN_EINVAL).
int adams_predict_f32(float *p_next, const float *y, const float *const *h_phi, const float *h_beta, const float *h_c, int order,
                      int64_t n, hipStream_t st);
int64_t adams_correct_ws_bytes();
int adams_correct_f32(float *y_next, const float *nf, const float *const *h_phi, const float *h_beta, int order, const float *p_next,
                      const float *y0, float c_corr, const float *h_coef4, unsigned mask, float rtol, float atol, int64_t n,
                      double *d_out4, void *d_ws, int64_t ws_bytes, hipStream_t st);
int adams_update_f32(float *const *h_out, const float *nf2, const float *const *h_phi, const float *h_beta, int order, int n_out,
                     int64_t n, hipStream_t st);
int interp_fit_f32(const float *y0, const float *y1, const float *const *h_k, const float *h_cmid, float dt, float *a,
                   float *b, float *c, float *d, int64_t n, hipStream_t st);
int interp_direct_f32(const float *y0, const float *y1, const float *const *h_k, const float *h_cmid, float dt,
                      const float xp[5], float *out, int64_t n, hipStream_t st);
// fit + evaluate nt <= 8 ticks of ONE accepted step in one pass (h_xp: nt x {x^4, x^3, x^2, x, 1}; h_out: nt panels)
int interp_direct_multi_f32(const float *y0, const float *y1, const float *const *h_k, const float *h_cmid, float dt,
                            const float *h_xp, float *const *h_out, int nt, int64_t n, hipStream_t st);
// the same pass with the decoder Linear(H, C) applied in registers: h_out holds nt panels of n_rows x C, each bit for bit
// linear_f32 of the tick panel interp_direct_multi_f32 would write; 64 <= H <= 512 (its row-dot route) or 16 <= H <= 60 in fours
// (its small route: a 64-row tile per workgroup), 1 <= C <= 15
int interp_readout_supported(int H, int C);
int interp_readout_f32(const float *y0, const float *y1, const float *const *h_k, const float *h_cmid, float dt, const float *h_xp,
                       float *const *h_out, int nt, const float *Wd, const float *bd, int64_t n_rows, int H, int C, hipStream_t st);
int interp_eval_f32(const float *a, const float *b, const float *c, const float *d, const float *e, const float xp[5],
                    float *out, int64_t n, hipStream_t st);
int fixed_stage_f32(int op, float *out, const float *y, const float *k1, const float *k2, const float *k3,
                    const float *k4, float dt, int64_t n, hipStream_t st, const float *dt_dev = nullptr);
// the ticks a sub-stepped fixed-grid step reports (solvers.py:92-108): h_tm[q] = t_q - t0, h_same[q] != 0: the tick is an end of the
// step (a plain copy); any nt (kMaxTicks = 8 panels per launch).  fixed_stage_emit: op 0 / 5 writing the new state and the ticks at once
int tick_emit_f32(const float *y, float dt, const float *h_tm, const int *h_same, float *const *h_out, int nt, int64_t n, hipStream_t st);
int fixed_stage_emit_f32(int op, float *out, const float *y, const float *k1, const float *k2, const float *k3, const float *k4,
                         float dt, const float *h_tm, const int *h_same, float *const *h_out, int nt, int64_t n, hipStream_t st);

// adams.hip: one Adams-Bashforth step of order n_terms = 3..11, out = y + dt * (((0 + a_0 f_0) + a_1 f_1) + ...), every product and sum
// rounded on its own; h_f newest first; out may be y, never one of h_f; any alignment (16-byte lanes where all panels share an offset)
int ab_step_f32(float *out, const float *y, const float *const *h_f, const float *h_a, int n_terms, float dt, int64_t n, hipStream_t st);
// adams_readout.hip: the same step with h_dec[t] = Wd * s_t + bd written in the same pass, t < nt <= 8: s_t the new state (h_tm[t] == 0) or tick_emit_f32's
// expression of it at offset h_tm[t]; bit for bit linear_f32 of that panel.  H, C: interp_readout_supported
int ab_step_readout_f32(float *out, const float *y, const float *const *h_f, const float *h_a, int n_terms, float dt, int64_t n_rows, int H,
                        const float *Wd, const float *bd, int C, float *const *h_dec, const float *h_tm, int nt, hipStream_t st);
// workgroups of a streaming launch over `items` work items of 256 lanes: eight per compute unit of the current device, fewer for less work
int ab_grid(int64_t items);
// adams_bwd.hip: the gradient of one evaluation gathered from the adjoints of the Adams-Bashforth steps that used it,
// out = [base +] (((0 + c_0 g_0) + c_1 g_1) + ...), n_terms = 1..11, base nullable and added last; out may be base, never one of h_g
int ab_adjoint_f32(float *out, const float *base, const float *const *h_g, const float *h_c, int n_terms, int64_t n, hipStream_t st);
// ... and of fixed_adams, from pairs of adjoints (predictor, explicit part of the corrector):
// out = [base +] ((((0 + cp_0 P_0) + cd_0 D_0) + cp_1 P_1) + cd_1 D_1 ...), n_pairs = 1..11; P_q may be D_q; out may be base, never a term
int abm_adjoint_f32(float *out, const float *base, const float *const *h_p, const float *h_cp, const float *const *h_d, const float *h_cd,
                    int n_pairs, int64_t n, hipStream_t st);
// adams_pc.hip: the predictor and one corrector pass of fixed_adams (fixed_adams.py:179-194).  predict: dy = dt * sum a_i f_i,
// delta = dt * sum m_i f_i, u = y + dy in one pass over the n_terms = 3..11 history panels (u may be y; no output may be a history panel).
// correct: dy <- c0 * f + delta in place, u = y + dy, *d_count = the elements that fail |old - new| < atol + rtol * max(|old|, |new|)
// (the counter is zeroed on the stream first; nothing else may overlap u or dy).  The lanes of ab_step_f32, any alignment, any n >= 0.
int abm_predict_f32(float *dy, float *delta, float *u, const float *y, const float *const *h_f, const float *h_a, const float *h_m,
                    int n_terms, float dt, int64_t n, hipStream_t st);
int abm_correct_f32(float *dy, float *u, const float *f, const float *delta, const float *y, float c0, float rtol, float atol, int64_t n,
                    unsigned long long *d_count, hipStream_t st);

int row_l1_normalize_f32(const float *X, float *Y, int64_t n_rows, int H, hipStream_t st);
int row_l1_normalize_bwd_f32(const float *G, const float *X, float *GX, int64_t n_rows, int H, hipStream_t st);
int gene_rhs_f32(const ndcn_csr *A, const float *x, float *out, float b, float f, float h, hipStream_t st);
int mutual_rhs_f32(const ndcn_csr *A, const float *x, float *out, float b, float k, float c, float d, float e, float h,
                   hipStream_t st);
// dynamics.hip: the three truth dynamics (kind NDCN_DYN_*, p: ndcn_dynamics::p) on an N x 1 state with the RK epilogue - modes, stage
// arguments, c_dev and the error record as rhs_small_f32 at H = 1; of RkOpt: y1 and y_aux / c_aux, NDCN_EINVAL for any other field
int dyn_rk_f32(int kind, const float *p, const ndcn_csr *A, const float *x, float *K, int mode, const float *y0,
               const float *const *h_kprev, const float *h_c, int n_prev, float *y_next, float rtol, float atol, double *d_out,
               void *d_ws, hipStream_t st, const float *c_dev = nullptr, const RkOpt *opt = nullptr);

// comm.hip
int comm_world(const ndcn_comm *c);
int comm_allreduce_sum_f64(ndcn_comm *c, double *d_buf, int n, hipStream_t st);
int64_t halo_plan_n_halo(const ndcn_halo_plan *p);
int64_t halo_plan_n_send(const ndcn_halo_plan *p);
const int32_t *halo_plan_send_idx(const ndcn_halo_plan *p);        // device array of n_send own-row indices
int halo_exchange_f32(ndcn_halo_plan *p, const float *X, int H, float *d_pack, float *X_halo, hipStream_t st);

int64_t solver_workspace_bytes(const ndcn_solver_desc *desc);
int solver_create(const ndcn_solver_desc *desc, void *workspace, int64_t ws_bytes, ndcn_solver **out);
int solver_destroy(ndcn_solver *s);
int solver_begin(ndcn_solver *s, const float *y0, double t0, hipStream_t st, bool borrow = false);
int solver_advance(ndcn_solver *s, double next_t, float *out, int64_t budget, hipStream_t st);
int solver_advance_many(ndcn_solver *s, const double *h_ticks, int64_t n_ticks, float *out, hipStream_t st);
int solver_advance_many_readout(ndcn_solver *s, const double *h_ticks, int64_t n_ticks, const float *Wd, const float *bd, int C,
                                float *out, float *scratch, hipStream_t st);
extern thread_local int g_last_readout_path;  // ndcn_last_readout_path (solver.hip)
int solver_advance_grid(ndcn_solver *s, const float *h_grid, int64_t n_grid, const int64_t *h_tick_step, const float *h_tick_time,
                        int64_t n_ticks, float *out, hipStream_t st);
int solver_stats(const ndcn_solver *s, double h[6]);
int64_t solver_steplog(const ndcn_solver *s, double *rows, int64_t cap);
// The solver's own switch for the one-launch kernels of rhs_mid.hip / rhs_abl.hip (ndcn_set_solver_mid / NDCN_SOLVER_MID; read at
// solver_create): 0 off, 1 the widths that did not measure slower, 2 every supported width.  solver_mid_takes: the sizes' part of the
// decision (no device, no operator): rhs_mid_supported with graph and control, rhs_abl_supported with exactly one of the two flags -
// at mode 1 without the widths above rhs_mid.hip's mode-1 bound (H > 96) in any variant
int solver_mid_mode();
int set_solver_mid(int mode);                 // returns the previous mode; < 0: back to the environment's
int solver_mid_takes(int64_t n_rows, int H, uint32_t flags, int mode);
int solver_rhs_kind(const ndcn_solver *s);    // NDCN_SOLVER_RHS_*

}  // namespace ndcn
