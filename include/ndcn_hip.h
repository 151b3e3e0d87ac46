/*
 * ndcn_hip.h - C ABI of libndcn_hip.so: the MI355X (gfx950) implementation of the NDCN ODEFunc hot path.
 *
 * The reference (calvin-zcx/ndcn) is pure Python and has no FFI of its own; its hot path is a set of
 * PyTorch op call sites.  Each entry point below replaces one of those call sites (or one
 * solver-side group of them) and is what a binding of the reference for this path would call.  The
 * reference-side ctypes stub is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name starts with h_ (host) ;
 *   - panels are dense row-major fp32, n_rows x H, H floats per node; 16-byte aligned base;
 *   - CSR operators are {rowptr int32[n_rows+1], colidx int32[nnz], val fp32[nnz]}, columns of a row
 *     in ascending order (summation order = stored order);
 *   - `stream` is a hipStream_t (passed as void*; NULL = the null stream); calls only ENQUEUE work, they
 *     never synchronise, allocate or free device memory, except where stated (ndcn_solver_*);
 *   - return value: 0 on success, a negative NDCN_E* code otherwise; ndcn_last_error() gives the text.
 *     Nothing throws across the boundary.
 *   - the library never falls back to a host computation.
 *
 * Reference paths are relative to the reference repository root.
 */
#ifndef NDCN_HIP_H
#define NDCN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDCN_ABI_VERSION 29
#define NDCN_API __attribute__((visibility("default")))

#define NDCN_OK          0
#define NDCN_EINVAL     -1   /* bad argument (null pointer, misaligned panel, unsupported H, ...) */
#define NDCN_EHIP       -2   /* a HIP runtime call failed; see ndcn_last_error() */
#define NDCN_ENONFINITE -3   /* solver: non-finite state  (dopri5.py:101-102 assertion)          */
#define NDCN_EUNDERFLOW -4   /* solver: t0 + dt <= t0     (dopri5.py:100 assertion)              */
#define NDCN_EMAXSTEPS  -5   /* solver: max_num_steps exceeded (dopri5.py:89 assertion)          */
#define NDCN_ESTATE     -6   /* solver handle used out of order                                   */
#define NDCN_ECAPACITY  -7   /* ndcn_fixed_adams_train_f32: the record of the corrector's evaluations is full */

/* rhs / spmm flags */
#define NDCN_F_RELU        1u   /* apply relu to the result            (neural_dynamics.py:36)   */
#define NDCN_F_NO_GRAPH    2u   /* skip A*x                            (neural_dynamics.py:27)   */
#define NDCN_F_NO_CONTROL  4u   /* skip the Linear                     (neural_dynamics.py:32)   */
#define NDCN_F_PACKED      8u   /* ndcn_rhs_f32 / ndcn_rhs_rk_f32, H = 256: `work` still holds the packed image of W that an
                                 * earlier call on this stream (flag clear, same W contents) left there - skip the re-pack   */
#define NDCN_F_ACCUM      16u   /* ndcn_rhs_rk_f32, NDCN_RK_ERROR: ADD this launch's {sum, bad} to d_out instead of overwriting
                                 * it - an evaluation split into several launches on one stream (row blocks of a shard)      */

/* integrator methods (torchdiffeq/_impl/odeint.py:8-17, the in-scope subset) */
#define NDCN_M_EULER    0
#define NDCN_M_MIDPOINT 1
#define NDCN_M_RK4      2   /* the 3/8 rule, rk_common.py:72-78 */
#define NDCN_M_DOPRI5   3

typedef struct ndcn_csr {
    int64_t n_rows;
    int64_t n_cols;           /* columns >= n_own address the halo panel (see ndcn_spmm_f32)     */
    int64_t nnz;
    const int32_t *rowptr;    /* [n_rows + 1] */
    const int32_t *colidx;    /* [nnz]        */
    const float   *val;       /* [nnz]        */
    const int32_t *row_order; /* [n_rows] or NULL: a permutation of the rows giving the order in which the
                                 kernels WALK them (a cache-locality hint, e.g. lattice tiles); results are
                                 identical for any permutation                                              */
    const int32_t *tile_order; /* [ceil(n_rows / 64)] or NULL: the order in which the fused RHS kernel walks its 64-row
                                 tiles (a permutation; locality hint like row_order - results are identical)      */
    /* Optional "group record" plan (rec = NULL when absent), built once per operator by ndcn_csr_create
     * (ndcn_amd/csrc/csr_plan.hip) for H = 256 panels.  The rows are cut into groups of rec_rows rows that are
     * consecutive in the operator's walk order (row_order, or 0..n-1); group g owns the fixed-size record
     * rec[g * rec_kib * 256 ...) of 32-bit words:
     *   [0, rec_cap)                    the DISTINCT columns the group's rows reference, ascending, padded by repetition
     *   [rec_cap, rec_cap + 2 rec_rows) per row {row id or -1, cnt | ofs << 16}; cnt = 0xffff flags a group the record
     *                                   cannot hold (the kernel gathers its rows from rowptr / colidx / val directly)
     *   [rec_cap + 2 rec_rows, ...)     the rows' entries as (index into the group's column list, fp32 value bits), row
     *                                   after row in stored (column-ascending) order
     * The SpMM kernel moves every record and every distinct neighbour row into LDS by DMA at addresses it can form
     * without first loading streamed index data (ndcn_amd/csrc/spmm_rec.hip).  Supported shapes:
     * {rec_rows, rec_cap, rec_kib} = {8, 32, 1}, {16, 40, 2} (lattice patches) and {8, 48, 2} (8 consecutive rows of a
     * ring-plus-shortcuts graph: 12 ring columns + ~2 shortcut endpoints per row).                            */
    int32_t        rec_rows, rec_cap, rec_kib, rec_groups;
    const int32_t *rec;       /* [rec_groups][rec_kib * 256] */
    /* Optional long-row plan (hub_n = 0 when absent), built once per operator by ndcn_csr_create
     * (ndcn_amd/csrc/csr_plan.hip) for graphs with a skewed degree distribution.  Rows with more than the
     * plan's threshold of entries ("hubs": a 3900-entry row of a 10^6-node Barabasi-Albert graph is otherwise
     * one wave's sequential work inside the fused RHS kernel) are evaluated ahead of that kernel:
     *   hub_seg_* : CSR over SEGMENTS of the hub rows (<= 256 entries each; columns as in colidx),
     *               S_seg = hub_seg x X                         -> hub_Sseg [hub_nseg][H]
     *   hub_cmb_* : CSR [hub_n x hub_nseg] of ones, row h = the segments of hub h in order,
     *               S_hub = hub_cmb x S_seg                     -> hub_S [hub_n][H]
     *   lt_*      : the operator with every hub row replaced by ONE entry (column n_cols + h, value 1): the
     *               fused kernel reads S_hub as its second ("halo") panel.
     * hub_S / hub_Sseg are scratch owned by the operator (one launch stream at a time).  Used by ndcn_rhs_f32 /
     * ndcn_rhs_rk_f32 / the solver when H == hub_H and either no halo panel is passed or hub_S lies directly behind
     * the halo panel in ONE allocation (hub_S == X_halo + n_halo * H: the kernel's second panel is then
     * [halo | hubs]; node-range shards of power-law graphs, ndcn_amd/sharding.py).                              */
    int32_t        hub_n, hub_nseg, hub_H;
    int64_t        hub_nnz, lt_nnz;
    const int32_t *hub_seg_rowptr;  /* [hub_nseg + 1] */
    const int32_t *hub_colidx;      /* [hub_nnz] */
    const float   *hub_val;         /* [hub_nnz] */
    const int32_t *hub_cmb_rowptr;  /* [hub_n + 1] */
    const int32_t *hub_cmb_colidx;  /* [hub_nseg] = 0 .. hub_nseg-1 */
    const float   *hub_cmb_val;     /* [hub_nseg] ones */
    const int32_t *lt_rowptr;       /* [n_rows + 1] */
    const int32_t *lt_colidx;       /* [lt_nnz] */
    const float   *lt_val;          /* [lt_nnz] */
    float         *hub_Sseg;        /* [hub_nseg][hub_H] */
    float         *hub_S;           /* [hub_n][hub_H] */
    /* Facts about the arrays that some entry points need and would otherwise read back from the device at every call
     * (ndcn_solve_small_*: the ELL width; its reverse sweep: whether A^T = A).  0 = not known: the library finds out, with one
     * small device-to-host copy per call.  ndcn_csr_create fills max_row_len; the Python binding fills both once per operator. */
    int32_t        max_row_len;     /* the longest row, or 0 */
    int32_t        symmetric;       /* 1: the stored arrays equal those of the transpose; 2: they do not; 0: unknown */
    /* Optional column-sweep plan (sweep_ent = NULL when absent), built by ndcn_csr_create for H = 256 operators WITHOUT
     * locality whose rows are long relative to their count (a 10^5-node G(n,p) graph of mean degree 40: heat_dynamics.py:89 at
     * BASELINE config 2).  A row gather fetches nnz rows of X through the fabric (L2 hit rate 6 %); the sweep keeps the partial
     * sums of ALL rows in registers and lets every XCD walk the columns of X in ascending order, so that the rows of X an XCD
     * needs at one time form a window of its 4 MiB L2: 8 * n_cols rows cross the fabric per pass instead of nnz
     * (ndcn_amd/csrc/spmm_sweep.hip).  Layout: the rows are cut into sweep_passes passes of <= 100 352 rows; a pass gives each of
     * its 8 x 256 waves a "slab" of sweep_rpw consecutive rows (8 XCD chunks of ceil(rows / 8) rows, 256 slabs per chunk);
     *   sweep_slab [passes * 2048][2]  {first entry (a multiple of 8), entries} of the slab in sweep_ent
     *   sweep_ent  pairs of 32-bit words {row within the slab << 24 | column, fp32 value bits}: the slab's entries merged over
     *              its rows and sorted by column - per row still in ascending column order, i.e. the fma chain of a sequential
     *              CSR loop: results are bit-identical to it - padded to groups of 8 with {49 << 24, 0}
     *   sweep_prog [passes][8][256] + [passes]   one word per wave: (launch tag << 16) | column block it fetches from, then one
     *              launch counter per pass (the tag's source: kept on the device so that a hipGraph replay advances it) - waves of an XCD
     *              keep within sweep_window blocks of 2^sweep_logb columns of each other (a locality hint with a bounded wait,
     *              never needed for correctness)
     *   sweep_S    [n_rows][256] scratch for S = A X in front of the Linear (ndcn_rhs_f32 / ndcn_rhs_rk_f32: the fused kernel
     *              then runs on the identity operator sweep_eye_* over S, whose 16-row group records stage S by LDS-DMA:
     *              rhs_fused3) - owned by the operator, like hub_S: one launch stream at a time.  Used when no halo panel is
     *              passed.                                                                                                 */
    int32_t         sweep_passes, sweep_rpw, sweep_logb, sweep_window;
    int64_t         sweep_rows_per_pass;
    const uint32_t *sweep_ent;
    const int32_t  *sweep_slab;
    uint32_t       *sweep_prog;
    float          *sweep_S;
    const int32_t  *sweep_eye_rowptr;  /* [n_rows + 1] = 0 .. n_rows */
    const int32_t  *sweep_eye_colidx;  /* [n_rows] = 0 .. n_rows - 1 */
    const float    *sweep_eye_val;     /* [n_rows] ones */
    const int32_t  *sweep_eye_rec;     /* the identity operator's group-record plan {16, 40, 2}: the dense stage runs rhs_fused3 */
    int32_t         sweep_eye_groups;
} ndcn_csr;

/* ------------------------------------------------------------------------------------------------
 * Operator handle.  The reference holds its operator `A` by reference on the module (neural_dynamics.py:9-18: `self.A = A`)
 * and the caller converts it once, before model construction (heat_dynamics.py:170-175: dense -> sparse COO, .to(device)).
 * The counterpart: hand the CSR arrays over ONCE and keep the handle next to the model.  ndcn_csr_create builds - on the
 * device, from the arrays alone - every plan the H = 256 kernels select on (struct ndcn_csr above: the group-record plan
 * with its lattice walk orders, the long-row plan), so a caller that binds nothing but this header reaches the same kernels
 * (rhs_fused3, spmm_rec) as the Python package, whose ndcn_amd/csr.py is a binding of these calls.
 *   rowptr / colidx / val   DEVICE arrays owned by the caller; they must outlive the handle (the view points into them)
 *   H                       panel width the operator will be applied to (plans exist for H = 256; other widths: a bare view)
 *   hints                   nullable; zero-initialise, then set what applies:
 *     lattice_row_base / lattice_n_own   this operator is a ROW BLOCK of a node-range shard: row r is node row_base + r of the
 *                           shard, columns < n_own are the shard's own nodes, columns >= n_own halo rows (lattice_n_own = 0:
 *                           a whole graph; stencil detection then requires a square operator)
 *     n_halo                rows of the halo panel that will be passed next to X: the long-row plan lays the hubs' scratch
 *                           rows out directly behind them ([halo | hub rows], ndcn_csr_halo_panel)
 *     row_order             [n_rows] walk order given by the caller (the view's row_order; also groups the records)
 *     group_order / n_group_order   row ids (-1 = empty slot) in the order the records group them, e.g. a lattice's patches
 *     rec_rows / rec_cap / rec_kib  != 0: build exactly this record shape and keep it whatever it covers (default: the
 *                           shapes are tried and one is kept only if it holds >= 90 % of the entries and stages <= 3/4 of
 *                           the rows a direct gather would fetch)
 *     hub_threshold         > 0: rows longer than this leave the fused kernel; 0: automatic (the lowest of 32 / 64 / 128 that
 *                           moves <= 5 % of the rows); < 0: no long-row plan
 *     flags                 NDCN_PLAN_*
 * Allocates the plans with hipMalloc (synchronises); every other call takes ndcn_csr_view(handle).  `stream` orders the
 * plan kernels; the call returns after they have finished.                                                              */
typedef struct ndcn_csr_handle ndcn_csr_handle;
typedef struct ndcn_csr_hints {
    int64_t        lattice_row_base, lattice_n_own;
    int64_t        n_halo;
    const int32_t *row_order;
    const int32_t *group_order;
    int64_t        n_group_order;
    int32_t        rec_rows, rec_cap, rec_kib;
    int32_t        hub_threshold;
    uint32_t       flags;
} ndcn_csr_hints;
#define NDCN_PLAN_NO_REC            1u   /* no group-record plan                                                     */
#define NDCN_PLAN_NO_STENCIL        2u   /* do not look for a lattice stencil (records group consecutive rows)        */
#define NDCN_PLAN_NO_TILE_ORDER     4u   /* no tile walk order for the fused kernel                                   */
#define NDCN_PLAN_NO_HUB            8u   /* no long-row plan                                                          */
#define NDCN_PLAN_EXTERNAL_SCRATCH 16u   /* the caller provides the long-row plan's scratch (ndcn_csr_set_hub_scratch) */
#define NDCN_PLAN_ORDER_ONLY       32u   /* lattice detection and walk orders only, no records                        */
#define NDCN_PLAN_NO_SWEEP         64u   /* no column-sweep plan                                                      */
#define NDCN_PLAN_FORCE_SWEEP     128u   /* build the column-sweep plan whatever the fetch arithmetic says (tests)     */
NDCN_API int ndcn_csr_create(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                             const float *val, int H, const ndcn_csr_hints *hints, void *stream, ndcn_csr_handle **out);
NDCN_API int ndcn_csr_destroy(ndcn_csr_handle *h);
/* the struct every other entry point takes; valid until ndcn_csr_destroy */
NDCN_API const ndcn_csr *ndcn_csr_view(const ndcn_csr_handle *h);
/* h_out = {rec_rows, rec_cap, rec_kib, rec_groups, entries held by records, distinct columns staged by them, lattice stride
 * (0: none), slots of the group order, hub_n, hub_nseg, hub threshold, hub_nnz, lt_nnz, n_halo, has tile order, H}     */
NDCN_API int ndcn_csr_info(const ndcn_csr_handle *h, int64_t h_out[16]);
/* the group order the records were built on when the library found it (a detected lattice): [info[7]] int32, or NULL    */
NDCN_API const int32_t *ndcn_csr_group_order(const ndcn_csr_handle *h);
/* long-row plan: the [n_halo + hub_n][H] buffer whose head receives the halo rows and whose tail holds the hubs' rows - pass
 * it as X_halo (NULL without a long-row plan, or before ndcn_csr_set_hub_scratch under NDCN_PLAN_EXTERNAL_SCRATCH)        */
NDCN_API float *ndcn_csr_halo_panel(const ndcn_csr_handle *h);
/* NDCN_PLAN_EXTERNAL_SCRATCH: Sseg [hub_nseg][H] and halo_S [n_halo + hub_n][H], 16-byte aligned, owned by the caller     */
NDCN_API int ndcn_csr_set_hub_scratch(ndcn_csr_handle *h, float *Sseg, float *halo_S);
/* column-sweep plan: h_out = {passes, rows per wave, log2 of the column block, window in blocks, padded entries, rows per pass,
 * 1 if the scratch panel is set, 0} (all zero without the plan); under NDCN_PLAN_EXTERNAL_SCRATCH the caller provides the
 * [n_rows][256] scratch panel (16-byte aligned) before the first right-hand side                                            */
NDCN_API int ndcn_csr_sweep_info(const ndcn_csr_handle *h, int64_t h_out[8]);
NDCN_API int ndcn_csr_set_sweep_scratch(ndcn_csr_handle *h, float *S);

NDCN_API int         ndcn_abi_version(void);
NDCN_API const char *ndcn_last_error(void);            /* thread-local, valid until the next failing call */
/* {multiProcessorCount, 8 XCDs assumed, warpSize, clock kHz, totalGlobalMem>>20, l2CacheSize>>10}      */
NDCN_API int         ndcn_device_info(int64_t h_out[6]);

/* ------------------------------------------------------------------------------------------------
 * Y = alpha * (A X)   [then relu if NDCN_F_RELU]
 * replaces torch.sparse.mm(A, x)  neural_dynamics.py:29 (and torch.mm(A, x) :31 for a dense A held as
 * CSR); ode_gcn.py:53; models.py:18; heat_dynamics.py:201 (alpha = -k, H = 1).
 * X_halo (nullable): rows of remote nodes; a column c >= n_own reads X_halo[c - n_own] (multi-GPU
 * node-range sharding). With X_halo == NULL every column must be < n_own == A->n_cols.
 * Y must not alias X.
 */
NDCN_API int ndcn_spmm_f32(const ndcn_csr *A, const float *X, const float *X_halo, int64_t n_own,
                  float *Y, int H, float alpha, uint32_t flags, void *stream);

/* Y[n, H_out] = S[n, H_in] W^T + b  [then relu]; W is nn.Linear's [H_out, H_in] row-major, b nullable.
 * replaces self.wt(x) neural_dynamics.py:33 ; the encoder/decoder Linears :143-148 ; models.py:15.
 * Y must not alias S. */
NDCN_API int ndcn_linear_f32(const float *S, const float *W, const float *b, float *Y,
                    int64_t n, int H_in, int H_out, uint32_t flags, void *stream);

/* GraphConvolution.forward in the reference's own order (models.py:14-18; neural_dynamics.py:171-176): support = X W^T + b, then
 * Y = A support  [then relu] - i.e. ndcn_linear_f32 followed by ndcn_spmm_f32 in ONE call (two launches on `stream`).
 * X [n_cols(A), H_in], Y [n_rows(A), H_out]; work: ndcn_gcn_work_bytes() bytes of device scratch (the support panel).       */
NDCN_API int ndcn_gcn_f32(const ndcn_csr *A, const float *X, const float *W, const float *b, float *Y, float *work,
                          int H_in, int H_out, uint32_t flags, void *stream);
NDCN_API int64_t ndcn_gcn_work_bytes(int64_t n_cols, int H_out);

/* Backward of Y = act(S W^T + b) - the reference trains by plain autograd through every solver op
 * (heat_dynamics.py:333, dgnn.py:204; neural_dynamics.py:33,36,143-148).  gZ = g (.) [Y > 0] when the ReLU output Y is
 * given (nullable: no activation; zero where Y <= 0, g elsewhere, a NaN Y included - torch's threshold_backward), then
 *   gS [n, H_in]      = gZ W               (nullable)
 *   gW [H_out, H_in]  = gZ^T S             (nullable; reduction over rows split into chunks, partials summed in a fixed
 *                                           order: deterministic, no atomics)
 *   gb [H_out]        = column sums of gZ  (nullable)
 * S: the forward input (needed for gW).  work: ndcn_linear_bwd_work_bytes() bytes of device scratch (gW / gb; with
 * H_in = H_out = 256 also gS: given scratch, the product runs on the fp16 matrix cores from two-piece splits of both
 * operands - fp32-grade, as the forward kernels - and the planes of W^T are packed there; without it, the fp32 MFMA).   */
NDCN_API int ndcn_linear_bwd_f32(const float *g, const float *Y, const float *S, const float *W, float *gS, float *gW,
                                 float *gb, void *work, int64_t n, int H_in, int H_out, uint32_t flags, void *stream);
/* flags: NDCN_F_PACKED (H_in = H_out = 256, gS) - `work` still holds the planes of W^T that an earlier call with the same W and
 * the same n packed there (its tail; the head is this call's scratch): the backward of a solve evaluates the right-hand side's
 * VJP dozens of times between two weight updates.                                                                          */
NDCN_API int64_t ndcn_linear_bwd_work_bytes(int64_t n, int H_in, int H_out);
/* out = w * x: the VJP of one term of the Runge-Kutta linear combinations (rk_common.py:51,75-78; interp.py:21-35). */
NDCN_API int ndcn_scale_f32(float *out, const float *x, float w, int64_t n_elem, void *stream);
/* out = 0 where y <= 0, else g: the VJP of relu given its OUTPUT y (neural_dynamics.py:36; the no_control RHS) - torch's
 * threshold_backward, so a NaN output passes g. */
NDCN_API int ndcn_relu_bwd_f32(float *out, const float *g, const float *y, int64_t n_elem, void *stream);
/* dst = src, the library's plain streaming pass (16 bytes per lane, non-temporal): what `x.clone()` / the solver's state
 * hand-overs cost, and the measured HBM ceiling bench.py quotes next to the 8 TB/s spec peak.                            */
NDCN_API int ndcn_copy_f32(float *dst, const float *src, int64_t n_elem, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Vector-Jacobian products of the dopri5 panel operations.  The reference's vendored torchdiffeq differentiates through
 * its step-size controller - dt, dt * beta, the error ratio, the initial-step norms and the interpolation abscissa are
 * tensors with autograd history (rk_common.py:41-61, misc.py:84-170, interp.py:38-65) - and the drivers train by plain
 * backprop through the solver.  Each call is ONE pass: every panel gradient of the operation (h_gk / g* entries may be
 * NULL) plus, in d_dots[0..7] (fp64, fixed-order sums), the inner products that become the gradients of the scalar
 * inputs.  d_ws: ndcn_rk_bwd_ws_bytes() bytes of device scratch.
 *   combine   (misc.py:22-25)     y = y0 + sum_j c_j k_j :  gk_j = c_j g ;  d_dots[j] = <g, k_j> (= g_cj) ;  g_y0 = g
 *   error     (misc.py:146-157)   r = mean((sum_j c_j k_j / tol)^2), tol = atol + rtol max(|y0|, |y1|), upstream g_r,
 *                                 inv_n = 1 / numel :  gk_j, gy0, gy1 ;  d_dots[j] = d r / d c_j (multiply by g_r)
 *   rms       (misc.py:71-76)     o = ||(a - b) / (atol + |y| rtol)||_2 / sqrt(N), coef = g_o / (||.|| sqrt(N)) :  ga, gb, gy
 *   interp    (dopri5.py:39-45, interp.py:21-65)  o = dense output at abscissa x for step size dt :  gy0, gy1, gk_0..6 ;
 *                                 d_dots[0] = <g, d o / d x>, d_dots[1] = <g, d o / d dt>                              */
NDCN_API int64_t ndcn_rk_bwd_ws_bytes(void);
/* Accumulating form (h_acc / acc_y0 / acc_y1, all nullable, entries nullable): a panel that feeds SEVERAL later operations - every
 * stage derivative of a Runge-Kutta step does - receives one gradient per consumer, which autograd would add up with a pass of its
 * own each (`add` kernels were 24 % of a dopri5 training step).  Given the gradient such a panel has ALREADY received (acc), the
 * kernels write  gk_j = acc_j + (this operation's contribution)  in the pass they make anyway; outputs may alias their acc.
 * combine: gy0 = acc_y0 + g is written only when acc_y0 is given (without one, g_y0 is g itself).                                */
NDCN_API int ndcn_rk_combine_bwd_f32(const float *g, const float *const *h_k, const float *h_c, int n_k, float *const *h_gk,
                                     const float *const *h_acc, float *gy0, const float *acc_y0, double *d_dots, void *d_ws,
                                     int64_t n_elem, void *stream);
/* The total gradient of a stage derivative in the reverse pass of an attempted step (the tape's pull), ONE pass (ABI 20):
 *   out = base + ((c_0 p_0 + c_1 p_1) + ...)  - ndcn_rk_combine_f32's order and arithmetic (the same bits);
 *         base nullable; with mask (nullable, a ReLU output) 0 where mask <= 0 (torch's threshold_backward: a NaN mask passes)
 *   d_dots[0] = <p_0, ua - ub>  (ua nullable: no product, d_dots / d_ws may be NULL then; ub nullable: <p_0, ua>; 0 for n = 0)
 * 1 <= n_p <= 8 terms; h_p / h_c are HOST arrays of device panels / coefficients.                                                  */
NDCN_API int ndcn_rk_pull_f32(float *out, const float *base, const float *const *h_p, const float *h_c, int n_p, const float *mask,
                              const float *ua, const float *ub, double *d_dots, void *d_ws, int64_t n_elem, void *stream);
/* d_dots[0] = <g, a - b> (b nullable: <g, a>), fp64 partial sums in a fixed order.  For a stage sum u = y0 + dt sum_j beta_j k_j the
 * gradient of dt is <g_u, u - y0> / dt - three panels read instead of one per term (rk_common.py:41-51 differentiated).            */
NDCN_API int ndcn_rk_dot_diff_f32(const float *g, const float *a, const float *b, double *d_dots, void *d_ws, int64_t n_elem,
                                  void *stream);
NDCN_API int ndcn_rk_error_bwd_f32(const float *y0, const float *y1, const float *const *h_k, const float *h_c, int n_k,
                                   float rtol, float atol, float g_r, double inv_n, float *gy0, float *gy1,
                                   float *const *h_gk, const float *acc_y0, const float *acc_y1, const float *const *h_acc,
                                   double *d_dots, void *d_ws, int64_t n_elem, void *stream);
NDCN_API int ndcn_rk_rms_bwd_f32(const float *a, const float *b, const float *y, float rtol, float atol, float coef, float *ga,
                                 float *gb, float *gy, int64_t n_elem, void *stream);
NDCN_API int ndcn_dopri5_interp_bwd_f32(const float *g, const float *y0, const float *y1, const float *const *h_k /*7*/,
                                        float dt, float x, float *gy0, float *gy1, float *const *h_gk /*7*/, const float *acc_y0,
                                        const float *acc_y1, const float *const *h_acc /*7*/, double *d_dots, void *d_ws,
                                        int64_t n_elem, void *stream);

/* n_t <= 7 ticks of ONE accepted step in one pass: the forward (fit + evaluate, as ndcn_dopri5_interp_direct_f32 per tick - the same
 * bits) and its VJP (as ndcn_dopri5_interp_bwd_f32 summed over the ticks; d_dots[t] = <g_t, d o / d x_t>, d_dots[7] = sum_t <g_t,
 * d o / d dt>).  The drivers sample 16-120 ticks over a handful of steps (heat_dynamics.py:35,123; dgnn.py:173-182): the step's
 * panels are read once per launch instead of once per tick.  h_out / h_g: HOST arrays of n_t device panels; h_xpow: n_t x 5.       */
NDCN_API int ndcn_dopri5_interp_direct_multi_f32(const float *y0, const float *y1, const float *const *h_k /*7*/,
                                                 const float *h_cmid /*7*/, float dt, const float *h_xpow, float *const *h_out,
                                                 int n_t, int64_t n_elem, void *stream);
NDCN_API int ndcn_dopri5_interp_bwd_multi_f32(const float *const *h_g, int n_t, const float *y0, const float *y1,
                                              const float *const *h_k /*7*/, float dt, const float *h_x, float *gy0, float *gy1,
                                              float *const *h_gk /*7*/, const float *acc_y0, const float *acc_y1,
                                              const float *const *h_acc /*7*/, double *d_dots, void *d_ws, int64_t n_elem,
                                              void *stream);

/* The whole ODEFunc.forward in one call: Y = relu(W (A X) + b) honouring NO_GRAPH / NO_CONTROL
 * (neural_dynamics.py:20-39; dropout p = 0 or eval mode - ndcn_rhs_drop_f32 below is the training form with 0 < p < 1).  `work`: device scratch of ndcn_rhs_work_bytes() bytes, 16-byte
 * aligned (H = 256: the fused SpMM->LDS->MFMA kernel keeps its packed weights there; other widths: the
 * S = A X panel between the SpMM and the Linear kernel; 0 bytes when the Linear or the SpMM is skipped). */
NDCN_API int ndcn_rhs_f32(const ndcn_csr *A, const float *X, const float *X_halo, int64_t n_own,
                 const float *W, const float *b, float *Y, float *work, int H, uint32_t flags, void *stream);
NDCN_API int64_t ndcn_rhs_work_bytes(int64_t n_rows, int H, uint32_t flags);

/* The right-hand side of the ADJOINT system for ODEFunc (odeint_adjoint: torchdiffeq/_impl/adjoint.py:34-59, where the reference
 * evaluates func under enable_grad and calls torch.autograd.grad with cotangent -adj_y at EVERY evaluation of the backward
 * solve).  With f = relu(W (A y) + b) the three vector-Jacobian products are closed forms; one call, no torch graph:
 *   K     [n][H]  = ODEFunc(y)                              (func_eval)
 *   vjp_y [n][H]  = -A^T ((a (.) [K > 0]) W)                (d/dt of adj_y)
 *   vjp_W [H][H]  = -(a (.) [K > 0])^T (A y)                (d/dt of adj_params, weight part; nn.Linear's [out][in] layout)
 *   vjp_b [H]     = -column sums of a (.) [K > 0]           (bias part)
 * (d/dt of adj_t is zero: the reference ODEFunc ignores t, neural_dynamics.py:20-26.)  a = adj_y.  A_t: the operator's
 * transpose as CSR.  NDCN_F_NO_GRAPH / NDCN_F_NO_CONTROL as ndcn_rhs_f32 (NO_CONTROL: vjp_W / vjp_b are not written).
 * work: ndcn_adjoint_rhs_work_bytes() bytes, 256-byte aligned.  b nullable.                                              */
NDCN_API int ndcn_adjoint_rhs_f32(const ndcn_csr *A, const ndcn_csr *A_t, const float *y, const float *a, const float *W,
                                  const float *b, float *K, float *vjp_y, float *vjp_W, float *vjp_b, void *work, int H,
                                  uint32_t flags, void *stream);
NDCN_API int64_t ndcn_adjoint_rhs_work_bytes(int64_t n_rows, int H, uint32_t flags);

/* ODEFunc.forward PLUS the Runge-Kutta algebra that consumes its result, in one pass over the panel
 * (H = 256: inside the fused kernel's epilogue; other widths: the same result from separate kernels).
 *   rk_mode 0                  K = ODEFunc(X)                                   (= ndcn_rhs_f32)
 *   rk_mode NDCN_RK_COMBINE    also y_next = y0 + sum_{m<n_prev} h_c[m] kprev[m] + h_c[n_prev] K
 *                              (stage input of the NEXT evaluation, rk_common.py:51; K is the last term)
 *   rk_mode NDCN_RK_ERROR      also d_out = {sum ((sum_m h_c[m] k_m) / (atol + rtol max(|y0|, |X|)))^2,
 *                              non-finite count of X}: the dopri5 error record, X being y1 (rk_common.py:60,
 *                              misc.py:146-157, dopri5.py:101-102); d_ws: ndcn_reduce_ws_bytes() bytes
 *   rk_mode NDCN_RK_RK4        also y_next = the input of the next stage of the 3/8-rule RK4 step - or, for the last
 *                              stage, the step's result - in the reference's operator order (rk_common.py:72-78,
 *                              solvers.py:92); n_prev = stage index 0..3, kprev = the earlier stages, h_c[0] = dt:
 *                                0: y0 + dt K / 3            1: y0 + dt (K - k1 / 3)
 *                                2: y0 + dt (k1 - k2 + K)    3: y0 + (k1 + 3 k2 + 3 k3 + K) dt / 8
 *                              (y_next may alias y0 here: both are row-local to the epilogue)
 * y1 (nullable, NDCN_RK_ERROR only): the state whose error record is formed, indexed by ROW OF THIS LAUNCH; NULL = X, the
 *   evaluation's own input (the single-launch case).  Two callers pass it: a launch over a row block [a, b) of a shard
 *   (X stays the whole own panel because columns index it; y1 = X + a * H), and the second phase of a two-phase
 *   evaluation, whose X is the partial sum A_own X rather than the state (ndcn_amd/sharding.py).  With NDCN_F_ACCUM the
 *   record is added to d_out.
 * y_aux / h_c_aux (nullable, NDCN_RK_COMBINE only): a SECOND linear combination of the same stages, without y0,
 *   y_aux = sum_{m<n_prev} h_c_aux[m] kprev[m] + h_c_aux[n_prev] K   (left to right, products rounded on their own),
 *   written in the same pass.  dopri5 forms E = dt sum_{j<=6} c_err[j] k_j this way in the launch that produces k6, whose
 *   epilogue holds k1, k3, k4, k5 already; the error launch then runs with n_prev = 1, kprev = {E}, h_c = {1, dt c_err[7]} and
 *   reads {y0, E, y1} instead of {y0, k1, k3, k4, k5, k6, y1}: 3 P less HBM traffic per step, the same sum in the same order
 *   (rk_common.py:60; E is the exact partial sum).  NDCN_RK_ERROR therefore accepts n_prev = 1 besides dopri5's 5 in the fused kernels.
 * h_kprev / h_c are HOST arrays (n_prev <= 5 device pointers; n_prev + 1 coefficients, already dt * beta in
 * fp32).  X, K, y_next, y0 and the kprev panels must not alias each other.                              */
#define NDCN_RK_COMBINE 1
#define NDCN_RK_ERROR   2
#define NDCN_RK_RK4     3
NDCN_API int ndcn_rhs_rk_f32(const ndcn_csr *A, const float *X, const float *X_halo, int64_t n_own,
                             const float *W, const float *b, float *K, float *work, int H, uint32_t flags,
                             int rk_mode, const float *y0, const float *const *h_kprev, const float *h_c, int n_prev,
                             float *y_next, const float *y1, float *y_aux, const float *h_c_aux, float rtol, float atol,
                             double *d_out, void *d_ws, void *stream);
/* The evaluation that OPENS a dopri5 step (rk_common.py:45-51 with i = 0): K = f(X + x_add_c * x_add), and in the same pass
 * y_next = y0 + (h_c[0] * k_prev + h_c[1] * K) - i.e. ndcn_rk_combine_f32(tmp, X, {x_add}, {x_add_c}) followed by
 * ndcn_rhs_rk_f32(..., tmp, ..., NDCN_RK_COMBINE, y0, {k_prev}, h_c, 1, y_next) without the temporary: the sum is formed on
 * the neighbour rows the kernel stages (one product, one sum per element: the same bits), 3 panels of traffic less.  For the
 * operators / widths ndcn_rhs_xadd_supported() accepts (H = 256, a 2-D lattice's group-record plan, no halo panel,
 * NDCN_RK_COMBINE with n_prev = 1); NDCN_EINVAL otherwise.  In the dopri5 step X = y0, x_add = k_prev = k1.             */
NDCN_API int ndcn_rhs_xadd_supported(const ndcn_csr *A, int H, uint32_t flags, int rk_mode, int n_prev);
NDCN_API int ndcn_rhs_rk_xadd_f32(const ndcn_csr *A, const float *X, const float *x_add, float x_add_c, const float *W,
                                  const float *b, float *K, float *work, int H, uint32_t flags, const float *y0,
                                  const float *k_prev, const float *h_c, float *y_next, void *stream);

/* The two halves of odeint_adjoint's right-hand side on the fused launch (reference torchdiffeq/_impl/adjoint.py:34-59, where
 * torch.autograd.grad forms -a^T df/dy and -a^T df/dtheta at every evaluation; ndcn_amd/torchdiffeq/_impl/adjoint_fused.py):
 *   s_out  (forward half, launch over (A, W, b)): besides K and the stage algebra, S = A X is written - the weight gradient
 *          gZ^T S of the same evaluation needs it (otherwise a second SpMM);
 *   x_mask (transposed half, launch over (A^T, W^T) without bias / activation): the evaluation's input is X (.) [x_mask > 0],
 *          formed on the rows the kernel stages - X = the adjoint state, x_mask = K of the forward half, i.e. the gathered rows are
 *          gZ = a (.) [K > 0] without a panel of its own (3 panels of traffic).
 * Exactly one of the two per call; arguments otherwise as ndcn_rhs_rk_f32 (no halo panel, no y_aux).  Provided for the operators /
 * launches ndcn_rhs_adj_supported() accepts: H = 256, a 2-D lattice's group-record plan, NDCN_RK_COMBINE with n_prev = 1..4 and
 * NDCN_RK_ERROR with n_prev = 5 (the launches of a dopri5 step); NDCN_EINVAL otherwise.                                           */
NDCN_API int ndcn_rhs_adj_supported(const ndcn_csr *A, int H, uint32_t flags, int rk_mode, int n_prev);
NDCN_API int ndcn_rhs_rk_adj_f32(const ndcn_csr *A, const float *X, const float *x_mask, float *s_out, const float *W, const float *b,
                                 float *K, float *work, int H, uint32_t flags, int rk_mode, const float *y0,
                                 const float *const *h_kprev, const float *h_c, int n_prev, float *y_next, const float *y1,
                                 float rtol, float atol, double *d_out, void *d_ws, void *stream);

/* Dropout on the right-hand side (neural_dynamics.py:34: dropout between the Linear and the ReLU; dgnn.py's default p = 0.5).
 * The mask is a pure function of (p, seed, evaluation, flat element index i = row * H + col) and of nothing else - not of the
 * route, the launch geometry or H - so that a reverse pass which re-forms a stage re-creates its mask from three numbers:
 *   p32 = float32(p), 0 < p32 < 1;  s = 1.0f / (1.0f - p32) in float32;  T = floor(double(p32) * 2^32);
 *   Philox4x32-10 with counter (lo32(i >> 2), hi32(i >> 2), lo32(evaluation), hi32(evaluation)) and key (lo32(seed), hi32(seed));
 *   u = output word i & 3;  kept iff u >= T;  m = kept ? s : 0;   K' = relu(z) * m (one rounded product; NaN * 0 stays NaN).
 * m is 0 or s > 0, so relu(z * m) = relu(z) * m: the factor multiplies the launch's output K before it is stored and before the
 * stage algebra consumes it.  [K' > 0] = [z > 0 and kept]: the exact gradient is gZ = s * g * [K' > 0], i.e. the existing
 * backward kernels masked by the stored K' (ndcn_linear_bwd_f32 with Y = K', ndcn_relu_bwd_f32) times the scalar s - no mask is
 * stored or re-created in the backward.
 * ndcn_rhs_drop_f32 / ndcn_rhs_rk_drop_f32: the argument lists of ndcn_rhs_f32 / ndcn_rhs_rk_f32 plus the descriptor (NULL: exactly
 * those calls).  H <= 128 on the one-launch route: the factor is applied in the launch's epilogue (NDCN_PATH_DROP_EPI); every other
 * route runs its launch without a stage epilogue, ndcn_dropout_apply_f32 and the un-fused stage kernel.  NDCN_EINVAL: p outside
 * (0, 1), a halo panel, NDCN_F_RELU off.
 * ndcn_dropout_apply_f32: K[i] *= m(i) in place for i < n_elem (16 bytes per lane where K is 16-byte aligned; any n_elem).
 * ndcn_dropout_combine_f32 (ABI 29): that pass and the stage sum that consumes its result, in ONE pass -
 *   K[i] = K[i] * m(i), stored;  out[i] = y0[i] + (((0 + h_c[0] h_kprev[0][i]) + ...) + h_c[n_prev] K'[i])   (y0 NULL: the sum alone)
 * - the bits of ndcn_dropout_apply_f32(K) followed by ndcn_rk_combine_f32(out, y0, {h_kprev..., K}, h_c, n_prev + 1): (n_prev + 2)
 * panel reads and two writes instead of (n_prev + 3) and two launches.  n_prev = 0..5; the mask index is the position in K; 16-byte
 * lanes where every pointer is 16-byte aligned, scalar lanes otherwise; out, y0 and the h_kprev must not overlap K.  It is what
 * ndcn_rhs_rk_drop_f32 runs behind the launch in NDCN_RK_COMBINE mode (without y_aux) on every route that has no dropout epilogue:
 * the stage input of the masked derivative - dropout(...) of neural_dynamics.py:34 feeding y0 + sum_j dt beta_ij k_j of
 * rk_common.py:51.                                                                                                              */
typedef struct ndcn_dropout {
    float p;
    uint64_t seed;
    uint64_t evaluation;
} ndcn_dropout;
NDCN_API int ndcn_dropout_apply_f32(float *K, int64_t n_elem, const ndcn_dropout *desc, void *stream);
NDCN_API int ndcn_dropout_combine_f32(float *K, int64_t n_elem, const ndcn_dropout *desc, float *out, const float *y0,
                                      const float *const *h_kprev, const float *h_c, int n_prev, void *stream);
NDCN_API int ndcn_rhs_drop_f32(const ndcn_csr *A, const float *X, const float *X_halo, int64_t n_own,
                               const float *W, const float *b, float *Y, float *work, int H, uint32_t flags, void *stream,
                               const ndcn_dropout *desc);
NDCN_API int ndcn_rhs_rk_drop_f32(const ndcn_csr *A, const float *X, const float *X_halo, int64_t n_own,
                                  const float *W, const float *b, float *K, float *work, int H, uint32_t flags,
                                  int rk_mode, const float *y0, const float *const *h_kprev, const float *h_c, int n_prev,
                                  float *y_next, const float *y1, float *y_aux, const float *h_c_aux, float rtol, float atol,
                                  double *d_out, void *d_ws, void *stream, const ndcn_dropout *desc);

/* Pack rows `idx[0..n_idx)` of X into out (halo send buffers).  out[i, :] = X[idx[i], :] */
NDCN_API int ndcn_gather_rows_f32(const float *X, const int32_t *idx, int64_t n_idx, int H, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Runge-Kutta bookkeeping, one pass each (the reference issues one ATen op per term).
 * h_k: HOST array of n_k device pointers; h_c: HOST array of n_k fp32 coefficients ALREADY multiplied by
 * dt and rounded to fp32, as misc.py:25 `(scale * x)` does.  Terms are added left to right, products and
 * sums rounded separately (no FMA), exactly like `sum([...])` over tensors.
 */
/* out = y0 + sum_j c_j k_j          rk_common.py:51 via misc.py:22-25 ; dopri5.py:42 (y_mid).  y0 == NULL: sum_j c_j k_j alone
 * (the gradient combinations of a reverse sweep).                                                      */
NDCN_API int ndcn_rk_combine_f32(float *out, const float *y0, const float *const *h_k, const float *h_c, int n_k,
                        int64_t n_elem, void *stream);

/* err = sum_j c_j k_j ; tol = atol + rtol * max(|y0|, |y1|) ; r = err / tol
 * d_out[0] = sum r^2 (fp64, deterministic order), d_out[1] = number of non-finite elements of y1.
 * rk_common.py:60 + misc.py:146-157 + the finiteness assertion of the NEXT step (dopri5.py:101-102).
 * d_ws: device scratch of ndcn_reduce_ws_bytes() bytes.                                               */
NDCN_API int ndcn_rk_error_f32(const float *y0, const float *y1, const float *const *h_k, const float *h_c, int n_k,
                      float rtol, float atol, int64_t n_elem, double *d_out, void *d_ws, void *stream);

/* Reductions of ndcn_rk_error_f32 / ndcn_scaled_sumsq_f32 over at most this many elements reproduce ATen's SINGLE-THREAD float32
 * summation order (torch.mean / Tensor.norm: misc.py:71-76,156 - one workgroup, serial: the reference-sized solves, whose accept /
 * reject decisions hang on the last bit; above 32768 elements torch.sum depends on the size of its thread pool, and the threaded sum
 * is not reproduced by anything here); larger ones use the parallel fixed-order fp64 reduction.  Default 2^18 (environment NDCN_ATEN_NORM_MAX).
 * This call overrides the bound PROCESS-WIDE at run time (n_elem < 0: back to the default) and returns the previous override
 * (-1: none).  odeint_adjoint's fused reverse pass lowers it around its parameter-gradient vector (65 792 elements riding next
 * to 10^5..10^6-row panels: 0.6 ms serial against 10 us parallel).                                                               */
NDCN_API int64_t ndcn_set_aten_norm_max(int64_t n_elem);
/* The bound in effect (override, else environment, else 2^18; 0: no panel keeps ATen's order).  Added to ABI 29.                   */
NDCN_API int64_t ndcn_aten_norm_max(void);

/* ------------------------------------------------------------------------------------------------
 * One step of method 'adams' (VariableCoefficientAdamsBashforth, adams.py:62-170) as three passes (csrc/adams_vc.hip).  Added to
 * ABI 29: nothing existing changes.  With e_0 = phi_0 and e_j = fl(beta_j * phi_j) - the bits ndcn_scale_f32 writes; here they are
 * re-formed in registers and never stored - every result below is, bit for bit, what the composition of ndcn_scale_f32,
 * ndcn_rk_combine_f32 and ndcn_rk_error_f32 calls named next to it gives: products and sums rounded separately, left to right, the
 * first product of a sum added to +0; a difference a - b is a + (0 + (-1) * b) (combine with the single coefficient -1).
 * h_phi: HOST array of `order` device pointers phi_0 .. phi_{order-1} (newest first); h_beta: HOST array of `order` fp32 factors,
 * h_beta[0] is not read (adams.py:37-42).  16 bytes per lane where n_elem % 4 == 0 and every panel is 16-byte aligned, single
 * elements otherwise.  NDCN_EINVAL (text: ndcn_last_error): order outside 1..12, n_elem < 1, a null panel, an output that overlaps
 * an input or another output, scratch too small.  Nothing is launched then.
 */
/* p_next = y + ((0 + h_c[0] e_0) + h_c[1] e_1 + ... + h_c[m-1] e_{m-1}), m = max(1, order - 1); h_c[j] = fl(dt * g_j)  (adams.py:44-50).
 * = m - 1 ndcn_scale_f32 + ndcn_rk_combine_f32(p_next, y, {e_j}, h_c, m) - which takes m <= 8; this call takes every order.
 * Reads m + 1 panels, writes 1.                                                                                                */
NDCN_API int ndcn_adams_predict_f32(float *p_next, const float *y, const float *const *h_phi, const float *h_beta, const float *h_c,
                           int order, int64_t n_elem, void *stream);

/* The implicit phi of the predictor ip_0 = nf = f(p_next), ip_j = ip_{j-1} - e_{j-1}, j = 1 .. order (adams.py:53-59; `order`
 * ndcn_rk_combine_f32 calls), of which only the last three links are kept; y_next = p_next + (0 + c_corr * ip_{order-1}) (:129-132);
 * and up to four sums of squared error ratios r = (0 + coef * ip_q) / (atol + rtol * max(|y0|, |y_next|)) (misc.py:146-157):
 *   d_out4[0]: q = order,     h_coef4[0] = fl(dt * fl(g_order - g_{order-1}))       the step's error (:135-139)
 *   d_out4[1]: q = order - 1, h_coef4[1] = fl(dt * fl(g_{order-1} - g_{order-2}))   order selection, one lower (:154-157)
 *   d_out4[2]: q = order - 2, h_coef4[2] = fl(dt * fl(g_{order-2} - g_{order-3}))   order selection, two lower (needs order >= 2)
 *   d_out4[3]: q = order,     h_coef4[3] = fl(dt * GAMMA_STAR[order])               order selection, one higher (:161-165)
 * mask bit q enables sum q (a disabled sum costs nothing and reads 0).  Each enabled sum is the fp64 value ndcn_rk_error_f32(y0,
 * y_next, {ip_q}, {coef}, 1, ...) returns in d_out[0] ABOVE the ATen-order bound (ndcn_aten_norm_max) or below 8 elements: the same
 * element-to-thread map, grid, per-thread order, workgroup sum and finish.  This call never sums in ATen's order, whatever the size;
 * the non-finite count of y_next is not formed.  d_out4: four doubles on the device.  d_ws: device scratch, ws_bytes >=
 * ndcn_adams_correct_ws_bytes().  Reads order + 3 panels, writes 1.                                                             */
NDCN_API int ndcn_adams_correct_f32(float *y_next, const float *nf, const float *const *h_phi, const float *h_beta, int order,
                           const float *p_next, const float *y0, float c_corr, const float *h_coef4, uint32_t mask, float rtol,
                           float atol, int64_t n_elem, double *d_out4, void *d_ws, int64_t ws_bytes, void *stream);
NDCN_API int64_t ndcn_adams_correct_ws_bytes(void);

/* The implicit phi of an accepted step (adams.py:142 via :53-59): new_phi_0 = nf2 = f(y_next) is the caller's panel and is not
 * copied; h_new_phi[j] = new_phi_j = new_phi_{j-1} - e_{j-1} for j = 1 .. n_out - 1 (h_new_phi: HOST array of n_out device pointers,
 * entry 0 is not read).  1 <= n_out <= min(order + 1, 12); the solver keeps min(order + 1, max_order).  Out of place: the old phi
 * are read until the kernel is done.  = n_out - 1 ndcn_rk_combine_f32 calls.  Reads n_out panels, writes n_out - 1.             */
NDCN_API int ndcn_adams_update_f32(float *const *h_new_phi, const float *nf2, const float *const *h_phi, const float *h_beta,
                          int order, int n_out, int64_t n_elem, void *stream);

/* d_out[0] = sum ((a - b) / (atol + |y| * rtol))^2  (b nullable), d_out[1] = non-finite count of a.
 * The three RMS norms of misc.py:123-138 (d0, d1, d2).                                               */
NDCN_API int ndcn_scaled_sumsq_f32(const float *a, const float *b, const float *y, float rtol, float atol,
                          int64_t n_elem, double *d_out, void *d_ws, void *stream);
NDCN_API int64_t ndcn_reduce_ws_bytes(void);

/* Dense-output fit of an accepted dopri5 step: y_mid from the 7 stage derivatives, then the quartic's
 * a, b, c, d (e aliases y0).  h_cmid = dt * DPS_C_MID rounded to fp32; dt in the state dtype.
 * dopri5.py:39-45 + interp.py:21-35.                                                                 */
NDCN_API int ndcn_dopri5_interp_fit_f32(const float *y0, const float *y1, const float *const *h_k /*7*/,
                               const float *h_cmid /*7*/, float dt, float *a, float *b, float *c, float *d,
                               int64_t n_elem, void *stream);
/* Fit and evaluate in one pass without storing the coefficients (same arithmetic as the pair above): for a step
 * that is sampled at a single tick this reads 9 panels and writes 1 instead of 13 + 6.                  */
NDCN_API int ndcn_dopri5_interp_direct_f32(const float *y0, const float *y1, const float *const *h_k /*7*/,
                                           const float *h_cmid /*7*/, float dt, const float h_xpow[5], float *out,
                                           int64_t n_elem, void *stream);
/* out = a x^4 + b x^3 + c x^2 + d x + e with h_xpow = {x^4, x^3, x^2, x, 1} formed by the caller in fp32
 * (interp.py:59-65).                                                                                  */
NDCN_API int ndcn_interp_eval_f32(const float *a, const float *b, const float *c, const float *d, const float *e,
                         const float h_xpow[5], float *out, int64_t n_elem, void *stream);

/* Fixed-grid stage algebra with the reference's operator order (fixed_grid.py:8,18-19; rk_common.py:72-78).
 *   op 0  out = y + dt * k1                          euler update (y + dt*f)
 *   op 1  out = y + k1 * dt / 2                      midpoint stage
 *   op 2  out = y + dt * k1 / 3                      rk4 stage 2
 *   op 3  out = y + dt * (k1 / -3 + k2)              rk4 stage 3
 *   op 4  out = y + dt * (k1 - k2 + k3)              rk4 stage 4
 *   op 5  out = y + (k1 + 3 k2 + 3 k3 + k4) * (dt/8) rk4 update
 * unused k pointers may be NULL.  out may alias y.                                                     */
NDCN_API int ndcn_fixed_stage_f32(int op, float *out, const float *y, const float *k1, const float *k2,
                         const float *k3, const float *k4, float dt, int64_t n_elem, void *stream);

/* The ticks a step of a SUB-STEPPED fixed grid reports (options={'step_size': h}: solvers.py:55-68 builds the grid, :79-108 reports).
 * After the step [t0, t1] the reference hands out every tick t with t1 >= t - and, because it has overwritten y0 with y1 before
 * calling `_linear_interp` (:93-96), the "interpolated" value is
 *     out_q = y1 + ((y1 - y1) / (t1 - t0)) * (t_q - t0)            three roundings, no contraction
 * i.e. the state at the END of the step with -0.0 turned into +0.0 and Inf into NaN, while a tick that equals t1 (or t0) returns
 * y1 itself (:102-105): a plain copy.  One pass reads y once and writes <= 8 tick panels per launch (any n_ticks: a launch per 8).
 *   dt = t1 - t0, h_tick_dt[q] = t_q - t0 (HOST arrays, formed in the state dtype), h_coincident[q] != 0: plain copy,
 *   h_out: HOST array of n_ticks device panels, none of them y.
 * ndcn_fixed_stage_emit_f32: ndcn_fixed_stage_f32 op 0 or op 5 - the stage that ENDS a step - writing the new state to `out`
 * (may alias y) and the step's ticks in the same pass, so that an emitting step does not read y1 again.                      */
NDCN_API int ndcn_tick_emit_f32(const float *y, float dt, const float *h_tick_dt, const int *h_coincident, float *const *h_out,
                                int n_ticks, int64_t n_elem, void *stream);
NDCN_API int ndcn_fixed_stage_emit_f32(int op, float *out, const float *y, const float *k1, const float *k2, const float *k3,
                                       const float *k4, float dt, const float *h_tick_dt, const int *h_coincident,
                                       float *const *h_out, int n_ticks, int64_t n_elem, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Truth dynamics of the three drivers on an N x 1 state, O(nnz).
 *   heat   : ndcn_spmm_f32 with H = 1, alpha = -k on L                    heat_dynamics.py:197-204
 *   gene   : out = -b x^f + A (x^h / (x^h + 1))                           gene_dynamics.py:201-204
 *   mutual : out = b + x(1-x/k)(x/c-1) + sum_j A_ij x_i x_j/(d + e x_j + h x_i)   (the branch that
 *            executes for N x 1, mutualistic_dynamics.py:206-216)
 */
NDCN_API int ndcn_gene_rhs_f32(const ndcn_csr *A, const float *x, float *out, float b, float f, float h, void *stream);
NDCN_API int ndcn_mutual_rhs_f32(const ndcn_csr *A, const float *x, float *out, float b, float k, float c, float d,
                        float e, float h, void *stream);

/* The same three right-hand sides with the Runge-Kutta algebra that consumes K in the launch's epilogue: ndcn_rhs_rk_f32's
 * contract (rk_mode, y0, h_kprev, h_c, n_prev <= 5, y_next, y1, y_aux / h_c_aux, the error record) on an N x 1 state - the
 * launches of the device-resident truth solve (ndcn_solver_desc::dyn), exported so that they can be driven alone.
 *   dyn->kind  NDCN_DYN_HEAT: K = -p[0] (A x), A = L;  NDCN_DYN_GENE: p = {b, f, h};  NDCN_DYN_MUTUAL: p = {b, k, c, d, e, h}
 *   K          bit for bit what ndcn_spmm_f32 (H = 1, alpha = -p[0]) / ndcn_gene_rhs_f32 / ndcn_mutual_rhs_f32 write
 *   c_dev      (nullable) the coefficients in DEVICE memory instead of h_c (a replayed step reads fl(dt * c) from there; RK4: dt);
 *              not together with y_aux
 * Everything after K in the reference's operator order with contraction off, as ndcn_rhs_rk_f32.  d_ws: ndcn_reduce_ws_bytes(). */
#define NDCN_DYN_HEAT   0
#define NDCN_DYN_GENE   1
#define NDCN_DYN_MUTUAL 2
typedef struct ndcn_dynamics {
    int   kind;               /* NDCN_DYN_*                                                          */
    float p[6];               /* the kind's scalar parameters in the order above, the rest unused    */
} ndcn_dynamics;
NDCN_API int ndcn_dyn_rk_f32(const ndcn_dynamics *dyn, const ndcn_csr *A, const float *x, float *K, int rk_mode, const float *y0,
                             const float *const *h_kprev, const float *h_c, int n_prev, float *y_next, const float *y1,
                             float *y_aux, const float *h_c_aux, float rtol, float atol, double *d_out, void *d_ws,
                             const float *c_dev, void *stream);

/* Row-wise L1 normalisation: Y[r,:] = X[r,:] / max(sum_j |X[r,j]|, 1e-12), infinities zeroed.  Replaces
 * `row_normalization` / `RowNorm.forward` (ode_gcn.py:9-26; used by ResBlock(normalize=True) ode_gcn.py:50-57 and the
 * odeGCN input stack dgnn.py:152).  Y may alias X.                                                                   */
NDCN_API int ndcn_row_l1_normalize_f32(const float *X, float *Y, int64_t n_rows, int H, void *stream);
/* Its vector-Jacobian product (training through ResBlock(normalize=True), ode_gcn.py:50-57): GX = dL/dX given G = dL/dY
 * and the forward input X.  GX may alias G.                                                                            */
NDCN_API int ndcn_row_l1_normalize_bwd_f32(const float *G, const float *X, float *GX, int64_t n_rows, int H, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU transport (ndcn_halo_plan_create / exchange; 8e).  The path shards by node range, one rank per
 * GPU: rank r owns rows [b_r, b_{r+1}) of the operator and of every panel; per right-hand side the X rows of remote
 * column neighbours ("halo") arrive by ONE all-to-all-v - a grouped ncclSend / ncclRecv per peer over RCCL / xGMI, only
 * the referenced rows travel - and the controller's 16-byte record is all-reduced.  The reference is single-device
 * (SURVEY 8e); these calls are what its `A x` (neural_dynamics.py:29) and `torch.mean` / `norm` (misc.py:71-76,156)
 * become when the node set is split.  librccl is bound at first use (dlopen): without it these calls return NDCN_EHIP. */
typedef struct ndcn_comm ndcn_comm;
typedef struct ndcn_halo_plan ndcn_halo_plan;
/* rank 0: a 128-byte id to hand to every rank (over the caller's own channel), then every rank: create on its device */
NDCN_API int ndcn_comm_unique_id(char h_id[128]);
NDCN_API int ndcn_comm_create(const char h_id[128], int world, int rank, ndcn_comm **out);
/* or adopt the caller's ncclComm_t (passed as void*; not destroyed by ndcn_comm_destroy) */
NDCN_API int ndcn_comm_adopt(void *nccl_comm, int world, int rank, ndcn_comm **out);
/* TEST transport: the same communicator interface over POSIX shared memory, host-staged and synchronous (csrc/comm.hip) - ranks
 * that share ONE device (RCCL refuses those) or have no RCCL at all can run every multi-rank entry point of this header, the
 * device-resident sharded solver included.  `name`: the same string on every rank, unique per communicator (<= 99 characters,
 * no '/'); world <= 64.  Collective: returns when every rank has joined (120 s bound).  Never the production path.               */
NDCN_API int ndcn_comm_create_loopback(const char *name, int world, int rank, ndcn_comm **out);
NDCN_API int ndcn_comm_destroy(ndcn_comm *c);
/* d_buf[0..n) <- sum over ranks (in place, enqueued on `stream`; a no-op for world 1) */
NDCN_API int ndcn_comm_allreduce_sum_f64(ndcn_comm *c, double *d_buf, int n, void *stream);
/* h_send_counts / h_recv_counts: HOST arrays [world] of ROW counts per peer (a rank may list itself: rows routed through
 * the exchange to itself); d_send_idx: DEVICE int32 rows of the own panel to pack, grouped by peer in rank order
 * (sum of send counts entries; must outlive the plan); the halo panel receives peer 0's rows first, then peer 1's ...
 * (sum of receive counts == n_halo).  any_rank_moves_rows: the caller's GLOBAL fact (an all-reduce at plan time) - the
 * exchange is skipped only when no rank sends or receives, never on a rank-local test.                                */
NDCN_API int ndcn_halo_plan_create(ndcn_comm *c, int64_t n_halo, const int64_t *h_send_counts, const int64_t *h_recv_counts,
                                   const int32_t *d_send_idx, int any_rank_moves_rows, ndcn_halo_plan **out);
NDCN_API int ndcn_halo_plan_destroy(ndcn_halo_plan *p);
/* X_halo[n_halo, H] <- the rows of the peers' panels this rank references; d_pack: scratch of (sum of send counts) * H floats */
NDCN_API int ndcn_halo_exchange_f32(ndcn_halo_plan *p, const float *X, int H, float *d_pack, float *X_halo, void *stream);

/* How one rank's shard is evaluated by the device-resident solver (ndcn_solver_desc::shard).  desc.A is then an operator
 * over the columns [own | halo] (n_cols = n_own + n_halo).  Three forms, all with the exchange on a side stream:
 *   row split  (n_blocks > 0)  the shard's rows in up to 4 contiguous blocks; blocks with needs_halo == 0 (operator over
 *              the own columns only) run while the halo is in flight, the others after it has landed.  Lattices: one long
 *              interior block between two thin boundary bands.  desc.A is unused.
 *   two-phase  (A_own.n_rows > 0)  S = A_own X during the exchange, then desc.A = [I | A_halo] over the panels
 *              [S | X_halo] (the same fma sequence per row as one launch).  Scattered halos: small-world, power-law shards.
 *   one launch (neither)       desc.A over [X | X_halo] after the exchange.
 * n_global_rows: the node count of the whole graph (means and RMS norms of the controller are global).               */
typedef struct ndcn_shard {
    ndcn_comm      *comm;
    ndcn_halo_plan *halo;
    int64_t         n_global_rows;
    int32_t         n_blocks;
    struct { int64_t row_lo, row_hi; int32_t needs_halo; ndcn_csr A; } blocks[4];
    ndcn_csr        A_own;
    float          *X_halo;       /* nullable: where the halo rows land (n_halo x H floats).  An operator with a long-row
                                     plan wants them directly in front of its hub rows (struct ndcn_csr: hub_S == X_halo +
                                     n_halo * H); NULL: inside the solver's workspace                                    */
} ndcn_shard;

/* ------------------------------------------------------------------------------------------------
 * Device-resident integrator for the ODEFunc RHS (state, stage derivatives and dense-output coefficients
 * stay in HBM across steps; the host only reads the 16-byte error record per adaptive step).
 * Mirrors the reference's per-call solver object (odeint.py:71-72; dopri5.py:58-122; solvers.py:79-99).
 *
 * The solver lives in ONE device workspace of ndcn_solver_workspace_bytes(desc) bytes (256-byte aligned):
 * pass the caller's (e.g. a torch allocation, so repeated solves reuse cached memory) or NULL to let
 * ndcn_solver_create hipMalloc it (that synchronises; ndcn_solver_destroy frees it).  All other calls only
 * enqueue work on `stream`, except that the dopri5 controller waits for each step's 16-byte error record.
 */
typedef struct ndcn_solver ndcn_solver;

typedef struct ndcn_solver_desc {
    int      method;          /* NDCN_M_*                                                            */
    int      H;
    uint32_t rhs_flags;       /* NDCN_F_RELU | NO_GRAPH | NO_CONTROL                                  */
    int      use_graph;       /* fixed-grid methods: replay one captured hipGraph per step            */
    ndcn_csr A;
    const float *W, *b;       /* nullable under NO_CONTROL                                            */
    double   rtol, atol;      /* dopri5                                                               */
    int64_t  max_num_steps;   /* dopri5.py:61 (2^31-1 in the reference)                               */
    double   safety, ifactor, dfactor;   /* dopri5 step-size controller (dopri5.py:60,72-74; misc.py:160-170); the
                                            reference's defaults pass through a float32 tensor: (double)0.9f, 10, (double)0.2f.
                                            Values <= 0 select those defaults.                                  */
    const ndcn_shard *shard;  /* NULL: the whole graph on this device.  Otherwise this rank's shard of a node-range
                                 sharded graph: A.n_rows = own rows, A.n_cols = own + halo columns (see ndcn_shard) */
    const ndcn_dynamics *dyn; /* NULL: the ODEFunc right-hand side above.  Otherwise one of the drivers' ground-truth dynamics on
                                 an N x 1 state (ndcn_dyn_rk_f32; read at ndcn_solver_create): H must be 1 and shard NULL; W, b
                                 and rhs_flags are ignored; A is L for heat, the adjacency for gene and mutual               */
} ndcn_solver_desc;

NDCN_API int64_t ndcn_solver_workspace_bytes(const ndcn_solver_desc *desc);
NDCN_API int ndcn_solver_create(const ndcn_solver_desc *desc, void *workspace, int64_t workspace_bytes,
                                ndcn_solver **out);
NDCN_API int ndcn_solver_destroy(ndcn_solver *s);
/* Start at (t0, y0): copies y0 in; dopri5 also evaluates f0 and the initial step (dopri5.py:77-83).   */
NDCN_API int ndcn_solver_begin(ndcn_solver *s, const float *y0, double t0, void *stream);
/* As ndcn_solver_begin, without the copy (dopri5; other methods and replay mode copy as above): the solver reads the
 * initial state where it lies - odeint.py:39-41 hands y0 over and never writes it - until its second accepted step.
 * y0 must stay valid and unchanged until the next ndcn_solver_begin* / ndcn_solver_destroy on `s`, and no `out` of
 * ndcn_solver_advance / _advance_many may overlap it (refused with NDCN_EINVAL).                       */
NDCN_API int ndcn_solver_begin_borrowed(ndcn_solver *s, const float *y0, double t0, void *stream);
/* Integrate to next_t and write y(next_t) to `out` (n_rows x H).
 * fixed grid: ONE step of size next_t - t (solvers.py:89-97).
 * dopri5: adaptive steps until t1 >= next_t, at most `step_budget` of them (<= 0: unlimited), then the
 * dense-output evaluation (dopri5.py:85-92).  When the budget is exhausted first, returns 1 and leaves
 * `out` untouched; call again to continue.                                                            */
NDCN_API int ndcn_solver_advance(ndcn_solver *s, double next_t, float *out, int64_t step_budget, void *stream);
/* All of h_ticks (HOST array, increasing, the first one > the current time) in one call: out[i] = y(h_ticks[i]), n_ticks
 * panels back to back.  dopri5: ticks that fall into the same accepted step are evaluated together, reading the step's
 * panels once per <= 8 ticks instead of once per tick (the reference's drivers sample 16-120 ticks over a handful of
 * steps: heat_dynamics.py:35,123; dgnn.py:173-182); same arithmetic per element as ndcn_solver_advance.  Fixed grid:
 * one step per tick.                                                                                     */
NDCN_API int ndcn_solver_advance_many(ndcn_solver *s, const double *h_ticks, int64_t n_ticks, float *out, void *stream);
/* Inference: ndcn_solver_advance_many with the decoder Linear(H, C) of neural_dynamics.py:148-160 applied to every tick as it is
 * produced, so that the hidden trajectory (n_ticks x n_rows x H) is never stored: out[i] (n_rows x C, panels back to back) =
 * Wd y(h_ticks[i]) + bd with Wd [C][H] row-major and bd [C] nullable - bit for bit ndcn_linear_f32 of the panel
 * ndcn_solver_advance_many writes there.  The steps, their launches and the accept / reject log are ndcn_solver_advance_many's.
 *   dopri5      the ticks of a fresh accepted step are evaluated AND decoded in one pass over the step's panels (<= 8 per launch: a
 *               wave per row holds the fitted row in registers and dots it with Wd in the lane order of the decoder's row-dot
 *               kernel; H < 64, where the decoder runs one in-order fma chain per (row, output): a workgroup per tile of 64 rows
 *               evaluates each tick into LDS and runs those chains from there); the single-tick paths (a stored fit, a tick without
 *               a fresh step) evaluate into `scratch` first
 *   fixed grid  one step per tick with the state inside the solver (Euler whose update rides in the right-hand side's epilogue
 *               alternates between the solver's panel and `scratch`), each new state decoded by ndcn_linear_f32
 *   scratch     caller-owned device memory, room for two n_rows x H panels (the staged ticks and the Euler alternation use the
 *               first; the second is reserved); free after the call
 * Declines with NDCN_EINVAL: a sharded solver; H neither in 64..512 (the decoder's row-dot route) nor one of 16, 20, .. 60 (its small
 * route at the widths of the one-launch right-hand side), or C outside 1..15; a fixed-grid
 * solve that ndcn_solve_small_supported would run as one launch (states of at most 1 MB: decode that trajectory instead).  The
 * step_size grid has no such form: ndcn_solver_advance_grid writes hidden ticks.  These are decided before anything else, so a call
 * with n_ticks = 0 (valid before ndcn_solver_begin, touches nothing) asks whether the solver would decline.
 * ndcn_last_readout_path: what the last call on this thread ran (cleared on its entry, so 0 after a call that declined);
 * ndcn_clear_readout_path zeroes it - for callers that decide above the library whether to call at all.                       */
#define NDCN_READOUT_FUSED   1      /* the fused dense-output kernel ran (interp_readout_kernel<ceil(H / 64)>)                       */
#define NDCN_READOUT_STAGED  2      /* a dopri5 tick was evaluated into `scratch` and decoded from there                            */
#define NDCN_READOUT_FIXED   4      /* fixed grid: the state decoded after each step                                                */
#define NDCN_READOUT_NARROW  8      /* beside FUSED: H < 64, the 64-row tile kernel (readout_narrow_kernel<ceil(H / 16)>)           */
/* (set by the ndcn_solve_*_adams_readout_f32 calls below, which also set FIXED for their staged decodes and NARROW beside ADAMS)  */
#define NDCN_READOUT_ADAMS   (1 << 4)   /* = 16: the fused Adams-Bashforth step + decode kernel ran (ndcn_ab_step_readout_f32)            */
NDCN_API int ndcn_solver_advance_many_readout(ndcn_solver *s, const double *h_ticks, int64_t n_ticks, const float *Wd, const float *bd,
                                              int C, float *out, float *scratch, void *stream);
NDCN_API int ndcn_last_readout_path(void);
NDCN_API void ndcn_clear_readout_path(void);
/* Fixed grid only (NDCN_EINVAL for dopri5 and for a sharded solver): FixedGridODESolver.integrate with the step_size option
 * (solvers.py:55-68,79-108) from the solver's current time.  h_grid (HOST, fp32, n_grid points, h_grid[0] = the current time in the
 * state dtype) is the solver's own grid; every one of its n_grid - 1 steps runs with the state INSIDE the solver - eager: the launches
 * of ndcn_solver_advance; replay mode: one replay of the captured step per grid step, its size through the pinned ring - and tick j
 * (h_tick_time[j], fp32; h_tick_step non-decreasing) is written to out[j] after step h_tick_step[j]: as the new state itself when
 * the tick equals an end of that step, else through the expression of ndcn_tick_emit_f32.  Device memory: the workspace plus the
 * n_ticks output panels, whatever n_grid is.  States that fit one compute unit run as one launch per 128 steps
 * (ndcn_solve_small_grid_f32).  Bit-identical to ndcn_solver_advance_many over all of h_grid, taken at the emitting steps.        */
NDCN_API int ndcn_solver_advance_grid(ndcn_solver *s, const float *h_grid, int64_t n_grid, const int64_t *h_tick_step,
                                      const float *h_tick_time, int64_t n_ticks, float *out, void *stream);
/* h_stats = {steps attempted, steps accepted, rhs evaluations, t1, dt_next, last mean_sq_error_ratio} */
NDCN_API int ndcn_solver_stats(const ndcn_solver *s, double h_stats[6]);
/* Copies up to `cap` rows {t0, dt, accepted, ratio, dt_next} of the per-attempt log; returns the count. */
NDCN_API int64_t ndcn_solver_steplog(const ndcn_solver *s, double *h_rows, int64_t cap);

/* ------------------------------------------------------------------------------------------------
 * A WHOLE fixed-grid solve in one launch, for states that fit one compute unit: FixedGridODESolver.integrate (solvers.py:79-99)
 * with Euler / midpoint / RK4-3/8 steps (fixed_grid.py:7-29, rk_common.py:72-78) over ODEFunc (neural_dynamics.py:27-36) - the
 * reference's own commands (heat_dynamics.py:20-22,33: Euler, H = 20, 400 nodes, 80-120 ticks), where a launch per step is
 * pure latency.  One workgroup keeps the stage input in LDS and the row-local panels in registers across all steps; every tick
 * is bit-identical to the per-step kernels.  ndcn_solver_advance_many takes this path by itself; the entry points are
 * public for callers that own their time loop and for the reverse sweep:
 *   h_dt      HOST array of the n_ticks step sizes, formed in the state dtype (solvers.py:81-84: t[i+1] - t[i] in fp32)
 *   out       n_ticks panels, out[i] = y(t[i+1])
 *   backward  (Euler; the drivers train by backprop through the solver, heat_dynamics.py:313-334): traj / g_out hold
 *             n_ticks + 1 panels - y(t[0]) .. y(t[n_ticks]), i.e. y0 followed by the forward's `out`, and dL/dy of each -
 *             g_y0 [n][H], g_W [H][H], g_b [H] receive the gradients (A_t: the operator's transpose as CSR).
 * supported: H <= 64 (backward: H <= 31), a plain operator (no halo), the state (backward: 4 panels) within 160 KB of LDS and
 * <= 576 * 20 / H rows; NDCN_EINVAL otherwise (ask ndcn_solve_small_supported first).                                      */
NDCN_API int ndcn_solve_small_supported(const ndcn_csr *A, int H, uint32_t flags, int method, int backward);
NDCN_API int ndcn_solve_small_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, int method,
                                  const float *y0, const float *h_dt, int64_t n_ticks, float *out, void *stream);
NDCN_API int ndcn_solve_small_bwd_f32(const ndcn_csr *A, const ndcn_csr *A_t, const float *W, const float *b, int H, uint32_t flags,
                                      int method, const float *traj, const float *g_out, const float *h_dt, int64_t n_ticks,
                                      float *g_y0, float *g_W, float *g_b, void *stream);
/* The one-launch solve on a grid finer than the ticks (the step_size option, solvers.py:55-68,79-108): n_steps steps of sizes h_dt,
 * still ONE launch per 128 steps, and only the ticks are written: tick j goes to out[j] after step h_tick_step[j] (HOST, non-
 * decreasing) - the new state as it is when h_tick_same[j] != 0 (the tick is an end of the step; only the LAST tick of a step can
 * be), else y1 + ((y1 - y1) / dt) * (t_j - t0) (ndcn_tick_emit_f32; its value does not depend on 0 < t_j - t0).  y_end (device,
 * one panel, NULL allowed while n_steps <= 128) receives the state after the last step.  Same support as the plain solve
 * (ndcn_solve_small_grid_supported); every emitted state is bit-identical to ndcn_solve_small_f32 on the same step sizes.          */
NDCN_API int ndcn_solve_small_grid_supported(const ndcn_csr *A, int H, uint32_t flags, int method);
NDCN_API int ndcn_solve_small_grid_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, int method,
                                       const float *y0, const float *h_dt, int64_t n_steps, const int64_t *h_tick_step,
                                       const int *h_tick_same, int64_t n_ticks, float *out, float *y_end, void *stream);
/* Euler training with the evaluations' intermediates KEPT (the README commands' shape: H = 16 / 20, a symmetric operator whose view has
 * max_row_len and symmetric filled - ndcn_solve_small_keep_supported says whether both launches take the form): the forward launch also
 * writes, per step, S_i = A y_i and K_i = f(y_i) into `keep` (n_ticks x 2 panels); the reverse sweep reads them instead of re-forming
 * them from y_i - no gather and no Linear per tick (a third of the sweep's cycles).  Same results as the pair above.                  */
NDCN_API int ndcn_solve_small_keep_supported(const ndcn_csr *A, int H, uint32_t flags);
NDCN_API int ndcn_solve_small_keep_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0,
                                       const float *h_dt, int64_t n_ticks, float *out, float *keep, void *stream);
NDCN_API int ndcn_solve_small_bwd_keep_f32(const ndcn_csr *A, const ndcn_csr *A_t, const float *W, const float *b, int H, uint32_t flags,
                                           const float *traj, const float *g_out, const float *h_dt, int64_t n_ticks, const float *keep,
                                           float *g_y0, float *g_W, float *g_b, void *stream);
/* Which instantiation the LAST launch of the ndcn_solve_small_* entry points of this PROCESS ran (a reverse sweep runs on autograd's
 * thread; tests: every template instantiation
 * of csrc/solve_small.hip is reached on purpose; an addition to ABI 29, nothing existing changes).  The word is formed from the
 * template arguments of the kernel that was launched; 0 before the first launch:
 *   direction | family | MAXIT << 4 | CSR_LDS | HT << 9 | KEEP | GRID | SYMMETRIC | method << 17
 * MAXIT: the passes the register arrays hold (4, 9 or 12).  CSR_LDS: the CSR arrays were copied into LDS (forward fast kernels
 * instantiate it set - their ELL image lives there; the fast reverse kernel has no such parameter: clear).  HT: the compile-time
 * width of the fast kernels (16 / 20), 0 on the generic ones.  SYMMETRIC (reverse only): the transposed gather read A's own
 * arrays (generic / rk: the `symmetric` argument; fast: always).  method: NDCN_M_*.                                              */
#define NDCN_SSR_FWD       1
#define NDCN_SSR_BWD       2
#define NDCN_SSR_GENERIC   4        /* solve_small_kernel<.., HT = 0> / solve_small_bwd_kernel                                       */
#define NDCN_SSR_FAST      8        /* solve_small_kernel<.., HT = 16 | 20> / solve_small_bwd_fast_kernel                            */
#define NDCN_SSR_RK        12       /* solve_small_bwd_rk_kernel (midpoint / RK4 reverse)                                            */
#define NDCN_SSR_MAXIT_SHIFT 4
#define NDCN_SSR_CSR_LDS   256
#define NDCN_SSR_HT_SHIFT  9
#define NDCN_SSR_KEEP      (1 << 14)
#define NDCN_SSR_GRID      (1 << 15)
#define NDCN_SSR_SYMMETRIC (1 << 16)
#define NDCN_SSR_METHOD_SHIFT 17
NDCN_API int ndcn_debug_last_small_route(void);

/* ------------------------------------------------------------------------------------------------
 * explicit_adams: the reference's AdamsBashforth (torchdiffeq/_impl/fixed_adams.py:151-211), a fixed-grid linear multistep method - two
 * RK4 (3/8 rule) steps, then ONE right-hand side per step combined with up to ten earlier ones.  Three calls added to ABI 29: no existing
 * declaration changes.
 * ndcn_ab_step_f32, one step of order n (fixed_adams.py:180-182, misc.py:22-25, solvers.py:92):
 *     out = y + dt * ((((0 + a[0] f[0]) + a[1] f[1]) + ...) + a[n-1] f[n-1])
 *   every product and every sum rounded to fp32 on its own, no contraction; the sum starts from an exact zero (Python's sum()), so a
 *   lone -0 product becomes +0.  h_f: HOST array of the n newest evaluations, newest first (device panels of n_elem floats); h_a: HOST
 *   array of their weights, float32((1 / div) * c_i) with the product taken in double.  3 <= n <= 11; NDCN_EINVAL - before any launch -
 *   for any other n, a null panel, or `out` equal to one of the f panels (out == y is allowed).  Any pointer alignment and any
 *   n_elem >= 0: where all panels share one offset from a 16-byte boundary the body runs by 16 bytes per lane behind a head of <= 3
 *   single elements, else by single elements.  One streaming launch on a grid sized from the compute-unit count; the history panels are
 *   read with the default cache policy (ten of them are read again by the next step).
 * ndcn_solve_explicit_adams_f32: FixedGridODESolver.integrate (solvers.py:79-99) with that step over ODEFunc, enqueued on `stream`
 *   without a read-back or a synchronisation:
 *     h_dt [n_steps]        the grid's differences in the state dtype (solvers.py:91)
 *     tick j < n_ticks      written to out[j] (panels back to back) after step h_tick_step[j] (HOST, non-decreasing, < n_steps): the new
 *                           state itself where h_tick_same[j] != 0 (the tick is an end of the step), else through the expression of
 *                           ndcn_tick_emit_f32 with h_tick_off[j] = t_j - t0 of that step (fp32)
 *     max_order             fixed_adams.py:162-163 after its clamp: 2 .. 12; the history keeps max_order - 1 evaluations and a step has
 *                           order min(evaluations so far, max_order - 1): below 3 it is the RK4 step with the new evaluation as k1 - the
 *                           launches of ndcn_solver_advance's un-fused RK4 step (ndcn_rhs_f32, ndcn_fixed_stage_f32 ops 2..5: its bits) -
 *                           else ONE ndcn_rhs_f32 written into the history slot of the oldest evaluation and ONE ndcn_ab_step_f32
 *     workspace             ndcn_explicit_adams_workspace_bytes(n_rows, H, max_order) bytes, 256-byte aligned, owned by the caller: the
 *                           history ring (max_order - 1 panels), three RK4 stage panels, a stage input, two state panels and the scratch of
 *                           ndcn_rhs_f32 (H = 256: the weights are packed there once per solve)
 *   Un-sharded, no dropout, flags == NDCN_F_RELU: NDCN_EINVAL (with a message) otherwise.  y0 is only read and may be the panel in
 *   front of `out`.  The weights of each order are derived in the library from the exact rationals
 *   beta_i = integral_0^1 prod_{j != i} (u + j) / (j - i) du over their least common denominator.                                   */
NDCN_API int ndcn_ab_step_f32(float *out, const float *y, const float *const *h_f, const float *h_a, int n, float dt, int64_t n_elem,
                              void *stream);
NDCN_API int64_t ndcn_explicit_adams_workspace_bytes(int64_t n_rows, int H, int max_order);
NDCN_API int ndcn_solve_explicit_adams_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0,
                                           const float *h_dt, int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same,
                                           const float *h_tick_off, int64_t n_ticks, int max_order, float *out, void *workspace,
                                           int64_t workspace_bytes, void *stream);
/* explicit_adams under a gradient (three more calls added to ABI 29: no existing declaration changes).
 * ndcn_explicit_adams_train_f32: ndcn_solve_explicit_adams_f32 - the same loop, launches, arguments, checks and bits in `out` - that KEEPS
 *   what a reverse sweep needs in a record the caller owns, in place of the history ring and the two state panels:
 *     rec_f [n_steps panels]   f_i, the evaluation grid step i starts with (a step's history is read from the panels i, i - 1, ...)
 *     rec_y [n_steps panels]   the state after step i (panels of n_rows * H floats back to back, as `out`)
 *   rec_y may be `out` itself when every step reports exactly one tick and that tick is an end of its step (the default grid: tick j
 *   after step j): the state is then stored once.  Neither record may overlap y0.
 *     workspace                ndcn_explicit_adams_train_workspace_bytes(n_rows, H) bytes, 256-byte aligned: three RK4 stage panels, the
 *                              stage input and the scratch of ndcn_rhs_f32, nothing else - a host function of its own rather than the
 *                              solve's formula at max_order = 2, which would add a ring panel and two state panels that are never touched
 * ndcn_ab_adjoint_f32, the gradient of one evaluation gathered from the adjoints of the <= 11 Adams-Bashforth steps that used it:
 *     out = [base +] ((((0 + c[0] g[0]) + c[1] g[1]) + ...) + c[n-1] g[n-1])
 *   every product and every sum rounded to fp32 on its own, no contraction, the sum started from an exact zero and the base added
 *   last.  h_g: HOST array of n device panels of n_elem floats, h_c: HOST array of their coefficients (fl32(dt * a), formed by the
 *   caller); base nullable.  1 <= n <= 11; NDCN_EINVAL - before any launch - for any other n, a null term, or `out` equal to one of the
 *   g panels (out == base is allowed).  Any alignment and any n_elem >= 0 (0: nothing is launched), the lanes of ndcn_ab_step_f32: 16
 *   bytes each where all panels share one offset from a 16-byte boundary, behind a head of <= 3 single elements, else single elements.
 *   It is not ndcn_ab_step_f32 with dt = 1: that call needs a state, starts at three terms and rounds dt * sum.                        */
NDCN_API int ndcn_ab_adjoint_f32(float *out, const float *base, const float *const *h_g, const float *h_c, int n, int64_t n_elem,
                                 void *stream);
NDCN_API int64_t ndcn_explicit_adams_train_workspace_bytes(int64_t n_rows, int H);
NDCN_API int ndcn_explicit_adams_train_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0,
                                           const float *h_dt, int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same,
                                           const float *h_tick_off, int64_t n_ticks, int max_order, float *out, float *rec_f,
                                           float *rec_y, void *workspace, int64_t workspace_bytes, void *stream);

/* fixed_adams: the reference's AdamsBashforthMoulton (torchdiffeq/_impl/fixed_adams.py:151-205) - explicit_adams' predictor corrected
 * by the Adams-Moulton formula over the same history, the corrector iterated until every element of the step's increment has settled.
 * Four calls added to ABI 29: no existing declaration changes.
 * ndcn_abm_predict_f32, the predictor and the explicit part of the corrector of a step that holds n evaluations (:180-188):
 *     dy    = dt * ((((0 + a[0] f[0]) + a[1] f[1]) + ...) + a[n-1] f[n-1])       a: the Adams-Bashforth weights of order n
 *     delta = dt * ((((0 + m[0] f[0]) + m[1] f[1]) + ...) + m[n-1] f[n-1])       m: the Adams-Moulton weights of the formula over the
 *     u     = y + dy                                                             n + 1 points t + dt, t, .. WITHOUT its leading one
 *   in ONE streaming pass over y and the history (the reference reads it twice), with the rounding, the argument conventions (h_f, h_a,
 *   h_m: HOST arrays), the lanes and the grid of ndcn_ab_step_f32.  3 <= n <= 11; NDCN_EINVAL - before any launch - for any other n, a
 *   null panel, an output that is a history panel, or outputs that alias each other or y (u == y alone is allowed).
 * ndcn_abm_correct_f32, one corrector iteration (:192-194, misc.py:33-37) on the evaluation f = func(t + dt, u):
 *     dy <- c0 * f + delta  (in place),   u = y + dy,   c0 = fl32(dt) * fl32(m_0 / div) formed by the caller
 *     *d_count = the number of elements for which  |dy_old - dy_new| < atol + rtol * max(|dy_old|, |dy_new|)  does NOT hold
 *   - float32 throughout, a strict `<`: err == tol fails, a NaN fails, rtol = atol = 0 fails everywhere.  d_count: a DEVICE uint64,
 *   8-byte aligned, zeroed by the call on `stream`; every workgroup counts in integers and adds its count with one integer atomic, so the
 *   result does not depend on the order of the workgroups.  The caller reads it back (8 bytes) to decide whether to iterate again.  u is
 *   the next iterate and, after the last iteration, the new state y1 (solvers.py:92).  NDCN_EINVAL before any launch for a null panel or
 *   u / dy overlapping an input.  Any alignment, any n_elem >= 0 (0: the counter is zeroed, nothing is launched).
 * ndcn_solve_fixed_adams_f32: ndcn_solve_explicit_adams_f32 - the same arguments, restrictions (plain ODEFunc, flags == NDCN_F_RELU,
 *   un-sharded, no dropout), history ring, warm-up launches and tick handling - with the corrector:
 *     rtol, atol, max_iters    of the convergence test (float32, as the reference forms them on the state dtype); max_iters >= 1
 *     h_iters [n_steps]        HOST, written: corrector iterations run by grid step i (0: an RK4 warm-up step)
 *     h_converged [n_steps]    HOST, written: 1 where step i converged (warm-up steps: 1), 0 where it ran max_iters iterations without
 *   UNLIKE the explicit solve this one is not enqueued blindly: every corrector iteration ends with ONE 8-byte read-back of the counter
 *   and a synchronisation of `stream`, because the HOST decides whether to iterate again and - a step that did not converge drops the
 *   OLDEST evaluation of its history (:199) - how long the ring is for the next step.  The evaluation of the corrector never enters the
 *   history.  The caller prints the reference's warning line (:198) for every step with h_converged[i] == 0.
 *     workspace                ndcn_fixed_adams_workspace_bytes(n_rows, H, max_order) bytes, 256-byte aligned: the explicit solve's panels,
 *                              three more (dy, delta, the corrector's evaluation) and the counter
 *   The Moulton weights of each order are derived in the library in 64-bit integers from the exact rationals
 *   mu_i = integral_0^1 prod_{j != i} (u + j - 1) / (j - i) du over their least common denominator, as the Bashforth ones are.          */
NDCN_API int ndcn_abm_predict_f32(float *dy, float *delta, float *u, const float *y, const float *const *h_f, const float *h_a,
                                  const float *h_m, int n, float dt, int64_t n_elem, void *stream);
NDCN_API int ndcn_abm_correct_f32(float *dy, float *u, const float *f, const float *delta, const float *y, float c0, float rtol, float atol,
                                  int64_t n_elem, uint64_t *d_count, void *stream);
NDCN_API int64_t ndcn_fixed_adams_workspace_bytes(int64_t n_rows, int H, int max_order);
NDCN_API int ndcn_solve_fixed_adams_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0,
                                        const float *h_dt, int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same,
                                        const float *h_tick_off, int64_t n_ticks, int max_order, float rtol, float atol, int max_iters,
                                        float *out, int *h_iters, int *h_converged, void *workspace, int64_t workspace_bytes, void *stream);
/* The two multistep solves with the decoder Linear(H, C) inside (inference: neural_dynamics.py:148-160 decodes every tick, and the
 * (n_ticks, n_rows, H) trajectory is the largest allocation of such a pass).  Three calls added to ABI 29: no existing declaration
 * changes, the existing calls keep their launches and bits.
 * ndcn_ab_step_readout_f32: ndcn_ab_step_f32 on a panel of n_rows x H - the same arithmetic, `out` bit for bit - that ALSO writes
 *     dec [n_rows][C] = Wd * s + bd,   s = the new state (emit_off == 0) or s = state + ((state - state) / dt) * emit_off
 *   (emit_off != 0: a tick strictly inside the step, the expression of ndcn_tick_emit_f32: -0 becomes +0, Inf becomes NaN; the state
 *   that is STORED is never transformed) in the same pass, bit for bit ndcn_linear_f32 of that panel: Wd [C][H] and bd [C] (nullable)
 *   in device memory.  64 <= H <= 512: a wave per row, the fma chain / butterfly / bias of the decoder's row-dot route; H = 16, 20,
 *   .. 60: a workgroup per tile of 64 rows staged in LDS, one in-order fma chain per (row, output) as its small route.  NDCN_EINVAL -
 *   before any launch - for C outside 1..15, any other H, n outside 3..11, a null panel, `out` equal to a history panel, `dec` equal to
 *   `out` or y (out == y is allowed).  Any pointer alignment (H < 64: 16-byte loads where every panel is 16-byte aligned).
 * ndcn_solve_explicit_adams_readout_f32 / ndcn_solve_fixed_adams_readout_f32: ndcn_solve_explicit_adams_f32 / ndcn_solve_fixed_adams_f32
 *   - the same arguments, checks, loop, launches, read-backs, h_iters / h_converged and workspace - with Wd, bd, C of the decoder (H and C
 *   as above, NDCN_EINVAL otherwise) and
 *     out                    n_ticks panels of n_rows x C: out[j] = Wd * tick_j + bd, bit for bit ndcn_linear_f32 of the tick panel the
 *                            un-decoded solve writes.  No hidden tick is written: the state alternates between the workspace's two panels.
 *   explicit_adams at order >= 3: a step that reports ticks runs ndcn_ab_step_readout_f32's kernel (its first 8 ticks in one launch), a
 *   step that reports none ndcn_ab_step_f32.  RK4 warm-up steps and every step of fixed_adams (which iterate of the corrector is final is
 *   known only after the read-back) run as in the un-decoded solve, then ndcn_linear_f32 decodes the state's panel - a tick inside the
 *   step through ndcn_tick_emit_f32 into the workspace's stage-input panel first.  ndcn_last_readout_path (cleared on entry):
 *   NDCN_READOUT_ADAMS for the fused kernel (NDCN_READOUT_NARROW beside it at H < 64), NDCN_READOUT_FIXED for the staged decodes.      */
NDCN_API int ndcn_ab_step_readout_f32(float *out, const float *y, const float *const *h_f, const float *h_a, int n, float dt,
                                      int64_t n_rows, int H, const float *Wd, const float *bd, int C, float *dec, float emit_off,
                                      void *stream);
NDCN_API int ndcn_solve_explicit_adams_readout_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags,
                                                   const float *y0, const float *h_dt, int64_t n_steps, const int64_t *h_tick_step,
                                                   const int *h_tick_same, const float *h_tick_off, int64_t n_ticks, int max_order,
                                                   const float *Wd, const float *bd, int C, float *out, void *workspace,
                                                   int64_t workspace_bytes, void *stream);
NDCN_API int ndcn_solve_fixed_adams_readout_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0,
                                                const float *h_dt, int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same,
                                                const float *h_tick_off, int64_t n_ticks, int max_order, float rtol, float atol,
                                                int max_iters, const float *Wd, const float *bd, int C, float *out, int *h_iters,
                                                int *h_converged, void *workspace, int64_t workspace_bytes, void *stream);
/* fixed_adams under a gradient (three more calls added to ABI 29: no existing declaration changes).
 * ndcn_fixed_adams_train_f32: ndcn_solve_fixed_adams_f32 - the same loop, launches, checks, read-backs, h_iters / h_converged and bits
 *   in `out` - that KEEPS what a reverse sweep needs in records the caller owns, in place of the history ring, the two state panels and
 *   the panel of the corrector's evaluation:
 *     rec_f [n_steps panels]   f_i, the evaluation grid step i starts with (as ndcn_explicit_adams_train_f32)
 *     rec_y [n_steps panels]   the state after step i; may be `out` itself on the default grid (tick j after step j)
 *     rec_u, rec_c [cap panels each]   per CORRECTOR evaluation, in the order they run: the iterate u_{r-1} it reads and F_r = func(u_{r-1})
 *     h_slot [n_steps]         HOST, written: the first slot of step i; the step uses the slots h_slot[i] .. h_slot[i] + h_iters[i] - 1
 *                              (a warm-up step uses none).  u_0 of a step is the predictor's u; u_R is the state in rec_y.
 *   The predictor writes u_0 into its slot, every evaluation writes into its slot, the corrector pass writes the new iterate into the
 *   state's panel: a step that iterates once copies nothing; each further iteration copies one panel (the iterate into its slot).
 *   The number of iterations is not known in advance.  When an evaluation would need slot `cap`, the call returns NDCN_ECAPACITY
 *   before anything is enqueued for it: no panel at or past `cap` is touched; the earlier steps' launches run to their end inside the
 *   caller's panels; `out`, the records and the host arrays are then incomplete and the caller runs the solve again with
 *   cap = n_steps * max_iters, which always suffices (cap = n_steps is the natural first attempt: one iteration per step).
 *     workspace                ndcn_fixed_adams_train_workspace_bytes(n_rows, H) bytes, 256-byte aligned: three RK4 stage panels, the
 *                              stage input, dy, delta, the counter and the scratch of ndcn_rhs_f32 - no ring, no state pair
 * ndcn_abm_adjoint_f32, the gradient of one evaluation gathered from the adjoints of the <= 11 predictor-corrector steps that held it -
 *   P_q the adjoint of step q's predictor increment, D_q that of the explicit part of its corrector:
 *     out = [base +] (((((0 + cp[0] P[0]) + cd[0] D[0]) + cp[1] P[1]) + cd[1] D[1]) + ...)
 *   every product and every sum rounded to fp32 on its own, no contraction, the sum started from an exact zero and the base added last:
 *   the chain of ndcn_ab_adjoint_f32 over the 2 n interleaved panels, n = 1..11 pairs, in ONE pass (up to 22 panels and the base read,
 *   every load of an item issued before its first use).  h_p, h_d: HOST arrays of n device panels; h_cp, h_cd: HOST arrays of their
 *   coefficients (fl32(dt * a), fl32(dt * m), formed by the caller).  P[q] and D[q] may be the same panel.  NDCN_EINVAL - before any
 *   launch - for any other n, a null panel, or `out` equal to a term (out == base is allowed).  Any alignment, any n_elem >= 0, the lanes
 *   of ndcn_ab_adjoint_f32.                                                                                                          */
NDCN_API int ndcn_abm_adjoint_f32(float *out, const float *base, const float *const *h_p, const float *h_cp, const float *const *h_d,
                                  const float *h_cd, int n, int64_t n_elem, void *stream);
NDCN_API int64_t ndcn_fixed_adams_train_workspace_bytes(int64_t n_rows, int H);
NDCN_API int ndcn_fixed_adams_train_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0,
                                        const float *h_dt, int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same,
                                        const float *h_tick_off, int64_t n_ticks, int max_order, float rtol, float atol, int max_iters,
                                        float *out, int *h_iters, int *h_converged, float *rec_f, float *rec_y, float *rec_u, float *rec_c,
                                        int64_t cap, int64_t *h_slot, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement aid (bench.py `roofline`): when enabled, every kernel launch made by this library is
 * bracketed by HIP events recorded on the launch stream.  ndcn_prof_read drains them into
 * h_out[kind*4 + {0: launches, 1: total ms, 2: total algorithmic bytes, 3: total flops}] for
 * kind in 0..ndcn_prof_kinds()-1 = {spmm, linear, rhs_fused, combine, error, sumsq, interp_fit,
 * interp_eval, fixed_stage, gather_rows, truth_dynamics}; returns 1 if the record ring overflowed.  */
NDCN_API int ndcn_prof_enable(int on);
NDCN_API int ndcn_prof_read(double *h_out, int n_kinds);
NDCN_API int ndcn_prof_kinds(void);
/* Which kernel family the LAST fused right-hand side of this thread was dispatched to (tests: the intended native path
 * ran, not merely a correct one): bit 0 rhs_fused2, bit 1 rhs_fused3 (group-record plan), bit 2 long-row plan active,
 * bit 3 a halo panel was passed; 0 before the first call.                                                          */
#define NDCN_PATH_FUSED2 1
#define NDCN_PATH_FUSED3 2
#define NDCN_PATH_HUB    4
#define NDCN_PATH_HALO   8
#define NDCN_PATH_SWEEP 16
#define NDCN_PATH_REC   32   /* no_control: relu(A X) + the stage algebra in the epilogue of the group-record SpMM (spmm_rec.hip) */
#define NDCN_PATH_WIDE  64   /* no_control: the same in the epilogue of the row SpMM (spmm.hip: spmm_wide_kernel)                */
#define NDCN_PATH_SMALL 128  /* H <= 128: the whole ODEFunc + epilogue in one launch (rhs_small.hip)                            */
#define NDCN_PATH_EXACT32 256 /* H = 256, range guard: the weights' in-row range exceeds what the two-piece fp16 product guarantees
                               * (four or more non-zero elements more than 2^19 below their row's largest magnitude: csrc/split16.h), found when
                               * the image was packed - the launch ran with the fp32 matrix cores as its consumer (v_mfma_f32_32x32x2_f32;
                               * nn.Linear in fp32, neural_dynamics.py:33; csrc/rhs_fused2_exact.hip).  NDCN_RANGE_GUARD=0
                               * switches the guard (and the 32-byte read-back per packed image) off                              */
#define NDCN_PATH_RANGE  512 /* such weights on a launch that exists only fused (x_add / x_mask / s_out): split product, warned once */
#define NDCN_PATH_DROP_EPI 1024 /* ndcn_rhs_drop_f32 / ndcn_rhs_rk_drop_f32: the dropout factor was applied inside the launch - with
                                 * NDCN_PATH_SMALL, or with NDCN_PATH_MID under ndcn_set_rhs_mid_drop (clear: by
                                 * the streaming pass ndcn_dropout_apply_f32 behind it)                                              */
#define NDCN_PATH_DYN 2048   /* a ground-truth dynamics launch with the RK epilogue (ndcn_dyn_rk_f32; ndcn_solver_desc::dyn)       */
#define NDCN_PATH_MID 4096   /* 16 <= H <= 128, H % 4 == 0, any number of rows: gather, fp32 MFMA Linear, ReLU and the COMBINE / RK4
                              * epilogue in one launch (rhs_mid.hip; ndcn_set_rhs_mid below).  An NDCN_RK_ERROR launch reports it for
                              * its K, the record is rk_error_f32's                                                                */
#define NDCN_PATH_ABL 8192   /* exactly one of NDCN_F_NO_GRAPH / NDCN_F_NO_CONTROL, 16 <= H <= 128, H % 4 == 0, any number of rows: K and the
                              * COMBINE / RK4 epilogue in one launch (rhs_abl.hip; ndcn_set_rhs_abl below), with NDCN_PATH_DROP_EPI when
                              * the dropout factor rode in it.  An NDCN_RK_ERROR launch reports it for its K, the record is rk_error_f32's */
NDCN_API int ndcn_debug_last_rhs_path(void);
/* Which kernels the LAST ndcn_linear_f32 / ndcn_linear_bwd_f32 call of this thread launched (tests: every dispatch route of the dense
 * Linear is reached on purpose, not merely some correct one); each call replaces the set, 0 for n = 0 and before the first call.
 * forward (linear.hip): */
#define NDCN_LIN_ROWDOT    1        /* Ho < 16, 64 <= Hi <= 512: a wave per row (linear_rowdot_kernel<ceil(Hi / 64)>)               */
#define NDCN_LIN_SMALL     2        /* other Hi < 16 or Ho < 16: a thread per output element                                      */
#define NDCN_LIN_MFMA64    4        /* fp32 MFMA tile kernel, 64 / 128 / 256 output features per workgroup (grid.y > 1 past 256)    */
#define NDCN_LIN_MFMA128   8
#define NDCN_LIN_MFMA256  16
#define NDCN_LIN_VEC      32        /* ... staging its operands by float4 (Hi % 4 == 0, S and W 16-byte aligned)                    */
/* backward, gS (linear_bwd.hip): */
#define NDCN_LIN_GS_SMALL  256      /* Hi < 16 or Ho < 16                                                                          */
#define NDCN_LIN_GS_FP32   512      /* fp32 MFMA GEMM (linear_gs_kernel<BN>): other shapes, and H = 256 without scratch, misaligned,
                                     * wide-range W (range guard) or NDCN_GS_SPLIT=0                                                */
#define NDCN_LIN_GS_RES    1024     /* H = 256 split product, resident weights (linear_gs_256_res_kernel), g already masked (Y null)  */
#define NDCN_LIN_GS_RES_MASK 2048   /* ... the same with the ReLU mask formed from Y                                                */
#define NDCN_LIN_GS_SPLIT32 4096    /* H = 256 split product, tile kernel of 32 rows (NDCN_GS_ROWS=32)                              */
#define NDCN_LIN_GS_SPLIT64 8192    /* ... of 64 rows (n x 1 KiB >= 4 GiB, or NDCN_GS_ROWS=64)                                      */
/* backward, gW / gb: */
#define NDCN_LIN_GW_SMALL  65536    /* Hi < 16 or Ho < 16                                                                          */
#define NDCN_LIN_GW_FP32   131072   /* fp32 MFMA (linear_wgrad_kernel<NI>): other shapes, and H = 256 with NDCN_GW_SPLIT=0          */
#define NDCN_LIN_GW_SPLIT  262144   /* H = 256: three bf16 pieces per operand (linear_wgrad_256_split_kernel)                       */
#define NDCN_LIN_GW_SUM2   524288   /* gW and gb summed over the chunks in one launch (chunk_sum2_kernel; otherwise chunk_sum_kernel) */
NDCN_API int ndcn_debug_last_linear_path(void);
/* Which kernel the LAST solver-VJP call of this thread launched (ABI 20; tests: each case reaches the element path and grid it targets),
 * as (grid << 16) | kernel | NDCN_RKB_VEC.  Each call replaces it; 0 before the first call and for ndcn_rk_pull_f32 with n = 0.         */
#define NDCN_RKB_COMBINE      1     /* ndcn_rk_combine_bwd_f32                                                                      */
#define NDCN_RKB_ERROR        2     /* ndcn_rk_error_bwd_f32                                                                        */
#define NDCN_RKB_RMS          4     /* ndcn_rk_rms_bwd_f32                                                                          */
#define NDCN_RKB_DENSE        8     /* ndcn_dopri5_interp_bwd_f32                                                                   */
#define NDCN_RKB_DENSE_MULTI 16     /* ndcn_dopri5_interp_bwd_multi_f32                                                             */
#define NDCN_RKB_DOT_DIFF    32     /* ndcn_rk_dot_diff_f32                                                                         */
#define NDCN_RKB_PULL        64     /* ndcn_rk_pull_f32                                                                             */
#define NDCN_RKB_VEC        128     /* ... by 16 bytes per lane (n % 4 == 0, every panel 16-byte aligned); the grid counts float4 items then */
NDCN_API int ndcn_debug_last_rk_bwd_path(void);
/* Which kernel of the FORWARD solver panel operations the last call of this thread launched (ABI 24; tests: each case reaches the kernel,
 * element path, reduction and grid it targets).  Set by ndcn_rk_combine_f32, ndcn_rk_error_f32, ndcn_scaled_sumsq_f32,
 * ndcn_dopri5_interp_fit_f32, ndcn_interp_eval_f32, ndcn_dopri5_interp_direct_f32, ndcn_dopri5_interp_direct_multi_f32,
 * ndcn_fixed_stage_f32, ndcn_tick_emit_f32, ndcn_fixed_stage_emit_f32, ndcn_scale_f32, ndcn_copy_f32 and ndcn_relu_bwd_f32 (and by the
 * solver's own use of the same wrappers).  Each of these calls clears the word on entry and records its LAST launch: 0 before the
 * first call, after a call that launched nothing (n_elem = 0 of an element-wise kernel, an argument error) - and a call that takes
 * several launches reports the last one (ndcn_tick_emit_f32 with more than 8 ticks: the launch of the last group;
 * ndcn_fixed_stage_emit_f32 with more than 8 ticks: the NDCN_RKF_TICK_EMIT launch behind the stage).  64 bits:
 *   bits  0..7   the kernel, one of the NDCN_RKF_* numbers below (NDCN_RKF_KERNEL_MASK)
 *   bits  8..11  op of ndcn_fixed_stage_f32 (0..5) / ndcn_fixed_stage_emit_f32 (0 or 5); 0 otherwise
 *   bit   12     NDCN_RKF_VEC: 16 bytes per lane (n % 4 == 0 and every panel 16-byte aligned; scale and copy: both panels aligned, any n,
 *                the n % 4 tail by single elements); the grid counts float4 items then
 *   bit   13     NDCN_RKF_ATEN: a reduction in ATen's single-thread float32 order (one workgroup; NDCN_RKF_VEC is clear)
 *   bit   14     NDCN_RKF_PAR64: a reduction by the parallel fixed-order fp64 pair (partial sums per workgroup, then reduce_finish)
 *   bits 32..63  the grid of that launch in workgroups (streaming kernels go up to 2^24; the partial-sum launch of a reduction, <= 2048) */
#define NDCN_RKF_COMBINE              1   /* ndcn_rk_combine_f32                                                                   */
#define NDCN_RKF_ERROR                2   /* ndcn_rk_error_f32                                                                     */
#define NDCN_RKF_SUMSQ                3   /* ndcn_scaled_sumsq_f32                                                                 */
#define NDCN_RKF_INTERP_FIT           4   /* ndcn_dopri5_interp_fit_f32                                                            */
#define NDCN_RKF_INTERP_EVAL          5   /* ndcn_interp_eval_f32                                                                  */
#define NDCN_RKF_INTERP_DIRECT        6   /* ndcn_dopri5_interp_direct_f32                                                         */
#define NDCN_RKF_INTERP_DIRECT_MULTI  7   /* ndcn_dopri5_interp_direct_multi_f32                                                   */
#define NDCN_RKF_FIXED_STAGE          8   /* ndcn_fixed_stage_f32                                                                  */
#define NDCN_RKF_TICK_EMIT            9   /* ndcn_tick_emit_f32                                                                    */
#define NDCN_RKF_FIXED_STAGE_EMIT    10   /* ndcn_fixed_stage_emit_f32                                                             */
#define NDCN_RKF_SCALE               11   /* ndcn_scale_f32                                                                        */
#define NDCN_RKF_COPY                12   /* ndcn_copy_f32                                                                         */
#define NDCN_RKF_RELU_BWD            13   /* ndcn_relu_bwd_f32 (always by single elements)                                         */
#define NDCN_RKF_KERNEL_MASK       0xff
#define NDCN_RKF_OP_SHIFT             8
#define NDCN_RKF_VEC             0x1000
#define NDCN_RKF_ATEN            0x2000
#define NDCN_RKF_PAR64           0x4000
#define NDCN_RKF_GRID_SHIFT          32
NDCN_API int64_t ndcn_debug_last_rk_path(void);
/* Which SpMM kernel the LAST SpMM of this thread launched (ABI 21; tests: each case reaches the route it targets): ndcn_spmm_f32, and the
 * no_control epilogues of ndcn_rhs_rk_f32 (NDCN_PATH_REC / NDCN_PATH_WIDE above).  A family bit | NDCN_SPMM_VEC | NDCN_SPMM_HALO |
 * (LPR or NV) << NDCN_SPMM_LANES_SHIFT | record shape << NDCN_SPMM_REC_SHIFT | mode << NDCN_SPMM_MODE_SHIFT | rows_per_block <<
 * NDCN_SPMM_RPB_SHIFT.  ndcn_spmm_f32 clears it first: 0 for an operator without rows and before the first call.                      */
#define NDCN_SPMM_CSR        1      /* spmm_csr_kernel<VW, LPR, HALO>: a block of rows per workgroup, LPR lanes per row                */
#define NDCN_SPMM_WIDE       2      /* spmm_wide_kernel<NV, HALO, MODE>: H = 256 NV, one row per wave                                 */
#define NDCN_SPMM_REC        4      /* spmm_rec_kernel<R, CAP, RECW, HALO, MODE>: the group-record plan                               */
#define NDCN_SPMM_SWEEP      8      /* spmm_sweep_kernel: the column-sweep plan                                                       */
#define NDCN_SPMM_HUB       16      /* long-row plan: segments and their combine ran first; the other bits are the light launch's     */
#define NDCN_SPMM_VEC       32      /* 16 bytes per lane slot (VW = 4; always for WIDE / REC / SWEEP)                                */
#define NDCN_SPMM_HALO      64      /* the kernel's HALO form (a halo panel was passed)                                               */
#define NDCN_SPMM_LANES_SHIFT 8     /* bits 8..15: LPR of CSR (1..64), NV of WIDE (1..4)                                               */
#define NDCN_SPMM_REC_SHIFT  16     /* bits 16..17: REC shape {R, CAP, KiB}: 1 {8, 32, 1}, 2 {16, 40, 2}, 3 {8, 48, 2}                 */
#define NDCN_SPMM_MODE_SHIFT 18     /* bits 18..19: REC / WIDE epilogue: 0 plain, NDCN_RK_COMBINE, NDCN_RK_ERROR, NDCN_RK_RK4          */
#define NDCN_SPMM_RPB_SHIFT  20     /* bits 20..28: rows_per_block of CSR (16..256)                                                    */
NDCN_API int ndcn_debug_last_spmm_path(void);
/* The range guard of the H = 256 Linear (NDCN_PATH_EXACT32 above): on = 1 / 0 switches it PROCESS-WIDE at run time, on < 0 returns to the
 * default (on, unless the environment says NDCN_RANGE_GUARD=0); returns the previous state (1 / 0).  Off, every packed image takes the
 * split fp16 product whatever its range, and packing does not read back.  Images packed while the guard was off are judged when
 * they are packed next.                                                                                                            */
NDCN_API int ndcn_set_range_guard(int on);
/* The one-launch right-hand side for hidden widths 16..128 at any size (NDCN_PATH_MID above, csrc/rhs_mid.hip; the three calls are additions to ABI 29:
 * no existing declaration changes, and tests/test_gpu_tape_dropout.py and tests/test_gpu_dropout_combine.py pin that number).   Without it
 * those widths run composed once n_rows * H exceeds 2^18: row SpMM into a scratch panel, MFMA Linear, stand-alone stage kernel.  Every
 * panel it writes - K, y_next, y_aux - equals the composed path's bit for bit, so the switch is invisible in the results.
 * ndcn_set_rhs_mid switches it PROCESS-WIDE at run time and returns the previous mode; mode < 0 returns to the environment's
 * (NDCN_RHS_MID, default 0):
 *   0  off
 *   1  on wherever the narrow-panel kernel (NDCN_PATH_SMALL) does not take the shape, for H <= 96 (wider, the launch holds one
 *      workgroup per compute unit and measured slower than the composed kernels: those widths stay composed)
 *   2  on for every supported shape, ahead of that kernel (tests, measuring the crossover; the narrow-panel kernel's stage sums
 *      start from the new stage's product, so the sign of an all-zero sum can differ from this route's there)
 * ndcn_rhs_f32 / ndcn_rhs_rk_f32 (plain, NDCN_RK_COMBINE with or without y_aux, NDCN_RK_RK4; NDCN_RK_ERROR as the plain launch plus the
 * stand-alone error kernel) take the route; it declines - the launch runs as without it - a halo panel, NDCN_F_NO_GRAPH /
 * NDCN_F_NO_CONTROL, x_add / x_mask / s_out and panels that are not 16-byte aligned, and it declines dropout unless
 * ndcn_set_rhs_mid_drop is on.  ndcn_rhs_work_bytes does not depend on the mode.
 * ndcn_set_rhs_mid_drop (NDCN_RHS_MID_DROP, default 0): on = 1 lets ndcn_rhs_drop_f32 / ndcn_rhs_rk_drop_f32 take the route too, wherever
 * the mode above takes the shape and under the same conditions - the dropout factor of ndcn_dropout is applied in the launch's epilogue
 * (K' = K * m, one Philox call per 16-byte lane) and K' is what the launch stores and what its stage algebra consumes: plain, NDCN_RK_COMBINE
 * with or without y_aux, NDCN_RK_RK4; NDCN_RK_ERROR as the plain dropout launch plus the stand-alone error kernel.  The launch reports
 * NDCN_PATH_MID | NDCN_PATH_DROP_EPI and writes the bits of the composed form (composed launches, ndcn_dropout_apply_f32 or
 * ndcn_dropout_combine_f32, stand-alone stage kernel).  PROCESS-WIDE; returns the previous value (1 / 0); on < 0 returns to the
 * environment's.  Without effect while the mode is 0 or does not take the shape; a halo panel with dropout stays NDCN_EINVAL.
 * ndcn_rhs_mid_supported: the shape part of that decision for `mode` - H a multiple of 4 in 16..128, n_rows >= 1, neither NO_ flag,
 * and in mode 1 H <= 96 and n_rows * H beyond the narrow-panel kernel's bound; a host predicate, no device needed.                          */
NDCN_API int ndcn_set_rhs_mid(int mode);
NDCN_API int ndcn_set_rhs_mid_drop(int on);
NDCN_API int ndcn_rhs_mid_supported(int64_t n_rows, int H, uint32_t flags, int mode);
/* The one-launch right-hand side of the two ablations for hidden widths 16..128 at any size (NDCN_PATH_ABL above, csrc/rhs_abl.hip; the two
 * calls are additions to ABI 29: no existing declaration changes).  Without it ndcn_rhs_rk_f32 with NDCN_F_NO_CONTROL (K = relu(A X)) or
 * NDCN_F_NO_GRAPH (K = relu(X W^T + b)) runs composed below H = 256: the SpMM or the MFMA Linear, a stand-alone stage kernel reading K
 * again and, under dropout, a mask pass.  With it ONE launch forms K - no_control: one fma per stored entry in stored order from +0;
 * no_graph: the fp32 MFMA sequence of ndcn_linear_f32 -, applies the dropout factor of ndcn_dropout behind the ReLU and runs the stage
 * algebra on it: plain, NDCN_RK_COMBINE with or without y_aux, NDCN_RK_RK4; NDCN_RK_ERROR and calls whose stage panels are not 16-byte
 * aligned as the plain launch plus the stand-alone stage kernel.  Every panel it writes - K, y_next, y_aux - and the error record equal the
 * composed path's bit for bit, so the switch is invisible in the results.
 * ndcn_set_rhs_abl switches it PROCESS-WIDE at run time and returns the previous value (1 / 0); on < 0 returns to the environment's
 * (NDCN_RHS_ABL, default 0).  It declines - the launch runs as without it - both flags or neither, other widths (H = 256 included), a halo
 * panel, x_add / x_mask / s_out, X or K (no_graph: or W) not 16-byte aligned, and an operator that carries a long-row plan for this width.
 * ndcn_rhs_work_bytes does not depend on it.
 * ndcn_rhs_abl_supported: the shape part of that decision - exactly one of the two flags, H a multiple of 4 in 16..128, n_rows >= 1; a
 * host predicate, no device needed.                                                                                                    */
NDCN_API int ndcn_set_rhs_abl(int on);
NDCN_API int ndcn_rhs_abl_supported(int64_t n_rows, int H, uint32_t flags);
/* The two one-launch kernels above inside the device-resident solver (ndcn_solver_*; four calls and the NDCN_SOLVER_RHS_* names added to
 * ABI 29: no existing declaration changes).  ndcn_solver_create chooses ONE launch kind per solve; without this switch a solve at hidden
 * widths 16..128 on more than 2^18 state elements - and every NDCN_F_NO_GRAPH solve below H = 256 - evaluates f composed: SpMM into a
 * scratch panel, MFMA Linear, a stand-alone stage kernel.  Under it such a solve takes NDCN_SOLVER_RHS_MID (graph and control,
 * ndcn_rhs_mid_supported) or NDCN_SOLVER_RHS_ABL (exactly one of the two flags, ndcn_rhs_abl_supported, no long-row plan for the width):
 * dopri5 runs one combine and six launches per attempted step, the stage algebra in the launches' epilogues - replayed steps read their
 * coefficients fl(dt * beta) from device memory as NDCN_SOLVER_RHS_SMALL does - and forms the error record as ndcn_rhs_rk_f32 builds an
 * NDCN_RK_ERROR launch on these routes, the plain launch plus ndcn_rk_error_f32's record; euler and rk4 carry their stage algebra in the
 * launches by value; midpoint, which has no such form, keeps its kind.  The kinds come behind every other choice and never apply to a
 * shard: no solve that has another kind changes it.  Trajectory, decoded ticks, step log and nfe are bit for bit those of the same solve
 * with the switch off; ndcn_debug_last_rhs_path reports NDCN_PATH_MID / NDCN_PATH_ABL after such a launch.
 * ndcn_set_solver_mid switches it PROCESS-WIDE at run time - read by ndcn_solver_create, a solver keeps its kind - and returns the previous
 * mode; mode < 0 returns to the environment's (NDCN_SOLVER_MID, default 0); independent of ndcn_set_rhs_mid / ndcn_set_rhs_abl:
 *   0  off
 *   1  on except where a solver step measured slower than the composed form - H > 96, in every variant -
 *      and the sizes ndcn_rhs_mid_supported leaves to the narrow-panel kernel in its mode 1
 *   2  on for every supported shape
 * ndcn_solver_mid_mode: the current mode, read without changing it.  ndcn_solver_mid_takes: the sizes' part of the decision for `mode` - a
 * host predicate, no device needed.  ndcn_solver_rhs_kind: the kind this solver was created with (NDCN_EINVAL for a null handle); a shard
 * reports NDCN_SOLVER_RHS_FUSED1 or NDCN_SOLVER_RHS_COMPOSED - whether its weights get packed - and dispatches every launch through
 * ndcn_rhs_rk_f32's selection.                                                                                                          */
#define NDCN_SOLVER_RHS_COMPOSED 0   /* ndcn_rhs_f32 picks the kernel, stand-alone stage kernels                                          */
#define NDCN_SOLVER_RHS_FUSED1   1   /* H = 256 without a row-group plan: packed weights, stand-alone stage kernels                       */
#define NDCN_SOLVER_RHS_MFMA     2   /* H = 256 on a row-group plan: the split-product launch with its epilogues                          */
#define NDCN_SOLVER_RHS_REC      3   /* NDCN_F_NO_CONTROL on a group-record plan                                                           */
#define NDCN_SOLVER_RHS_WIDE     4   /* NDCN_F_NO_CONTROL, the wide row SpMM with epilogues                                                */
#define NDCN_SOLVER_RHS_SMALL    5   /* dopri5 on a narrow panel (n_rows * H <= 2^18): one launch per evaluation                          */
#define NDCN_SOLVER_RHS_DYN      6   /* the truth dynamics (ndcn_solver_desc::dyn)                                                        */
#define NDCN_SOLVER_RHS_MID      7   /* 16 <= H <= 128 at any size under ndcn_set_solver_mid: csrc/rhs_mid.hip                            */
#define NDCN_SOLVER_RHS_ABL      8   /* the ablations at 16 <= H <= 128 under ndcn_set_solver_mid: csrc/rhs_abl.hip                       */
NDCN_API int ndcn_set_solver_mid(int mode);
NDCN_API int ndcn_solver_mid_mode(void);
NDCN_API int ndcn_solver_mid_takes(int64_t n_rows, int H, uint32_t flags, int mode);
NDCN_API int ndcn_solver_rhs_kind(const ndcn_solver *solver);
/* The reverse of ONE right-hand-side evaluation K = relu(W (A X) + b) as a call (csrc/rhs_mid_bwd.hip; five calls added to ABI 29: no
 * existing declaration changes) - what autograd executes for ODEFunc.forward (neural_dynamics.py:27-36) under the drivers' training
 * step, and what the two native tapes run per evaluation:
 *   gZ = g (.) [K > 0]   (NDCN_F_RELU in flags and premasked = 0; otherwise gZ = g: the caller masked it already, or there is no ReLU)
 *   gX = acc_scale * A^T (gZ W)                    gX nullable: not wanted
 *   gW = acc_scale * gZ^T S,  gb = acc_scale * colsum gZ,  S = A X;  accumulate != 0: added to what gW / gb hold (product and sum
 *        rounded separately).  gb nullable.  With dropout K is the stored K' and acc_scale the kept elements' factor s (ndcn_dropout).
 *   S    nullable: A X as the forward launch wrote it; it is re-formed (gathered) when absent
 *   work ndcn_rhs_vjp_work_bytes(n_rows, H, flags) bytes, 256-byte aligned: [S panel | gS panel | ndcn_linear_bwd_f32's scratch], each part
 *        rounded up to 256 bytes; after a call with gX the n_rows x H panel gS = gZ W stands at byte offset
 *        ndcn_rhs_vjp_work_bytes(n_rows, H, NDCN_F_NO_CONTROL) / 2 (tests read it there)
 * A square, A_t its transpose (both ignored under NDCN_F_NO_GRAPH except A->n_rows); no halo panel.  Composed, the call is five launches:
 * SpMM, ndcn_linear_bwd_f32's three, transposed SpMM.  For 16 <= H <= 128 (H a multiple of 4) at any number of rows ONE launch can form
 * gS and the row-chunk partials of gW / gb - S never leaves the compute unit, gZ is formed once: three launches - with the raw 32-bit
 * words of the composed launches in gS, gX, gW and gb, signs of zero and NaN positions included.  ndcn_set_rhs_mid_bwd switches that route
 * PROCESS-WIDE at run time and returns the previous mode; mode < 0 returns to the environment's (NDCN_RHS_MID_BWD, default 0):
 *   0  off
 *   1  on for the widths at which it measured not slower than the composed launches
 *   2  on for every supported shape
 * The native tapes (ndcn_tape_backward_f32, ndcn_fixed_backward_f32 and their variants) follow the same switch.  The route declines - the
 * call runs composed - NDCN_F_NO_GRAPH / NDCN_F_NO_CONTROL, other widths (H = 256 included) and panels that are not 16-byte aligned.
 * ndcn_rhs_mid_bwd_supported: the shape part of that decision for `mode` (mode < 0: the switch's current mode); a host predicate, no
 * device needed.  ndcn_debug_last_rhs_vjp_path: the route of the LAST reverse evaluation of this PROCESS (a reverse pass runs on
 * autograd's thread), whoever ran it; 0 before the first.                                                                          */
#define NDCN_VJP_COMPOSED 1   /* SpMM (unless S was given), ndcn_linear_bwd_f32's launches, transposed SpMM                           */
#define NDCN_VJP_MID      2   /* gS and the partials of gW / gb in one launch (rhs_mid_bwd.hip), chunk sum, transposed SpMM           */
#define NDCN_VJP_ABL      3   /* an ablation's one-launch reverse (rhs_abl_bwd.hip; ndcn_set_rhs_abl_bwd below)                        */
NDCN_API int ndcn_rhs_vjp_f32(const ndcn_csr *A, const ndcn_csr *A_t, const float *X, const float *K, const float *g, const float *W,
                              const float *S, float *gX, float *gW, float *gb, void *work, int H, uint32_t flags, int premasked,
                              float acc_scale, int accumulate, void *stream);
NDCN_API int64_t ndcn_rhs_vjp_work_bytes(int64_t n_rows, int H, uint32_t flags);
NDCN_API int ndcn_set_rhs_mid_bwd(int mode);
NDCN_API int ndcn_rhs_mid_bwd_supported(int64_t n_rows, int H, uint32_t flags, int mode);
NDCN_API int ndcn_debug_last_rhs_vjp_path(void);
/* The one-launch reverse of the two ablations for hidden widths 16..128 at any size (csrc/rhs_abl_bwd.hip; NDCN_VJP_ABL and the three
 * calls are additions to ABI 29: no existing declaration changes).  Without it ndcn_rhs_vjp_f32 and the native tapes run the reverse of an
 * NDCN_F_NO_CONTROL evaluation as two launches (the ReLU mask into a scratch panel, the transposed SpMM over it) and of an NDCN_F_NO_GRAPH
 * evaluation as ndcn_linear_bwd_f32's three plus a scaling pass whenever acc_scale has no SpMM to ride in.  With it
 *   NO_CONTROL  ONE launch: gX = acc_scale * A^T (g (.) [K > 0]) with the mask applied to the gathered rows of g - one fma per stored entry
 *               of A_t in stored order from +0, then the product with acc_scale (also when it is 1)
 *   NO_GRAPH    the NDCN_VJP_MID launch with S = X forms gS and the row-chunk partials of gW / gb, stores gS straight into gX - times
 *               acc_scale exactly where the composed call runs its scaling pass - and the chunk sum follows: two launches
 * with the raw 32-bit words of the composed launches in gX, gW and gb, signs of zero and NaN positions included, for every accumulate /
 * acc_scale combination; no gS panel is left in `work`.  ndcn_set_rhs_abl_bwd switches it PROCESS-WIDE at run time and returns the
 * previous value (1 / 0); on < 0 returns to the environment's (NDCN_RHS_ABL_BWD, default 0); independent of ndcn_set_rhs_abl and
 * ndcn_set_rhs_mid_bwd.  The native tapes follow it.  It declines - the call runs composed, NDCN_VJP_COMPOSED - both flags or neither,
 * other widths (H = 256 included), NO_CONTROL without a mask to fuse (premasked, or no NDCN_F_RELU: one launch already) or without gX,
 * NO_GRAPH without gW, a non-square operator, X / g / K / W / gX not 16-byte aligned or gX aliasing an input, and for NO_CONTROL an A_t
 * that carries a long-row plan for this width.  ndcn_rhs_vjp_work_bytes does not depend on it.
 * ndcn_rhs_abl_bwd_supported: the shape part of that decision - exactly one of the two flags, H a multiple of 4 in 16..128,
 * 1 <= n_rows < 2^31 - 64; a host predicate, no device needed.  ndcn_rhs_abl_bwd_on: the switch's current value (1 / 0), read without
 * changing it - a caller that picks between one ndcn_rhs_vjp_f32 call and its own per-operation calls decides by it.                   */
NDCN_API int ndcn_set_rhs_abl_bwd(int on);
NDCN_API int ndcn_rhs_abl_bwd_on(void);
NDCN_API int ndcn_rhs_abl_bwd_supported(int64_t n_rows, int H, uint32_t flags);

/* ---- training through the adaptive solver: the solve that keeps its tape, and its reverse pass ---------------------------------
 * Replaces, for a plain ODEFunc on one state tensor, what the reference's drivers do by autograd through odeint
 * (heat_dynamics.py:313-334, dgnn.py:192-222; torchdiffeq/_impl/dopri5.py:58-122, rk_common.py:41-61, misc.py:84-170, interp.py:21-65):
 * ndcn_tape_dopri5_f32 integrates y' = relu(W (A y) + b) over the n_t strictly increasing ticks (out: n_t panels, the first is y0)
 * with the launches of the per-operation path (same kernels, same order: bit-identical values and accept / reject decisions) and
 * records every attempted step; ndcn_tape_backward_f32 turns g_out (n_t panels: the gradient of the trajectory) into the gradients
 * of y0, W and b - the panel operations' VJP kernels of this header plus the adjoint of the step-size controller's scalar chain
 * (dt, t0 / t1, the initial step and the interpolation abscissa carry gradient in the reference: csrc/tape.hip).  The reverse pass
 * may run any number of times over one tape (retain_graph, Jacobian rows): it only reads the record; memory it asks `alloc` for is
 * scratch of that call and may be released when the call returns (stream-ordered).
 * opts: {first_step given (0 / 1), safety, ifactor, dfactor, max_num_steps, keep S (0 / 1: evaluations that can - ndcn_rhs_adj_supported -
 * also store S = A u on the tape, one panel more per evaluation, instead of one SpMM per evaluation in the reverse pass)}.
 * At: the transposed operator (unused with NDCN_F_NO_GRAPH).
 * alloc: device memory for the tape (12 panels per attempted step, 18 where S is kept; ~24 more during a reverse pass), owned by the
 * caller; what ndcn_tape_dopri5_f32 asked for is kept until ndcn_tape_destroy.  y0, W, b and the operators must stay valid and
 * unchanged until then.
 * Errors as the solver's: NDCN_EMAXSTEPS, NDCN_EUNDERFLOW, NDCN_ENONFINITE; the tape handle is set on every path - destroy it.
 * ndcn_tape_dopri5_budget_f32 (ABI 28) bounds that record: record_budget_bytes < 0 is ndcn_tape_dopri5_f32 (which calls it with -1);
 * otherwise an attempt is recorded in full while (panels held by full attempts) * panel bytes + (12 + (keep S ? 6 : 0)) * panel bytes
 * fits the budget - ndcn_tape_attempt_is_full, asked before the attempt starts - and is THIN from the first one that does not fit on
 * (0: every attempt).  A thin attempt forms its stage inputs, derivatives and S panels in a ring of <= 10 + 6 panels all thin attempts
 * share and keeps y1 and k7 alone - the next attempt's y0 and k1; a rejected one hands those two panels on.  The reverse pass re-forms
 * a thin attempt's ring panels from (y0, k1, dt) by the forward pass's own launches before it processes the attempt: the gradients
 * are the same bits, for six more right-hand-side evaluations per thin attempt and pass; ndcn_tape_nfe does not count them.
 * ndcn_tape_record: out = {panels held by full attempts, panels kept for thin attempts (2 per accepted one + 2 spare), ring panels,
 * thin attempts}.
 * ndcn_tape_dopri5_drop_f32 (ABI 29): the budgeted call plus a dropout descriptor - training through dopri5 with ODEFunc's dropout
 * active (dgnn.py:192-222 at its default --dropout 0.5; heat_dynamics.py:313-334 with --dropout p).  desc NULL: exactly
 * ndcn_tape_dopri5_budget_f32 (which calls it so).  Otherwise every evaluation's launch carries the mask of (desc->p, desc->seed) and
 * a number of its own: desc->evaluation is the number of the solve's FIRST evaluation f0, the initial step's f1 follows when it is
 * evaluated (first_step not given), then six per attempted step, accepted or rejected, in stage order -
 * ndcn_tape_attempt_evaluation(first, probe evaluated, attempt index) is the first number of an attempt (no device call), and
 * ndcn_tape_evaluations how many numbers the solve consumed.  An attempt keeps its numbers: re-formed in the reverse pass (budget) it
 * re-creates its masks and consumes none.  The record holds K' = relu(z) * m; the reverse pass is the p = 0 one with every J^T g times
 * s = 1 / (1 - p) (no mask stored or re-created).  S = A u is not kept (opts[5] is ignored: 12 panels per full attempt) and the error
 * record always comes from ndcn_rk_error_f32's kernel, as on the per-operation path with dropout.                                  */
typedef struct ndcn_tape ndcn_tape;
typedef void *(*ndcn_alloc_fn)(void *ctx, int64_t bytes);
NDCN_API int ndcn_tape_dopri5_f32(const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H, uint32_t flags,
                                  const float *y0, const double *ticks, int64_t n_t, double rtol, double atol, const double *opts,
                                  float *out, ndcn_alloc_fn alloc, void *alloc_ctx, ndcn_tape **tape, void *stream);
NDCN_API int ndcn_tape_dopri5_budget_f32(const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H, uint32_t flags,
                                         const float *y0, const double *ticks, int64_t n_t, double rtol, double atol,
                                         const double *opts, float *out, ndcn_alloc_fn alloc, void *alloc_ctx, ndcn_tape **tape,
                                         void *stream, int64_t record_budget_bytes);
NDCN_API int ndcn_tape_dopri5_drop_f32(const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H, uint32_t flags,
                                       const float *y0, const double *ticks, int64_t n_t, double rtol, double atol,
                                       const double *opts, float *out, ndcn_alloc_fn alloc, void *alloc_ctx, ndcn_tape **tape,
                                       void *stream, int64_t record_budget_bytes, const ndcn_dropout *desc);
NDCN_API int64_t ndcn_tape_attempt_evaluation(int64_t first, int probe_evaluated, int64_t attempt);
NDCN_API int64_t ndcn_tape_evaluations(const ndcn_tape *tape);
NDCN_API int ndcn_tape_attempt_is_full(int64_t record_budget_bytes, int64_t full_panels, int64_t panel_bytes, int keep_s,
                                       int thin_already);             /* 1: recorded in full, 0: thin (no device call) */
NDCN_API int ndcn_tape_record(const ndcn_tape *tape, int64_t out[4]);
NDCN_API int ndcn_tape_backward_f32(ndcn_tape *tape, const float *g_out, float *g_y0, float *g_W, float *g_b, void *stream);
NDCN_API int64_t ndcn_tape_steplog(const ndcn_tape *tape, double *rows, int64_t cap);   /* 5 doubles per attempt, as ndcn_solver_steplog */
NDCN_API int64_t ndcn_tape_nfe(const ndcn_tape *tape);
NDCN_API void ndcn_tape_destroy(ndcn_tape *tape);
/* The fixed-grid methods (solvers.py:79-99 with fixed_grid.py:7-29, rk_common.py:72-78; method: NDCN_M_EULER / _MIDPOINT / _RK4) the same
 * way, without a tape object - the reverse pass re-forms the stages of a step from the stored trajectory:
 * ndcn_fixed_grid_train_f32 writes the n_ticks + 1 states (out[0] = y0) for the step sizes h_dt (the grid's differences in the state
 * dtype, solvers.py:81), ndcn_fixed_grid_backward_f32 maps g_out (n_ticks + 1 panels) to the gradients of y0, W and b.  Any size; the
 * launches of _impl/fixed_train.py::_FixedGridSolve.  alloc: scratch (<= 22 panels), may be released when the call returns (stream-ordered). */
NDCN_API int ndcn_fixed_grid_train_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, int method,
                                       const float *y0, const float *h_dt, int64_t n_ticks, float *out, ndcn_alloc_fn alloc,
                                       void *alloc_ctx, void *stream);
NDCN_API int ndcn_fixed_grid_backward_f32(const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H, uint32_t flags,
                                          int method, const float *traj, const float *g_out, const float *h_dt, int64_t n_ticks,
                                          float *g_y0, float *g_W, float *g_b, ndcn_alloc_fn alloc, void *alloc_ctx, void *stream);
/* ---- the decoder inside the fixed-grid reverse sweep (ABI 27) ------------------------------------------------------------------
 * NDCN decodes every tick (neural_dynamics.py:148-160: output_layer over the whole trajectory); trained through odeint's `readout`
 * the solve's autograd node receives the gradient of the DECODED ticks, g_dec (n_ticks + 1, N, C), and the (n_ticks + 1, N, H) tensor
 * g_dec . Wd that the Linear's own backward would write is never formed.
 * ndcn_readout_bwd_f32, one tick:  gi[n,h] = the fp32 fma chain over c = 0 .. C-1 of gd[n,c] * Wd[c,h] from +0;
 *   out = a + ((((0 + h_add[0]) + h_add[1]) + ...) + gi), every sum rounded on its own - what ndcn_rk_combine_f32(out, a, {h_add..., gi},
 *   {1, ..}) gives - and out = gi when a is NULL and n_add is 0 (a NULL with addends: the sum without the base);  n_add <= 5;
 *   acc (nullable: then y and ws may be NULL): C*H + C doubles, acc[c*H + h] += sum_n gd[n,c] y[n,h] and acc[C*H + c] += sum_n gd[n,c]
 *   in fp64 in a fixed order (no atomics: the same inputs give the same bits); the caller zeroes it before the first tick and rounds
 *   it to fp32 after the last.  ws: ndcn_readout_bwd_ws_bytes(n_rows, H, C) bytes of scratch.  1 <= C <= 15, any H >= 1: NDCN_EINVAL
 *   otherwise.  Panels whose base is 16-byte aligned with H % 4 == 0 take 16-byte lanes.
 * ndcn_fixed_grid_backward_readout_f32: ndcn_fixed_grid_backward_f32 with (g_dec, Wd (C, H), C) in place of g_out and the decoder's
 *   gradients g_Wd (C, H) / g_bd (C) as further outputs (both nullable; g_bd alone nullable): bit for bit the gradients that
 *   ndcn_fixed_grid_backward_f32 gives for g_out[i] = the chain above of g_dec[i].                                                 */
NDCN_API int64_t ndcn_readout_bwd_ws_bytes(int64_t n_rows, int H, int C);
NDCN_API int ndcn_readout_bwd_f32(float *out, const float *a, const float *const *h_add, int n_add, const float *gd, const float *Wd,
                                  const float *y, int64_t n_rows, int H, int C, double *acc, void *ws, void *stream);
NDCN_API int ndcn_fixed_grid_backward_readout_f32(const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H,
                                                  uint32_t flags, int method, const float *traj, const float *g_dec, const float *Wd,
                                                  int C, const float *h_dt, int64_t n_ticks, float *g_y0, float *g_W, float *g_b,
                                                  float *g_Wd, float *g_bd, ndcn_alloc_fn alloc, void *alloc_ctx, void *stream);

/* ---- TemporalGCN (neural_dynamics.py:179-238): the LSTM-GNN / GRU-GNN / RNN-GNN baselines (csrc/tgcn.hip) ------------------------
 * Per tick the reference runs a GraphConvolution on an N x 1 column, flattened to 1 x (N Hg), into an LSTMCell / GRUCell / RNNCell whose
 * input weight W_ih is M x (N Hg), M = G Hr with G = 4 / 3 / 1.  With S = A X (N x T, ticks in columns, row-major) and r = A 1 the
 * convolution is Z[i, j, tau] = S[i, tau] w[j] + r[i] b[j] (w, b: the Hg weights and biases of the convolution's Linear(1, Hg)).
 * ndcn_tgcn_proj_f32: GI[tau, g] = b_ih[g] + sum_{i, j} W_ih[g, i Hg + j] relu(Z[i, j, tau]) for ALL ticks, GI (T x M, row-major); W_ih
 *   is read once per ndcn_tgcn_chunk(0) ticks; a NaN in Z reaches GI.  ws: ndcn_tgcn_proj_ws_bytes(N, T, M) bytes (per-workgroup partial
 *   blocks, summed by a second launch in workgroup order: no atomics, the same inputs give the same bits).
 * ndcn_tgcn_proj_bwd_f32: from GGI = dL/dGI (T x M): g_Wih[g, i Hg + j] = sum_tau GGI[tau, g] relu(Z)[i, j, tau], written once, never
 *   read; with gZ = [Z > 0] sum_g W_ih[g, .] GGI[tau, g] (0 at Z = 0; a NaN Z passes the gradient), g_w[j] = sum gZ S, g_b[j] = sum gZ r
 *   (per-workgroup partials summed in fp64 in workgroup order); g_bih[g] = sum_tau GGI[tau, g] (fp64, tick order).
 *   ws: ndcn_tgcn_proj_bwd_ws_bytes(N) bytes.
 * Both: N >= 1, T >= 1, 1 <= Hg <= 8, 1 <= M <= 64; NDCN_EINVAL - before any launch - otherwise, for a null pointer and for an output
 * that is an input or another output.
 * ndcn_tgcn_cell_f32: the recurrence over all T ticks in one launch.  rnn_type 0 rnn (tanh), 1 gru, 2 lstm, torch's cell definitions
 *   (lstm gates in order i, f, g, o; gru n = tanh(gi_n + r (W_hn h + b_hn)), h' = (1 - z) n + z h).  GI (T x G Hr) carries b_ih already;
 *   W_hh (G Hr x Hr), b_hh (G Hr); h0, c0 (Hr; nullable: zeros; c0 lstm only).  Writes H (T x Hr) and the record the reverse reads:
 *   gates (T x 4 Hr: lstm i, f, g, o; gru r, z, n, W_hn h + b_hn; rnn h' in the first Hr) and, lstm only, c_rec (T x Hr); hT / cT
 *   (nullable): the state after the last tick.
 * ndcn_tgcn_cell_bwd_f32: its reverse from gH = dL/dH (T x Hr): GGI (T x G Hr), g_Whh, g_bhh and (nullable) g_h0, g_c0.
 * Both: T >= 1, Hr >= 1, G Hr <= 64; NDCN_EINVAL - before any launch - otherwise, for a null pointer and for aliased outputs.       */
NDCN_API int ndcn_tgcn_chunk(int reverse);
NDCN_API int64_t ndcn_tgcn_proj_ws_bytes(int64_t n_nodes, int T, int M);
NDCN_API int ndcn_tgcn_proj_f32(const float *S, const float *r, const float *w, const float *b, const float *W_ih, const float *b_ih,
                                float *GI, void *ws, int64_t n_nodes, int T, int Hg, int M, void *stream);
NDCN_API int64_t ndcn_tgcn_proj_bwd_ws_bytes(int64_t n_nodes);
NDCN_API int ndcn_tgcn_proj_bwd_f32(const float *S, const float *r, const float *w, const float *b, const float *W_ih, const float *GGI,
                                    float *g_Wih, float *g_w, float *g_b, float *g_bih, void *ws, int64_t n_nodes, int T, int Hg, int M,
                                    void *stream);
NDCN_API int ndcn_tgcn_cell_f32(int rnn_type, const float *GI, const float *W_hh, const float *b_hh, const float *h0, const float *c0,
                                float *H, float *gates, float *c_rec, float *hT, float *cT, int T, int Hr, void *stream);
NDCN_API int ndcn_tgcn_cell_bwd_f32(int rnn_type, const float *gH, const float *gates, const float *c_rec, const float *H, const float *h0,
                                    const float *c0, const float *W_hh, float *GGI, float *g_Whh, float *g_bhh, float *g_h0, float *g_c0,
                                    int T, int Hr, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NDCN_HIP_H */
