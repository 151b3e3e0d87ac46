// Training through the adaptive solver as ONE native object: a dopri5 solve of y' = relu(W (A y) + b) that keeps what its
// reverse pass needs (the "tape"), and that reverse pass.
//
// The reference trains by autograd THROUGH its solver (heat_dynamics.py:313-334, dgnn.py:192-222): every panel operation of
// every attempted step and the whole scalar chain of the step-size controller (dt, t0 / t1, the initial step, the interpolation
// abscissa are tensors with history: dopri5.py:76-122, rk_common.py:41-61, misc.py:84-170, interp.py:38-65) are nodes of a graph
// the interpreter builds and walks - ~65 nodes forward and as many backward for a README-sized solve, 5 + 7 ms of host time
// around < 1 ms of kernels (tools/micro/c1_host_profile.py).  Here the same launches, in the same order with the same arguments
// as ndcn_amd/torchdiffeq/_impl/autograd_path.py issues them (forward values bit-identical: same kernels), are enqueued by one
// C call per direction; the scalar chain's adjoint is written out by hand below (tape_backward: "scalar chain") and follows
// torch's conventions where they matter (maximum / minimum halve the gradient on ties, python max() picks the first maximum,
// float32 tensors take float32 gradients).
//
// Backward of one attempted step, stage sums in PULL form (autograd_path._RhsStagePullFn): with g_u_m the gradient of the m-th
// stage input (u_7 = y1), evaluation e receives  g_k_e = (what the dense output, the error ratio and later steps sent)
// + sum_{m > e} dt beta_{m,e} g_u_m  in one ndcn_rk_combine_f32 pass, then the right-hand side's VJP (mask, gS = gZ W, A^T gS;
// g_W += gZ^T S, g_b += sum gZ) yields g_u_e; the step size receives <g_u_m, u_m - y0> / dt per stage (one ndcn_rk_dot_diff_f32
// pass), the error ratio's and the dense output's inner products from their VJP kernels.  All inner products of an attempt land
// in one device array and come back in ONE read: the only host synchronisation per attempted step, as in the forward pass.
//
// Memory: panels come from the caller's allocator (ndcn_alloc_fn: torch's caching allocator through the binding) and live until
// ndcn_tape_destroy: 12 panels per attempted step (stage inputs and derivatives; + up to 6 of S = A u with keep_s) + ~24 of scratch in
// the reverse pass.  Under a record budget (ndcn_tape_dopri5_budget_f32) the attempts past the budget are THIN: everything an attempt
// computes is a function of (y0, k1, dts) and the operator, y0 is the previous accepted attempt's u[7] and k1 its k[6] (FSAL), so a thin
// attempt keeps those two panels alone (when it is accepted; a rejected one leaves them to the next attempt) and forms the rest in a ring
// of <= 10 + 6 panels that every thin attempt shares.  The reverse pass re-forms a thin attempt's ring panels by the forward's own launch
// sequence (attempt_launches: same modes, coefficients, S decisions, packed weights - the same bits) before it processes the attempt:
// 2 accepted + 2 + 16 panels instead of 12 A (+ 6 A), for six more right-hand-side evaluations per thin attempt and pass.
//
// Dropout (ndcn_tape_dopri5_drop_f32): every evaluation's launch carries the counter-based mask of csrc/dropout.h - (p, seed) of the solve
// and a number of its own, in the order autograd_path.integrate_dopri5_grad evaluates: f0, the initial step's f1, then six per attempted
// step (ndcn_tape_attempt_evaluation).  An attempt records its first number: re-forming it in the reverse pass re-creates its masks and
// consumes none.  The stored derivatives are K' = relu(z) * m with m in {0, s}: [K' > 0] is the mask of ReLU and dropout together, so the
// reverse pass is the p = 0 one with J^T g scaled by s (rhs_vjp) - no mask stored, none re-created there.  The error record is never
// taken in evaluation 7's epilogue (the per-operation path with dropout runs the stand-alone kernel at every size) and S = A u is not
// kept (the dropout launches do not write it).
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>

#include "common.h"
#include "dopri5_tableau.h"
#include "hostrec.h"
#include "kernels.h"

using namespace ndcn;

namespace {

struct Attempt {
    bool accept = false, fused_err = false;
    bool thin = false;                 // u[2..6], k[1..5], S live in the tape's ring: the reverse pass re-forms them first
    int64_t ev0 = 0;                   // dropout: the solve-relative number of evaluation 2 of this attempt (3 .. 7: the five after it)
    double t0 = 0, dt = 0, dt_next = 0, factor = 0;
    float dts = 0, ratio = 0;
    const float *y0 = nullptr;
    const float *k[7] = {};
    const float *u[8] = {};            // u[2..6]: stage inputs, u[7] = y1
    const float *S[8] = {};            // S[e] = A u[e] where the evaluation's launch wrote it on the side (keep_s), else null
    std::vector<int> dense;            // indices into ndcn_tape::groups, in forward order
};

struct DenseGroup {
    int attempt = -1, nt = 0;
    int tick[7] = {};
    float x[7] = {};
    float a0 = 0, a1 = 0;
};

struct HostScratch {                   // per host thread: pinned mirror of the device records + an event
    double *h = nullptr;               // kDotSlots x 8 doubles (inner products) ...
    double *rec = nullptr;             // ... + 8 (a reduction record), same allocation
    double *h_dev = nullptr, *rec_dev = nullptr;      // their device aliases (polling mode: hostrec.h), else null
    hipEvent_t ev = nullptr;
};

// the panels one attempt's launches write; S[e]: in - the panel evaluation e stores S = A u in where its launch can (null: one from the
// arena), out - that panel, or untouched where the launch cannot
struct StagePanels {
    float *u[8] = {}, *k[7] = {}, *S[8] = {};
};

constexpr int kDotSlots = 40;          // 8 doubles each
constexpr int kDenseBatch = 24;        // dense-output groups (<= 7 ticks each) whose inner products one read-back carries; the other slots: error + 6 rows

int host_scratch(HostScratch **out) {
    static thread_local HostScratch hs;
    if (!hs.h) {
        NDCN_HIP(hipHostMalloc(reinterpret_cast<void **>(&hs.h), (size_t)(kDotSlots + 1) * 8 * sizeof(double), hipHostMallocDefault));
        hs.rec = hs.h + (size_t)kDotSlots * 8;
        NDCN_HIP(hipEventCreateWithFlags(&hs.ev, hipEventDisableTiming));
        void *alias = nullptr;
        if (poll_records_enabled() && hipHostGetDevicePointer(&alias, hs.h, 0) == hipSuccess && alias) {
            hs.h_dev = static_cast<double *>(alias);
            hs.rec_dev = hs.h_dev + (size_t)kDotSlots * 8;
        }
    }
    *out = &hs;
    return NDCN_OK;
}

}  // namespace

struct ndcn_tape {
    ndcn_csr A = {}, At = {};
    const float *W = nullptr, *b = nullptr;
    int H = 0;
    uint32_t flags = 0;
    int64_t n_rows = 0, n = 0;
    double rtol = 0, atol = 0, safety = 0, ifactor = 0, dfactor = 0;
    int64_t max_steps = 0;
    bool first_given = false;
    bool keep_s = false;               // opts[5]: evaluations on the lattice-plan kernel also store S = A u (ndcn_rhs_rk_adj_f32's s_out): one panel
                                       // more per evaluation on the tape instead of one SpMM per evaluation in the reverse pass
    ndcn_alloc_fn alloc = nullptr;
    void *alloc_ctx = nullptr;
    // arena
    char *chunk = nullptr;
    size_t chunk_left = 0, panel_bytes = 0;
    // forward record
    std::vector<double> ticks;
    std::vector<Attempt> attempts;
    std::vector<DenseGroup> groups;
    std::vector<double> log;
    int64_t nfe = 0;
    const float *y_in = nullptr, *f0 = nullptr, *yh = nullptr, *f1 = nullptr;      // initial step: y0, f(y0), y0 + h0 f0, f(yh)
    double s0 = 0, s1 = 0, s2 = 0;     // the three sums of squares
    float d0 = 0, d1 = 0, d2r = 0, d2 = 0, h0 = 0, h1 = 0;
    bool h0_const = false, h1_alt = false;
    double dt_init = 0;
    // device scratch
    double *d_red = nullptr, *d_dots = nullptr;
    void *d_ws = nullptr, *d_ws2 = nullptr, *d_bws = nullptr;
    float *work = nullptr;             // rhs scratch (packed weights for H = 256)
    bool packed = false;
    void *bwork = nullptr;             // linear_bwd scratch
    bool bpacked = false;
    // dropout (ndcn_tape_dopri5_drop_f32): (p, seed) in the kernels' form, the number of the solve's first evaluation, numbers consumed
    bool drop = false;
    DropArgs dargs = {};
    uint64_t ev_first = 0;
    int64_t evals = 0;
    // record budget (ndcn_tape_dopri5_budget_f32): < 0 unlimited
    int64_t budget = -1;
    bool thin_mode = false;            // an attempt did not fit: it and all later ones are thin
    int64_t full_panels = 0, thin_kept = 0, ring_panels = 0, thin_attempts = 0;
    StagePanels ring;                  // u[2..6], k[1..5], S[2..7]: shared by the thin attempts; u[7] / k[6]: the spare pair (the kept pair of
                                       // the next accepted thin attempt; at the end of the forward pass, where a re-run's y1 / k7 land)
    double *d_red_rerun = nullptr;     // the error record of a re-run attempt (nobody reads it)
    bool bwd_marked = false;           // arena position behind the forward record: every reverse pass starts its scratch there
    char *mark_chunk = nullptr;
    size_t mark_left = 0;
};

namespace {

int arena(ndcn_tape *t, size_t bytes, void **out) {
    bytes = (bytes + 255u) & ~(size_t)255u;
    if (bytes > t->chunk_left) {
        // small panels share a chunk (one allocator call per 64), large ones get their own
        size_t want = bytes;
        if (bytes * 64 <= ((size_t)32 << 20)) want = bytes * 64;
        void *p = t->alloc(t->alloc_ctx, (int64_t)want + 256);
        if (!p) { set_error("tape: the allocator returned no memory for %zu bytes", want); return NDCN_EINVAL; }
        t->chunk = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(p) + 255u) & ~(uintptr_t)255u);
        t->chunk_left = want;
    }
    *out = t->chunk;
    t->chunk += bytes;
    t->chunk_left -= bytes;
    return NDCN_OK;
}

int panel(ndcn_tape *t, float **p) {
    void *q = nullptr;
    int rc = arena(t, t->panel_bytes, &q);
    *p = static_cast<float *>(q);
    return rc;
}

// the descriptor of the solve's evaluation number `ev`
DropArgs drop_at(const ndcn_tape *t, int64_t ev) {
    DropArgs d = t->dargs;
    const uint64_t e = t->ev_first + (uint64_t)ev;
    d.e0 = (uint32_t)(e & 0xffffffffu);
    d.e1 = (uint32_t)(e >> 32);
    return d;
}

// the flags of the tape's evaluations (the H = 256 launches read the image of W the tape packed once)
uint32_t eval_flags(const ndcn_tape *t) { return t->flags | (t->packed ? NDCN_F_PACKED : 0u); }

// out = f(x) without a stage epilogue.  ev: the evaluation's number within the solve (read with dropout only)
int eval_plain(ndcn_tape *t, const float *x, float *out, hipStream_t st, int64_t ev, bool count = true) {
    if (count) t->nfe++;
    const DropArgs d = drop_at(t, ev);
    return rhs_f32(&t->A, x, nullptr, t->A.n_cols, t->W, t->b, out, t->work, t->H, eval_flags(t), st, t->drop ? &d : nullptr);
}

// the n doubles the launches enqueued since the matching arm wrote at `d_src` -> hs->h[0..n) (polling mode: d_src IS hs->h's alias)
int fetch(ndcn_tape *t, const double *d_src, int n_doubles, hipStream_t st, HostScratch *hs) {
    (void)t;
    if (hs->h_dev && d_src == hs->h_dev) return rec_wait(hs->h, n_doubles, st);
    NDCN_HIP(hipMemcpyAsync(hs->h, d_src, (size_t)n_doubles * sizeof(double), hipMemcpyDeviceToHost, st));
    NDCN_HIP(hipEventRecord(hs->ev, st));
    NDCN_HIP(hipEventSynchronize(hs->ev));
    return NDCN_OK;
}

// the 2-double reduction record: armed before the launches, then read into hs->h[0..1]
void arm_record(ndcn_tape *t, HostScratch *hs) {
    if (hs->rec_dev && t->d_red == hs->rec_dev) rec_arm(hs->rec, 2);
}
int fetch_record(ndcn_tape *t, hipStream_t st, HostScratch *hs) {
    if (hs->rec_dev && t->d_red == hs->rec_dev) {
        int rc = rec_wait(hs->rec, 2, st);
        hs->h[0] = hs->rec[0];
        hs->h[1] = hs->rec[1];
        return rc;
    }
    return fetch(t, t->d_red, 2, st, hs);
}

// misc.py:71-76: x.norm() / numel ** 0.5 as float32 values (autograd_path._rms_value)
float rms_value(double s, double numel) {
    const float nrm = (s == s && s >= 0) ? (float)sqrt(s) : NAN;
    return nrm / (float)sqrt(numel);
}

int rms(ndcn_tape *t, const float *a, const float *b, const float *y, hipStream_t st, HostScratch *hs, double &sum, double &bad) {
    arm_record(t, hs);
    int rc = scaled_sumsq_f32(a, b, y, (float)t->rtol, (float)t->atol, t->n, t->d_red, t->d_ws, st);
    if (rc) return rc;
    rc = fetch_record(t, st, hs);
    if (rc) return rc;
    sum = hs->h[0];
    bad = hs->h[1];
    return NDCN_OK;
}

// misc.py:84-143 with order = 4, as autograd_path._initial_step evaluates it
int initial_step(ndcn_tape *t, hipStream_t st, HostScratch *hs, int64_t &pending_bad) {
    double bad;
    int rc = rms(t, t->y_in, nullptr, t->y_in, st, hs, t->s0, bad);
    if (rc) return rc;
    pending_bad = (int64_t)bad;
    rc = rms(t, t->f0, nullptr, t->y_in, st, hs, t->s1, bad);
    if (rc) return rc;
    t->d0 = rms_value(t->s0, (double)t->n);
    t->d1 = rms_value(t->s1, (double)t->n);
    t->h0 = initial_h0(t->d0, t->d1, &t->h0_const);
    float *yh, *f1;
    if ((rc = panel(t, &yh)) || (rc = panel(t, &f1))) return rc;
    const float *kp[1] = {t->f0};
    const float cp[1] = {t->h0};
    rc = rk_combine_f32(yh, t->y_in, kp, cp, 1, t->n, st);
    if (rc) return rc;
    rc = eval_plain(t,yh, f1, st, 1);
    if (rc) return rc;
    t->yh = yh;
    t->f1 = f1;
    rc = rms(t, f1, t->f0, t->y_in, st, hs, t->s2, bad);
    if (rc) return rc;
    t->d2r = rms_value(t->s2, (double)t->n);
    t->d2 = t->d2r / t->h0;
    t->h1 = initial_h1(t->d1, t->d2, t->h0, &t->h1_alt);
    t->dt_init = initial_dt(t->h0, t->h1);
    return NDCN_OK;
}

// The launches of one attempted step from (y0, k0 = f(y0), dts) into the panels of P: the forward pass, and the reverse pass where it
// re-forms a thin attempt (rerun: the evaluations are not counted, the error record goes to `d_red`, which nobody reads).  S_used[e]:
// the panel evaluation e's launch wrote S = A u to, else null.  ev0: the number of the attempt's first evaluation (dropout).
int attempt_launches(ndcn_tape *t, const float *y0, const float *k0, float dts, StagePanels &P, const float **S_used, bool *fused_err,
                     double *d_red, bool rerun, int64_t ev0, hipStream_t st) {
    int rc;
    float *const *u = P.u, *const *k = P.k;
    const bool both = !(t->flags & (NDCN_F_NO_GRAPH | NDCN_F_NO_CONTROL));
    const float *kall[7] = {k0, k[1], k[2], k[3], k[4], k[5], k[6]};
    const float *kp[8];
    float cp[8];
    for (int e = 0; e < 8; ++e) S_used[e] = nullptr;
    auto s_panel = [&](int e, float **out) -> int {
        if (!P.S[e]) {
            if (rerun) { set_error("tape: a re-formed attempt asks for an S panel its forward pass did not"); return NDCN_EINVAL; }
            int r = panel(t, &P.S[e]);
            if (r) return r;
        }
        S_used[e] = *out = P.S[e];
        return NDCN_OK;
    };
    int m = dt_terms(dts, kBeta[0], 1, kall, kp, cp);
    rc = rk_combine_f32(u[2], y0, kp, cp, m, t->n, st);
    if (rc) return rc;
    const uint32_t fl = t->flags;
    for (int i = 0; i < 5; ++i) {
        // evaluation i + 2: k[i + 1] = f(u[i + 2]); its epilogue forms u[i + 3] from row i + 1 of the tableau
        const int mp = dt_terms(dts, kBeta[i + 1], i + 1, kall, kp, cp);
        cp[mp] = dts * (float)kBeta[i + 1][i + 1];
        if (!rerun) t->nfe++;
        RkOpt opt = {};
        // (the lattice-plan kernel, or the narrow-panel one - what rhs_rk_f32 picks for H <= 128 at launch-bound sizes -: both write S on the side)
        if (t->keep_s && both && rhs_s_out_supported(&t->A, t->H, fl, NDCN_RK_COMBINE, mp)) {
            if ((rc = s_panel(i + 2, &opt.s_out))) return rc;
        }
        const DropArgs d = drop_at(t, ev0 + i);
        rc = rhs_rk_f32(&t->A, u[i + 2], nullptr, t->A.n_cols, t->W, t->b, k[i + 1], t->work, t->H, eval_flags(t), NDCN_RK_COMBINE, y0, kp, cp,
                        mp, u[i + 3], 0.f, 0.f, nullptr, nullptr, st, opt.s_out ? &opt : nullptr, t->drop ? &d : nullptr);
        if (rc) return rc;
    }
    *fused_err = !t->drop && t->n > aten_order_max_elems();
    if (*fused_err) {
        const int mp = dt_terms(dts, kCErr, 6, kall, kp, cp);
        cp[mp] = dts * (float)kCErr[6];
        if (!rerun) t->nfe++;
        RkOpt opt = {};
        if (t->keep_s && both && rhs_adj_supported(&t->A, t->H, fl, NDCN_RK_ERROR, mp)) {
            if ((rc = s_panel(7, &opt.s_out))) return rc;
        }
        rc = rhs_rk_f32(&t->A, u[7], nullptr, t->A.n_cols, t->W, t->b, k[6], t->work, t->H, eval_flags(t),
                        NDCN_RK_ERROR, y0, kp, cp, mp, nullptr, (float)t->rtol, (float)t->atol, d_red, t->d_ws2, st,
                        opt.s_out ? &opt : nullptr);
        if (rc) return rc;
    } else {
        rc = eval_plain(t,u[7], k[6], st, ev0 + 5, !rerun);
        if (rc) return rc;
        m = dt_terms(dts, kCErr, 7, kall, kp, cp);
        rc = rk_error_f32(y0, u[7], kp, cp, m, (float)t->rtol, (float)t->atol, t->n, d_red, t->d_ws, st);
        if (rc) return rc;
    }
    return NDCN_OK;
}

// a thin attempt's panels: the ring (allocated at the first thin attempt) and the spare pair for y1 / k7
int thin_panels(ndcn_tape *t, StagePanels &P) {
    int rc;
    if (!t->ring.u[2]) {
        for (int e = 2; e <= 6; ++e)
            if ((rc = panel(t, &t->ring.u[e]))) return rc;
        for (int j = 1; j <= 5; ++j)
            if ((rc = panel(t, &t->ring.k[j]))) return rc;
        t->ring_panels = 10;
        void *p;
        if ((rc = arena(t, 2 * sizeof(double) + 256, &p))) return rc;
        t->d_red_rerun = static_cast<double *>(p);
    }
    if (!t->ring.u[7]) {
        if ((rc = panel(t, &t->ring.u[7])) || (rc = panel(t, &t->ring.k[6]))) return rc;
        t->thin_kept += 2;
    }
    P = t->ring;
    return NDCN_OK;
}

int forward_attempt(ndcn_tape *t, Attempt &a, hipStream_t st, HostScratch *hs, double &bad_out) {
    int rc;
    arm_record(t, hs);
    StagePanels P;
    a.thin = t->thin_mode = !ndcn_tape_attempt_is_full(t->budget, t->full_panels, (int64_t)t->panel_bytes, t->keep_s, t->thin_mode);
    if (a.thin) {
        if ((rc = thin_panels(t, P))) return rc;
        t->thin_attempts++;
    } else {
        for (int e = 2; e <= 7; ++e)
            if ((rc = panel(t, &P.u[e]))) return rc;
        for (int j = 1; j < 7; ++j)
            if ((rc = panel(t, &P.k[j]))) return rc;
        t->full_panels += 12;
    }
    a.ev0 = ndcn_tape_attempt_evaluation(0, t->first_given ? 0 : 1, (int64_t)t->attempts.size() - 1);
    t->evals = a.ev0 + 6;
    rc = attempt_launches(t, a.y0, a.k[0], a.dts, P, a.S, &a.fused_err, t->d_red, false, a.ev0, st);
    for (int e = 2; e <= 7; ++e)                   // (S panels the launches took from the arena)
        if (a.thin && P.S[e] && !t->ring.S[e]) t->ring.S[e] = P.S[e], t->ring_panels++;
        else if (!a.thin && P.S[e]) t->full_panels++;
    if (rc) return rc;
    rc = fetch_record(t, st, hs);
    if (rc) return rc;
    a.ratio = (float)(hs->h[0] / (double)t->n);
    bad_out = hs->h[1];
    for (int e = 2; e <= 7; ++e) a.u[e] = P.u[e];
    for (int j = 1; j < 7; ++j) a.k[j] = P.k[j];
    return NDCN_OK;
}

// ---------------------------------------------------------------------------------------------------- reverse pass helpers
struct Bwd {
    ndcn_tape *t;
    hipStream_t st;
    float *gW_acc = nullptr, *gb_acc = nullptr;
    bool have_w = false;
    float *tmpS = nullptr, *tmpG = nullptr;      // S = A x ; gS / gZ
};

int add_into(float *acc, const float *x, int64_t n, hipStream_t st) {
    const float *kp[1] = {x};
    const float one[1] = {1.f};
    return rk_combine_f32(acc, acc, kp, one, 1, n, st);
}

// (g_X into gx (nullable: not wanted); g_W, g_b accumulated) of K = f(X) for the upstream gradient g: autograd_ops.rhs_vjp
// premasked: g already IS gZ = g (.) [K > 0] (rk_pull_f32 applied the mask where it formed g)
// dropout: K is K' = relu(z) * m, m in {0, s}, and J^T g = s * (this closed form masked by K') - s rides in the scalars below: the
// accumulation scale of g_W / g_b, the alpha of the transposed SpMM, and without a graph one scaling pass (autograd_ops.rhs_vjp)
int rhs_vjp(Bwd &B, const float *X, const float *K, const float *g, float *gx, const float *S_kept = nullptr, bool premasked = false) {
    ndcn_tape *t = B.t;
    const float s = t->drop ? t->dargs.s : 1.f;
    // g_W / g_b: this evaluation's + what the later evaluations sent (autograd_path._add_carried), in the launch that sums the chunks
    int rc = rhs_vjp_f32(&t->A, &t->At, X, K, g, t->W, S_kept, gx, B.gW_acc, t->b ? B.gb_acc : nullptr, B.tmpS, B.tmpG, t->bwork, t->H,
                         t->flags, premasked, s, s, B.have_w, true, &t->bpacked, B.st);
    if (rc) return rc;
    if (!(t->flags & NDCN_F_NO_CONTROL)) B.have_w = true;
    return NDCN_OK;
}

// out = base (nullable) + sum_i c_i p_i over the non-null p_i; returns the result pointer through `res` (nullptr: nothing to add;
// base itself when there are no terms)
// must_own: the result has to live in `out` (it outlives the scratch panels `base` may point into)
int gather_sum(ndcn_tape *t, float *out, const float *base, const float *const *p, const float *c, int n_p, hipStream_t st, const float **res,
               bool must_own = false) {
    const float *kp[8];
    float cp[8];
    int m = 0;
    for (int i = 0; i < n_p; ++i)
        if (p[i] && c[i] != 0.f) {
            kp[m] = p[i];
            cp[m] = c[i];
            ++m;
        }
    if (m == 0) {
        if (must_own && base && base != out) {
            NDCN_HIP(hipMemcpyAsync(out, base, (size_t)t->n * sizeof(float), hipMemcpyDeviceToDevice, st));
            base = out;
        }
        *res = base;
        return NDCN_OK;
    }
    int rc = rk_combine_f32(out, base, kp, cp, m, t->n, st);
    *res = out;
    return rc;
}

inline double half_on_tie_gt(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }    // share of max(a, b)'s gradient that a receives

}  // namespace

// ====================================================================================================== C ABI
extern "C" {

int ndcn_tape_attempt_is_full(int64_t record_budget_bytes, int64_t full_panels, int64_t panel_bytes, int keep_s, int thin_already) {
    if (record_budget_bytes < 0) return 1;
    if (thin_already) return 0;
    const int64_t cost = (12 + (keep_s ? 6 : 0)) * panel_bytes;       // the upper bound for one full attempt
    return full_panels * panel_bytes + cost <= record_budget_bytes ? 1 : 0;
}

int64_t ndcn_tape_attempt_evaluation(int64_t first, int probe_evaluated, int64_t attempt) {
    return first + 1 + (probe_evaluated ? 1 : 0) + 6 * attempt;       // f0, the initial step's f1, six per attempted step before this one
}

int ndcn_tape_dopri5_f32(const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H, uint32_t flags, const float *y0,
                         const double *ticks, int64_t n_t, double rtol, double atol, const double *opts, float *out, ndcn_alloc_fn alloc,
                         void *alloc_ctx, ndcn_tape **tape, void *stream) {
    return ndcn_tape_dopri5_budget_f32(A, At, W, b, H, flags, y0, ticks, n_t, rtol, atol, opts, out, alloc, alloc_ctx, tape, stream, -1);
}

int ndcn_tape_dopri5_budget_f32(const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H, uint32_t flags,
                                const float *y0, const double *ticks, int64_t n_t, double rtol, double atol, const double *opts, float *out,
                                ndcn_alloc_fn alloc, void *alloc_ctx, ndcn_tape **tape, void *stream, int64_t record_budget_bytes) {
    return ndcn_tape_dopri5_drop_f32(A, At, W, b, H, flags, y0, ticks, n_t, rtol, atol, opts, out, alloc, alloc_ctx, tape, stream,
                                     record_budget_bytes, nullptr);
}

int ndcn_tape_dopri5_drop_f32(const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H, uint32_t flags, const float *y0,
                              const double *ticks, int64_t n_t, double rtol, double atol, const double *opts, float *out,
                              ndcn_alloc_fn alloc, void *alloc_ctx, ndcn_tape **tape, void *stream, int64_t record_budget_bytes,
                              const ndcn_dropout *desc) {
    NDCN_CHECK_ARG(A && y0 && ticks && n_t >= 1 && out && alloc && tape && opts && H > 0, "bad argument");
    const bool no_graph = flags & NDCN_F_NO_GRAPH, no_control = flags & NDCN_F_NO_CONTROL;
    NDCN_CHECK_ARG(no_graph || (At && A->n_rows == A->n_cols), "a square operator and its transpose are required");
    NDCN_CHECK_ARG(no_control || W, "weight missing");
    for (int64_t i = 1; i < n_t; ++i) NDCN_CHECK_ARG(ticks[i] > ticks[i - 1], "t must be strictly increasing");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HostScratch *hs;
    int rc = host_scratch(&hs);
    if (rc) return rc;
    ndcn_tape *t = new (std::nothrow) ndcn_tape();
    if (!t) { set_error("out of host memory"); return NDCN_EINVAL; }
    *tape = t;                                     // (the caller destroys it on every path, errors included)
    t->A = *A;
    if (At) t->At = *At;
    t->W = W;
    t->b = b;
    t->H = H;
    t->flags = flags;
    t->n_rows = A->n_rows;
    t->n = A->n_rows * (int64_t)H;
    t->rtol = rtol;
    t->atol = atol;
    t->first_given = opts[0] != 0.0;
    t->safety = opts[1];
    t->ifactor = opts[2];
    t->dfactor = opts[3];
    t->max_steps = (int64_t)opts[4];
    t->keep_s = opts[5] != 0.0;
    if (desc) {
        NDCN_CHECK_ARG(flags & NDCN_F_RELU, "dropout without NDCN_F_RELU is not supported");
        if ((rc = drop_args(desc, &t->dargs))) return rc;
        t->drop = true;
        t->ev_first = desc->evaluation;
        t->keep_s = false;                         // (the dropout launches write no S: the reverse pass forms it by its SpMM)
    }
    t->alloc = alloc;
    t->alloc_ctx = alloc_ctx;
    t->budget = record_budget_bytes;
    t->panel_bytes = (size_t)t->n * sizeof(float) + 16;
    t->ticks.assign(ticks, ticks + n_t);
    void *p;
    if (hs->rec_dev) {
        t->d_red = hs->rec_dev;                    // the record lands in pinned host memory, the host polls (hostrec.h)
    } else {
        if ((rc = arena(t, 2 * sizeof(double) + 256, &p))) return rc;
        t->d_red = static_cast<double *>(p);
    }
    if ((rc = arena(t, (size_t)reduce_ws_bytes(), &t->d_ws))) return rc;
    if ((rc = arena(t, (size_t)reduce_ws_bytes(), &t->d_ws2))) return rc;
    const int64_t wb = rhs_work_bytes(t->n_rows, H, flags);
    if (wb > 0) {
        if ((rc = arena(t, (size_t)wb, &p))) return rc;
        t->work = static_cast<float *>(p);
        if (H == 256 && !no_control && !no_graph) {
            // the packed image of W once per solve (every evaluation reads it: NDCN_F_PACKED)
            if ((rc = pack_weight_256(W, t->work, st))) return rc;
            if (weights_wide_range(t->work)) t->keep_s = false;       // range guard: the fp32 route has no S output (rhs.hip)
            t->packed = true;
        }
    }
    // ---- dopri5.py:76-83
    t->y_in = y0;
    NDCN_HIP(hipMemcpyAsync(out, y0, (size_t)t->n * sizeof(float), hipMemcpyDeviceToDevice, st));
    float *f0;
    if ((rc = panel(t, &f0))) return rc;
    if ((rc = eval_plain(t,y0, f0, st, 0))) return rc;
    t->f0 = f0;
    t->evals = ndcn_tape_attempt_evaluation(0, t->first_given ? 0 : 1, 0);       // (what the solve consumes before its first attempt)
    t->nfe = 2;                                    // (the count the python path reports: autograd_path.py nfe = 2)
    int64_t pending_bad = 0;
    double dt;
    if (!t->first_given) {
        if ((rc = initial_step(t, st, hs, pending_bad))) return rc;
        t->nfe = 2;
        dt = t->dt_init;
    } else {
        dt = 0.01;                                 // dopri5.py:82
    }
    const float *y_cur = y0, *f_cur = f0;
    double t_lo = ticks[0], t_hi = ticks[0];
    int last_acc = -1;
    int64_t i = 0;
    while (i + 1 < n_t) {
        ++i;
        const double nxt = ticks[i];
        int64_t n_steps = 0;
        while (nxt > t_hi) {
            if (n_steps >= t->max_steps) { set_error("max_num_steps exceeded (%lld>=%lld)", (long long)n_steps, (long long)t->max_steps); return NDCN_EMAXSTEPS; }
            const double t0 = t_hi;
            if (!(t0 + dt > t0)) { set_error("underflow in dt %g", dt); return NDCN_EUNDERFLOW; }
            if (pending_bad != 0) { set_error("non-finite values in state `y`: %lld elements", (long long)pending_bad); return NDCN_ENONFINITE; }
            t->attempts.emplace_back();
            Attempt &a = t->attempts.back();
            a.t0 = t0;
            a.dt = dt;
            a.dts = (float)dt;
            a.y0 = y_cur;
            a.k[0] = f_cur;
            double bad = 0;
            if ((rc = forward_attempt(t, a, st, hs, bad))) return rc;
            const float ratio = a.ratio;
            a.accept = ratio <= 1.f;
            // misc.py:160-170 as the python path evaluates it (float64 scalars; sqrt in the ratio's float32)
            double dt_next;
            if (ratio == 0.f) {
                dt_next = dt * t->ifactor;
                a.factor = 0;
            } else {
                a.factor = step_factor(ratio, t->safety, t->ifactor, t->dfactor).factor;
                dt_next = dt / a.factor;
            }
            a.dt_next = dt_next;
            const double row[5] = {t0, dt, a.accept ? 1.0 : 0.0, (double)ratio, dt_next};
            t->log.insert(t->log.end(), row, row + 5);
            if (a.accept) {
                y_cur = a.u[7];
                f_cur = a.k[6];
                if (a.thin) t->ring.u[7] = t->ring.k[6] = nullptr;    // the spare pair is this step's kept pair now
                t_lo = t0;
                t_hi = t0 + dt;
                pending_bad = (int64_t)bad;
                last_acc = (int)t->attempts.size() - 1;
            } else {
                t_lo = t_hi = t0;
            }
            dt = dt_next;
            ++n_steps;
        }
        // interp.py:51-65: this tick and the following ones the accepted step covers (<= 7 per pass)
        if (last_acc < 0) { set_error("invalid interpolation: no accepted step covers t = %g", nxt); return NDCN_EINVAL; }
        const Attempt &a = t->attempts[(size_t)last_acc];
        DenseGroup g;
        g.attempt = last_acc;
        g.a0 = (float)t_lo;
        g.a1 = (float)t_hi;
        float xp[7 * 5];
        float *outs[7];
        for (;;) {
            const float at = (float)ticks[i];
            float *q = xp + 5 * g.nt;
            if (!interp_abscissa(g.a0, g.a1, at, q)) { set_error("invalid interpolation, fails `t0 <= t <= t1`: %g, %g, %g", (double)g.a0, (double)at, (double)g.a1); return NDCN_EINVAL; }
            outs[g.nt] = out + (size_t)i * t->n;
            g.tick[g.nt] = (int)i;
            g.x[g.nt] = q[3];
            ++g.nt;
            if (i + 1 < n_t && g.nt < 7 && !(ticks[i + 1] > t_hi)) ++i;
            else break;
        }
        float cm[7];
        for (int j = 0; j < 7; ++j) cm[j] = a.dts * (float)kCMid[j];
        rc = interp_direct_multi_f32(a.y0, a.u[7], a.k, cm, a.dts, xp, outs, g.nt, t->n, st);
        if (rc) return rc;
        t->attempts[(size_t)last_acc].dense.push_back((int)t->groups.size());
        t->groups.push_back(g);
    }
    if (t->thin_attempts > 0) {
        // where a re-run's y1 / k7 land: the spare pair (part of the forward record - the reverse pass may run again).  The rejected
        // thin attempts wrote theirs into panels later attempts took over: their reverse pass reads the re-run's
        StagePanels P;
        if ((rc = thin_panels(t, P))) return rc;
        for (Attempt &a : t->attempts)
            if (a.thin && !a.accept) a.u[7] = P.u[7], a.k[6] = P.k[6];
    }
    return NDCN_OK;
}

int ndcn_tape_record(const ndcn_tape *t, int64_t out[4]) {
    NDCN_CHECK_ARG(t && out, "bad argument");
    out[0] = t->full_panels;
    out[1] = t->thin_kept;
    out[2] = t->ring_panels;
    out[3] = t->thin_attempts;
    return NDCN_OK;
}

int64_t ndcn_tape_steplog(const ndcn_tape *t, double *rows, int64_t cap) {
    if (!t) return NDCN_EINVAL;
    const int64_t n = (int64_t)t->log.size() / 5;
    if (rows)
        for (int64_t i = 0; i < n && i < cap; ++i) memcpy(rows + 5 * i, t->log.data() + 5 * i, 5 * sizeof(double));
    return n;
}

int64_t ndcn_tape_nfe(const ndcn_tape *t) { return t ? t->nfe : NDCN_EINVAL; }

int64_t ndcn_tape_evaluations(const ndcn_tape *t) { return t ? t->evals : NDCN_EINVAL; }

void ndcn_tape_destroy(ndcn_tape *t) { delete t; }

int ndcn_tape_backward_f32(ndcn_tape *t, const float *g_out, float *g_y0, float *g_W, float *g_b, void *stream) {
    NDCN_CHECK_ARG(t && g_out && g_y0, "bad argument");
    const bool no_control = t->flags & NDCN_F_NO_CONTROL;
    NDCN_CHECK_ARG(no_control || (g_W && (g_b || !t->b)), "g_W / g_b missing");
    // The reverse pass may run more than once over one forward record (loss.backward(retain_graph=True), several torch.autograd.grad
    // calls, a retry after a failed pass): the record is only read; the scratch of a pass is carved from the arena at the mark the FIRST
    // pass found, the caller frees the blocks a pass asked for when it returns (the forward record's blocks live until ndcn_tape_destroy).
    if (!t->bwd_marked) {
        t->bwd_marked = true;
        t->mark_chunk = t->chunk;
        t->mark_left = t->chunk_left;
    } else {
        t->chunk = t->mark_chunk;
        t->chunk_left = t->mark_left;
    }
    t->bpacked = false;                            // (the packed W^T lives in this pass's scratch)
    hipStream_t st = static_cast<hipStream_t>(stream);
    HostScratch *hs;
    int rc = host_scratch(&hs);
    if (rc) return rc;
    const int64_t n = t->n;
    const int H = t->H;
    Bwd B;
    B.t = t;
    B.st = st;
    void *p;
    // ---- scratch
    if (hs->h_dev) {
        t->d_dots = hs->h_dev;
    } else {
        if ((rc = arena(t, (size_t)kDotSlots * 8 * sizeof(double), &p))) return rc;
        t->d_dots = static_cast<double *>(p);
    }
    if ((rc = arena(t, (size_t)rk_bwd_ws_bytes(), &t->d_bws))) return rc;
    if (!no_control) {
        if ((rc = arena(t, (size_t)linear_bwd_work_bytes(t->n_rows, H, H), &t->bwork))) return rc;
        B.gW_acc = g_W;
        B.gb_acc = g_b;
    }
    float *own_gk[7], *own_gy0, *own_gy1, *GU[8] = {}, *T, *CY[2], *CF[2];
    for (int j = 0; j < 7; ++j)
        if ((rc = panel(t, &own_gk[j]))) return rc;
    if ((rc = panel(t, &own_gy0)) || (rc = panel(t, &own_gy1)) || (rc = panel(t, &T))) return rc;
    for (int e = 2; e <= 7; ++e)
        if ((rc = panel(t, &GU[e]))) return rc;
    for (int q = 0; q < 2; ++q)
        if ((rc = panel(t, &CY[q])) || (rc = panel(t, &CF[q]))) return rc;
    if ((rc = panel(t, &B.tmpS)) || (rc = panel(t, &B.tmpG))) return rc;

    const float *Gy = nullptr, *Gf = nullptr;      // gradients of the state / its derivative as they stand behind the attempt being processed
    int pp = 0;
    double g_dt_next = 0.0, g_t = 0.0;             // adjoints of the step size / the time the NEXT attempt started from
    const float rtol = (float)t->rtol, atol = (float)t->atol;

    for (int s = (int)t->attempts.size() - 1; s >= 0; --s) {
        const Attempt &a = t->attempts[(size_t)s];
        if (a.thin) {
            // re-form u[2..6], k[1..5] and the S panels in the ring (where `a` points) by the forward's launches; y1 / k7 land in the
            // spare pair - an accepted attempt's kept pair, which the next attempt read in the forward pass, is what `a` points to
            StagePanels P = t->ring;
            const float *S_used[8];
            bool fused_err;
            rc = attempt_launches(t, a.y0, a.k[0], a.dts, P, S_used, &fused_err, t->d_red_rerun, true, a.ev0, st);
            if (rc) return rc;
        }
        int slot = 0;
        if (hs->h_dev) rec_arm(hs->h, kDotSlots * 8);
        auto dots_at = [&](int sl) { return t->d_dots + 8 * sl; };
        // ---- scalar chain, part 1: the error ratio's gradient comes from the NEXT step size (misc.py:160-170)
        double g_dt = 0.0;                         // adjoint of this attempt's dt (float64)
        float g_r = 0.f;
        if (a.ratio == 0.f) {
            g_dt += g_dt_next * t->ifactor;
        } else {
            g_dt += g_dt_next / a.factor;
            const double g_factor = -g_dt_next * a.dt / (a.factor * a.factor);
            const StepFactor sf = step_factor(a.ratio, t->safety, t->ifactor, t->dfactor);
            const double er = sf.er, expo = kStepExpo, Bv = sf.b, Cv = sf.c, Av = sf.a;
            const double inner = nan_min(Bv, Cv);
            // torch.max(A, min(B, C)): maximum / minimum split the gradient evenly on ties
            const double share_inner = half_on_tie_gt(inner, Av);
            const double share_B = Bv < Cv ? 1.0 : (Bv == Cv ? 0.5 : 0.0);
            const double g_B = g_factor * share_inner * share_B;
            const double g_er = g_B * expo * pow(er, expo - 1.0) / t->safety;
            g_r = (float)g_er * (0.5f / sqrtf(a.ratio));         // sqrt's backward in the ratio's float32
        }
        // ---- received gradients
        const float *cur_gk[7] = {}, *cur_gy0 = nullptr, *cur_gy1 = nullptr;
        if (a.accept) {
            cur_gy1 = Gy;
            cur_gk[6] = Gf;
        } else {
            cur_gy0 = Gy;
            cur_gk[0] = Gf;
        }
        // ---- dense output of the ticks this step covers (interp.py:21-65)
        // (a step that covers more ticks than the slots hold - a dense time grid over a long accepted step - hands its inner products
        // over in batches: read, added to the scalar adjoints, slots re-armed)
        double g_dts = 0.0;                        // adjoint of the float32 step size dts = float(dt)
        double g_a0 = 0.0, g_a1 = 0.0;
        int dense_slot[kDenseBatch], dense_group[kDenseBatch], n_dense = 0;
        auto take_dense = [&](const double *h) {
            for (int di = 0; di < n_dense; ++di) {
                const DenseGroup &g = t->groups[(size_t)dense_group[di]];
                const double *d = h + 8 * dense_slot[di];
                g_dts += (double)(float)d[7];
                const float w = g.a1 - g.a0;
                for (int q = 0; q < g.nt; ++q) {
                    const float gx = (float)d[q];
                    // x = (at - a0) / (a1 - a0):  dx/da0 = (x - 1) / (a1 - a0),  dx/da1 = -x / (a1 - a0)
                    g_a0 += (double)(gx * ((g.x[q] - 1.f) / w));
                    g_a1 += (double)(gx * (-g.x[q] / w));
                }
            }
            n_dense = 0;
        };
        for (int gi = (int)a.dense.size() - 1; gi >= 0; --gi) {
            const DenseGroup &g = t->groups[(size_t)a.dense[(size_t)gi]];
            const float *hg[7];
            for (int q = 0; q < g.nt; ++q) hg[q] = g_out + (size_t)g.tick[q] * n;
            if (n_dense == kDenseBatch) {
                rc = fetch(t, t->d_dots, 8 * slot, st, hs);
                if (rc) return rc;
                take_dense(hs->h);
                slot = 0;
                if (hs->h_dev) rec_arm(hs->h, kDotSlots * 8);
            }
            rc = rk_dense_bwd_multi_f32(hg, g.nt, a.y0, a.u[7], a.k, a.dts, g.x, own_gy0, own_gy1, own_gk, cur_gy0, cur_gy1, cur_gk,
                                        dots_at(slot), t->d_bws, n, st);
            if (rc) return rc;
            dense_group[n_dense] = a.dense[(size_t)gi];
            dense_slot[n_dense++] = slot++;
            cur_gy0 = own_gy0;
            cur_gy1 = own_gy1;
            for (int j = 0; j < 7; ++j) cur_gk[j] = own_gk[j];
        }
        // ---- error ratio (misc.py:146-157)
        int err_slot = -1, err_idx[8], err_m = 0;
        float err_c[8];
        if (g_r != 0.f) {
            const float *kp[8];
            float *hgk[8];
            const float *hacc[8];
            err_m = dt_terms(a.dts, kCErr, 7, a.k, kp, err_c, err_idx);
            for (int q = 0; q < err_m; ++q) {
                hgk[q] = own_gk[err_idx[q]];
                hacc[q] = cur_gk[err_idx[q]];
            }
            err_slot = slot++;
            rc = rk_error_bwd_f32(a.y0, a.u[7], kp, err_c, err_m, rtol, atol, g_r, 1.0 / (double)n, own_gy0, own_gy1, hgk, cur_gy0, cur_gy1,
                                  hacc, dots_at(err_slot), t->d_bws, n, st);
            if (rc) return rc;
            cur_gy0 = own_gy0;
            cur_gy1 = own_gy1;
            for (int q = 0; q < err_m; ++q) cur_gk[err_idx[q]] = own_gk[err_idx[q]];
        }
        // ---- evaluations 7 .. 2 and the stage sums, pull form
        const float *gu[8] = {};
        {
            const float *g7 = cur_gk[6];
            if (g7) {
                rc = rhs_vjp(B, a.u[7], a.k[6], g7, GU[7], a.S[7]);
                if (rc) return rc;
                if (cur_gy1) {
                    if ((rc = add_into(GU[7], cur_gy1, n, st))) return rc;     // gx + what y1 received (a + b in float32: order-free)
                }
                gu[7] = GU[7];
            } else {
                gu[7] = cur_gy1;
            }
        }
        int row_slot[8];
        for (int m = 2; m <= 7; ++m) row_slot[m] = -1;
        for (int e = 6; e >= 1; --e) {
            // total gradient of k_e: received + sum_{m' > e} dt beta[m' - 2][e - 1] g_u_m', and the step size through stage sum
            // m = e + 1 (all its g_u is known now): <g_u_m, u_m - y0> / dt
            const int m = e + 1;
            const float *pp_[8];
            float cc_[8];
            int np = 0;
            for (int m2 = e + 1; m2 <= 7; ++m2) {
                pp_[np] = gu[m2];
                cc_[np] = a.dts * (float)kBeta[m2 - 2][e - 1];
                ++np;
            }
            float *dst = (e == 1) ? CF[1 - pp] : T;
            const float *tot;
            bool premasked = false;
            if (gu[m]) {
                // one pass: the sum, the ReLU mask of evaluation e (none for k_1: that evaluation belongs to the previous attempt), the product
                const float *kp[8];
                float cp[8];
                int mm = 0;
                for (int q = 0; q < np; ++q)
                    if (pp_[q] && cc_[q] != 0.f) { kp[mm] = pp_[q]; cp[mm] = cc_[q]; ++mm; }
                const float *mask = (e > 1 && (t->flags & NDCN_F_RELU)) ? a.k[e - 1] : nullptr;
                row_slot[m] = slot++;
                rc = rk_pull_f32(dst, cur_gk[e - 1], kp, cp, mm, mask, a.u[m], a.y0, dots_at(row_slot[m]), t->d_bws, n, st);
                if (rc) return rc;
                tot = dst;
                premasked = mask != nullptr;
            } else {                                              // stage sum m received nothing: no step-size term, the sum alone
                rc = gather_sum(t, dst, cur_gk[e - 1], pp_, cc_, np, st, &tot, e == 1);
                if (rc) return rc;
            }
            if (e == 1) {
                Gf = tot;
                break;
            }
            if (tot) {
                rc = rhs_vjp(B, a.u[e], a.k[e - 1], tot, GU[e], a.S[e], premasked);
                if (rc) return rc;
                gu[e] = GU[e];
            }
        }
        {
            const float *pp_[8];
            float cc_[8];
            int np = 0;
            for (int m2 = 2; m2 <= 7; ++m2) {
                pp_[np] = gu[m2];
                cc_[np] = 1.f;
                ++np;
            }
            const float *tot;
            rc = gather_sum(t, CY[1 - pp], cur_gy0, pp_, cc_, np, st, &tot, true);
            if (rc) return rc;
            Gy = tot;
        }
        pp = 1 - pp;
        // ---- scalar chain, part 2: one read of the attempt's inner products
        if (slot > 0) {
            rc = fetch(t, t->d_dots, 8 * slot, st, hs);
            if (rc) return rc;
            const double *h = hs->h;
            take_dense(h);
            if (err_slot >= 0) {
                const double *d = h + 8 * err_slot;
                for (int q = 0; q < err_m; ++q) g_dts += (double)((float)((double)g_r * d[q]) * (float)kCErr[err_idx[q]]);
            }
            for (int m = 2; m <= 7; ++m)
                if (row_slot[m] >= 0) g_dts += (double)(float)(h[8 * row_slot[m]] / (double)a.dts);
        }
        g_dt += g_dts;
        double g_t0 = g_t;                         // t_next = t0 (+ dt): the time passes through
        if (a.accept) {
            g_dt += g_t + g_a1;                    // t_hi = t0 + dt feeds the next attempt's t0 and the abscissae's a1
            g_t0 += g_a1 + g_a0;
        }
        g_t = g_t0;
        g_dt_next = g_dt;
    }

    // ---- the initial step and the first evaluation (misc.py:84-143, dopri5.py:76-83)
    // gradients so far: Gy (state the first attempt started from), Gf (its derivative f0), g_dt_next (the initial step size)
    const float *acc_y = Gy;                       // everything y0 receives is added up in `accY`
    float *accY = own_gy0, *accF = own_gk[0];
    const float *acc_f = Gf;
    auto add_y = [&](const float *x) -> int {
        if (!x) return NDCN_OK;
        const float *kp[1] = {x};
        const float one[1] = {1.f};
        int r = rk_combine_f32(accY, acc_y, kp, one, 1, n, st);      // (acc_y null: a copy)
        acc_y = accY;
        return r;
    };
    auto add_f = [&](const float *x, float c) -> int {
        if (!x) return NDCN_OK;
        const float *kp[1] = {x};
        const float cc[1] = {c};
        int r = rk_combine_f32(accF, acc_f, kp, cc, 1, n, st);
        acc_f = accF;
        return r;
    };
    if ((rc = add_y(g_out))) return rc;            // the trajectory's first tick IS y0
    if (!t->first_given && g_dt_next != 0.0) {
        const float g_dt0 = (float)g_dt_next;      // dt = min(100 h0, h1).to(float64)
        const float h100 = 100.f * t->h0;
        const float g_h100 = g_dt0 * (float)(h100 < t->h1 ? 1.0 : (h100 == t->h1 ? 0.5 : 0.0));
        const float g_h1 = g_dt0 * (float)(t->h1 < h100 ? 1.0 : (h100 == t->h1 ? 0.5 : 0.0));
        float g_h0 = 100.f * g_h100;
        float g_d1 = 0.f, g_d2 = 0.f;
        if (t->h1_alt) {
            const float b1 = t->h0 * 1e-3f;
            g_h0 += 1e-3f * g_h1 * (float)half_on_tie_gt((double)b1, (double)1e-6f);
        } else {
            float m;
            const float av = initial_h1_base(t->d1, t->d2, &m);
            const float g_av = g_h1 * (float)(0.2 * pow((double)av, 0.2 - 1.0));
            const float g_m = -g_av * 0.01f / (m * m);
            if (t->d1 >= t->d2) g_d1 += g_m;
            else g_d2 += g_m;
        }
        // d2 = rms(f1 - f0 over scale(y0)) / h0
        const float g_rms2 = g_d2 / t->h0;
        g_h0 += -g_d2 * t->d2r / (t->h0 * t->h0);
        float *ga = own_gk[1], *gb_ = own_gk[2], *gy = own_gk[3], *gyh = own_gk[4];
        bool have_yh = false;
        if (g_rms2 != 0.f && t->s2 > 0) {
            const float coef = (float)((double)g_rms2 / (sqrt(t->s2) * sqrt((double)n)));
            rc = rk_rms_bwd_f32(t->f1, t->f0, t->y_in, rtol, atol, coef, ga, gb_, gy, n, st);
            if (rc) return rc;
            if ((rc = add_f(gb_, 1.f)) || (rc = add_y(gy))) return rc;
            // f1 = f(y0 + h0 f0)
            rc = rhs_vjp(B, t->yh, t->f1, ga, gyh);
            if (rc) return rc;
            have_yh = true;
        }
        if (have_yh) {
            if (hs->h_dev) rec_arm(hs->h, 8);
            rc = rk_dot_diff_f32(gyh, t->f0, nullptr, t->d_dots, t->d_bws, n, st);
            if (rc) return rc;
            rc = fetch(t, t->d_dots, 8, st, hs);
            if (rc) return rc;
            g_h0 += (float)hs->h[0];
            if ((rc = add_y(gyh)) || (rc = add_f(gyh, t->h0))) return rc;
        }
        float g_d0 = 0.f;
        if (!t->h0_const) {
            g_d0 = g_h0 * 0.01f / t->d1;
            g_d1 += -g_h0 * 0.01f * t->d0 / (t->d1 * t->d1);
        }
        if (g_d1 != 0.f && t->s1 > 0) {
            const float coef = (float)((double)g_d1 / (sqrt(t->s1) * sqrt((double)n)));
            rc = rk_rms_bwd_f32(t->f0, nullptr, t->y_in, rtol, atol, coef, ga, nullptr, gy, n, st);
            if (rc) return rc;
            if ((rc = add_f(ga, 1.f)) || (rc = add_y(gy))) return rc;
        }
        if (g_d0 != 0.f && t->s0 > 0) {
            const float coef = (float)((double)g_d0 / (sqrt(t->s0) * sqrt((double)n)));
            rc = rk_rms_bwd_f32(t->y_in, nullptr, t->y_in, rtol, atol, coef, ga, nullptr, gy, n, st);
            if (rc) return rc;
            if ((rc = add_y(ga)) || (rc = add_y(gy))) return rc;
        }
    }
    // f0 = f(y0)
    if (acc_f) {
        rc = rhs_vjp(B, t->y_in, t->f0, acc_f, own_gk[5]);
        if (rc) return rc;
        if ((rc = add_y(own_gk[5]))) return rc;
    }
    if (acc_y) NDCN_HIP(hipMemcpyAsync(g_y0, acc_y, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    else NDCN_HIP(hipMemsetAsync(g_y0, 0, (size_t)n * sizeof(float), st));
    if (!no_control && !B.have_w) {
        NDCN_HIP(hipMemsetAsync(g_W, 0, (size_t)H * H * sizeof(float), st));
        if (g_b) NDCN_HIP(hipMemsetAsync(g_b, 0, (size_t)H * sizeof(float), st));
    }
    return NDCN_OK;
}


// ====================================================================================================== fixed grids
// FixedGridODESolver.integrate (solvers.py:79-99; fixed_grid.py:7-29, rk_common.py:72-78) over ODEFunc, differentiated as the drivers
// train (heat_dynamics.py:313-334: plain backpropagation through every step), as two calls.  The launches and their order are those of
// _impl/fixed_train.py::_FixedGridSolve (kept as the A/B partner: results are bit-identical): forward - every evaluation carries the stage
// algebra that consumes it in its epilogue (ndcn_rhs_rk_f32), only the trajectory is kept; backward - per step, in reverse: the stages
// re-formed from the stored state by the same launches, then the closed-form VJPs (S = A u, the masked Linear backward, A^T with the
// step's factor folded into alpha) and the stage recurrences as one linear-combination launch each.  README-sized RK4 training was 34 ms
// per Adam step in the interpreter's hands (320 evaluations forward, 640 launches backward), midpoint 17 ms.

namespace {

struct Fixed {
    ndcn_tape t;                       // arena + operator + weights (no attempts)
    hipStream_t st;
    int method;
};

int fixed_init(Fixed &F, const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H, uint32_t flags, int method,
               ndcn_alloc_fn alloc, void *alloc_ctx, void *stream) {
    ndcn_tape &t = F.t;
    t.A = *A;
    if (At) t.At = *At;
    t.W = W;
    t.b = b;
    t.H = H;
    t.flags = flags;
    t.n_rows = A->n_rows;
    t.n = A->n_rows * (int64_t)H;
    t.alloc = alloc;
    t.alloc_ctx = alloc_ctx;
    t.panel_bytes = (size_t)t.n * sizeof(float) + 16;
    F.st = static_cast<hipStream_t>(stream);
    F.method = method;
    const int64_t wb = rhs_work_bytes(t.n_rows, H, flags);
    if (wb > 0) {
        void *p;
        int rc = arena(&t, (size_t)wb, &p);
        if (rc) return rc;
        t.work = static_cast<float *>(p);
        if (H == 256 && !(flags & (NDCN_F_NO_GRAPH | NDCN_F_NO_CONTROL))) {
            if ((rc = pack_weight_256(W, t.work, F.st))) return rc;
            t.packed = true;
        }
    }
    return NDCN_OK;
}

// one step from y into out_y; u / K (nullable arrays of 4): the stage inputs and derivatives, in caller-provided panels
// last_k: the step's last stage derivative is wanted too (the reverse pass needs its sign pattern; the forward pass does not)
int fixed_step(Fixed &F, const float *y, float dt, float *out_y, float *const *u, float *const *K, bool last_k = true) {
    ndcn_tape *t = &F.t;
    const uint32_t fl = eval_flags(t);
    auto eval = [&](const float *x, float *k, int mode, const float *const *kp, const float *cp, int n_prev, float *y_next, bool need_k = true) {
        RkOpt opt = {};
        opt.no_k = need_k ? 0 : 1;
        return rhs_rk_f32(&t->A, x, nullptr, t->A.n_cols, t->W, t->b, k, t->work, t->H, fl, mode, y, kp, cp, n_prev, y_next, 0.f, 0.f, nullptr,
                          nullptr, F.st, need_k ? nullptr : &opt);
    };
    if (F.method == NDCN_M_EULER) {
        const float c[1] = {dt};
        return eval(y, K[0], NDCN_RK_COMBINE, nullptr, c, 0, out_y, last_k);          // y + dt k1
    }
    if (F.method == NDCN_M_MIDPOINT) {
        const float c1[1] = {(float)((double)dt / 2.0)}, c2[1] = {dt};
        int rc = eval(y, K[0], NDCN_RK_COMBINE, nullptr, c1, 0, u[1]);               // ym = y + k1 dt / 2
        if (rc) return rc;
        return eval(u[1], K[1], NDCN_RK_COMBINE, nullptr, c2, 0, out_y, last_k);      // y + dt k2
    }
    const float c[1] = {dt};
    const float *x = y;
    for (int i = 0; i < 4; ++i) {
        const float *kp[3] = {K[0], K[1], K[2]};
        int rc = eval(x, K[i], NDCN_RK_RK4, kp, c, i, i == 3 ? out_y : u[i + 1], i < 3 || last_k);
        if (rc) return rc;
        x = u[i + 1 < 4 ? i + 1 : 3];
    }
    return NDCN_OK;
}

}  // namespace

int ndcn_fixed_grid_train_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, int method, const float *y0,
                              const float *h_dt, int64_t n_ticks, float *out, ndcn_alloc_fn alloc, void *alloc_ctx, void *stream) {
    NDCN_CHECK_ARG(A && y0 && h_dt && n_ticks >= 1 && out && alloc && H > 0, "bad argument");
    NDCN_CHECK_ARG(method == NDCN_M_EULER || method == NDCN_M_MIDPOINT || method == NDCN_M_RK4, "method must be euler, midpoint or rk4");
    NDCN_CHECK_ARG((flags & NDCN_F_NO_CONTROL) || W, "weight missing");
    Fixed F;
    int rc = fixed_init(F, A, nullptr, W, b, H, flags, method, alloc, alloc_ctx, stream);
    if (rc) return rc;
    float *u[4] = {}, *K[4] = {};
    for (int i = 0; i < 4; ++i)
        if ((rc = panel(&F.t, &u[i])) || (rc = panel(&F.t, &K[i]))) return rc;
    const int64_t n = F.t.n;
    NDCN_HIP(hipMemcpyAsync(out, y0, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, F.st));
    for (int64_t i = 0; i < n_ticks; ++i)
        if ((rc = fixed_step(F, out + (size_t)i * n, h_dt[i], out + (size_t)(i + 1) * n, u, K, false))) return rc;
    return NDCN_OK;
}

}  // extern "C"

namespace {

// Where the reverse sweep takes a tick's gradient from: the (n_ticks + 1, N, H) tensor g_out itself, or - the decoder inside the
// sweep - the (n_ticks + 1, N, C) gradient of the decoded ticks, turned into g_dec[i] . Wd where the sweep adds it (readout_bwd.hip)
struct TickGrad {
    const float *g_out = nullptr;
    const float *g_dec = nullptr, *Wd = nullptr;
    int C = 0;
    float *g_Wd = nullptr, *g_bd = nullptr;       // both nullable: the decoder's own gradients are not wanted
};

int fixed_backward(const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H, uint32_t flags, int method,
                   const float *traj, const TickGrad &tg, const float *h_dt, int64_t n_ticks, float *g_y0, float *g_W,
                   float *g_b, ndcn_alloc_fn alloc, void *alloc_ctx, void *stream) {
    const float *g_out = tg.g_out;
    NDCN_CHECK_ARG(A && traj && h_dt && n_ticks >= 1 && g_y0 && alloc && H > 0, "bad argument");
    NDCN_CHECK_ARG(method == NDCN_M_EULER || method == NDCN_M_MIDPOINT || method == NDCN_M_RK4, "method must be euler, midpoint or rk4");
    const bool no_graph = flags & NDCN_F_NO_GRAPH, no_control = flags & NDCN_F_NO_CONTROL;
    NDCN_CHECK_ARG(no_graph || At, "the transposed operator is required");
    NDCN_CHECK_ARG(no_control || (W && g_W && (g_b || !b)), "weight / g_W / g_b missing");
    Fixed F;
    int rc = fixed_init(F, A, At, W, b, H, flags, method, alloc, alloc_ctx, stream);
    if (rc) return rc;
    ndcn_tape *t = &F.t;
    hipStream_t st = F.st;
    const int64_t n = t->n;
    void *p;
    if (!no_control) {
        if ((rc = arena(t, (size_t)linear_bwd_work_bytes(t->n_rows, H, H), &t->bwork))) return rc;
        NDCN_HIP(hipMemsetAsync(g_W, 0, (size_t)H * H * sizeof(float), st));
        if (g_b) NDCN_HIP(hipMemsetAsync(g_b, 0, (size_t)H * sizeof(float), st));
    }
    float *u[4] = {}, *K[4] = {}, *gu[4] = {}, *a2[2], *gk, *tmpS, *tmpG, *scratch;
    for (int i = 0; i < 4; ++i)
        if ((rc = panel(t, &u[i])) || (rc = panel(t, &K[i])) || (rc = panel(t, &gu[i]))) return rc;
    if ((rc = panel(t, &a2[0])) || (rc = panel(t, &a2[1])) || (rc = panel(t, &gk)) || (rc = panel(t, &tmpS)) || (rc = panel(t, &tmpG)) ||
        (rc = panel(t, &scratch)))
        return rc;
    // alpha J(x)^T g for K = relu(W (A x) + b) into out (fixed_train.py: _vjp); g_W / g_b += scale * (this evaluation's)
    auto vjp = [&](const float *x, const float *Kx, const float *g, float alpha, float scale, float *out) -> int {
        return rhs_vjp_f32(&t->A, &t->At, x, Kx, g, t->W, nullptr, out, g_W, t->b ? g_b : nullptr, tmpS, tmpG, t->bwork, H, flags, false,
                           scale, alpha, true, false, &t->bpacked, st);                       // gW_tot.add_(gW, alpha = scale)
    };
    auto lincomb = [&](float *out, const float *y0p, std::initializer_list<const float *> ks, std::initializer_list<float> cs) -> int {
        const float *kp[8];
        float cp[8];
        int m = 0;
        for (const float *k : ks) kp[m++] = k;
        m = 0;
        for (float c : cs) cp[m++] = c;
        return rk_combine_f32(out, y0p, kp, cp, m, n, st);
    };
    // the tick gradient source: tick(out, a, addends, i) = a + sum(addends) + (gradient of tick i), the sweep's last combination
    double *dacc = nullptr;
    void *dws = nullptr;
    const int64_t n_dec = (int64_t)t->n_rows * tg.C;
    if (tg.g_dec) {
        if (tg.g_Wd) {
            if ((rc = arena(t, (size_t)((int64_t)tg.C * H + tg.C) * sizeof(double), &p))) return rc;
            dacc = static_cast<double *>(p);
            NDCN_HIP(hipMemsetAsync(dacc, 0, (size_t)((int64_t)tg.C * H + tg.C) * sizeof(double), st));
            if ((rc = arena(t, (size_t)readout_bwd_ws_bytes(t->n_rows, H, tg.C), &dws))) return rc;
        }
    }
    auto tick = [&](float *out, const float *base, std::initializer_list<const float *> adds, int64_t i) -> int {
        if (!tg.g_dec) {
            const float *kp[8];
            float cp[8];
            int m = 0;
            for (const float *k : adds) { kp[m] = k; cp[m++] = 1.f; }
            kp[m] = g_out + (size_t)i * n;
            cp[m++] = 1.f;
            return rk_combine_f32(out, base, kp, cp, m, n, st);
        }
        const float *ap[5];
        int m = 0;
        for (const float *k : adds) ap[m++] = k;
        return readout_bwd_f32(out, base, ap, m, tg.g_dec + (size_t)i * n_dec, tg.Wd, traj + (size_t)i * n, t->n_rows, H, tg.C, dacc, dws, st);
    };
    const float *a;
    int pp = 0;
    if (tg.g_dec) {                                           // the seed: the last tick's gradient by the kernel into a panel
        if ((rc = tick(a2[1], nullptr, {}, n_ticks))) return rc;
        a = a2[1];
    } else {
        a = g_out + (size_t)n_ticks * n;
    }
    for (int64_t i = n_ticks - 1; i >= 0; --i) {
        const float dt = h_dt[i];
        const float *y = traj + (size_t)i * n;
        u[0] = const_cast<float *>(y);
        if ((rc = fixed_step(F, y, dt, scratch, u, K))) return rc;
        float *a_new = a2[pp];
        if (method == NDCN_M_EULER) {                         // y1 = y + dt k1
            if ((rc = vjp(y, K[0], a, dt, dt, gu[0]))) return rc;
            rc = tick(a_new, a, {gu[0]}, i);
        } else if (method == NDCN_M_MIDPOINT) {               // ym = y + (dt / 2) k1 ; y1 = y + dt k2
            const float h = (float)((double)dt / 2.0);
            if ((rc = vjp(u[1], K[1], a, dt, dt, gu[1]))) return rc;          // dL / d ym
            if ((rc = vjp(y, K[0], gu[1], h, h, gu[0]))) return rc;
            rc = tick(a_new, a, {gu[1], gu[0]}, i);
        } else {                                              // the 3/8 rule, rk_common.py:72-78
            const float c8 = (float)((double)dt / 8.0), c38 = (float)(3.0 * (double)c8), d3 = (float)((double)dt / 3.0);
            if ((rc = vjp(u[3], K[3], a, c8, c8, gu[3]))) return rc;          // J4^T (c8 a)
            if ((rc = lincomb(gk, nullptr, {a, gu[3]}, {c38, dt}))) return rc;
            if ((rc = vjp(u[2], K[2], gk, 1.f, 1.f, gu[2]))) return rc;
            if ((rc = lincomb(gk, nullptr, {a, gu[3], gu[2]}, {c38, -dt, dt}))) return rc;
            if ((rc = vjp(u[1], K[1], gk, 1.f, 1.f, gu[1]))) return rc;
            if ((rc = lincomb(gk, nullptr, {a, gu[3], gu[2], gu[1]}, {c8, dt, -d3, d3}))) return rc;
            if ((rc = vjp(y, K[0], gk, 1.f, 1.f, gu[0]))) return rc;
            rc = tick(a_new, a, {gu[3], gu[2], gu[1], gu[0]}, i);
        }
        if (rc) return rc;
        a = a_new;
        pp = 1 - pp;
    }
    NDCN_HIP(hipMemcpyAsync(g_y0, a, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (dacc) return readout_bwd_finish_f32(dacc, tg.g_Wd, tg.g_bd, H, tg.C, st);
    return NDCN_OK;
}

}  // namespace

extern "C" {

int ndcn_fixed_grid_backward_f32(const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H, uint32_t flags, int method,
                                 const float *traj, const float *g_out, const float *h_dt, int64_t n_ticks, float *g_y0, float *g_W,
                                 float *g_b, ndcn_alloc_fn alloc, void *alloc_ctx, void *stream) {
    NDCN_CHECK_ARG(g_out, "bad argument");
    TickGrad tg;
    tg.g_out = g_out;
    return fixed_backward(A, At, W, b, H, flags, method, traj, tg, h_dt, n_ticks, g_y0, g_W, g_b, alloc, alloc_ctx, stream);
}

int ndcn_fixed_grid_backward_readout_f32(const ndcn_csr *A, const ndcn_csr *At, const float *W, const float *b, int H, uint32_t flags,
                                         int method, const float *traj, const float *g_dec, const float *Wd, int C, const float *h_dt,
                                         int64_t n_ticks, float *g_y0, float *g_W, float *g_b, float *g_Wd, float *g_bd,
                                         ndcn_alloc_fn alloc, void *alloc_ctx, void *stream) {
    NDCN_CHECK_ARG(g_dec && Wd && (g_Wd || !g_bd), "bad argument");
    if (!readout_bwd_supported(H, C)) { set_error("%s: 1 <= C <= 15 is supported (C = %d)", __func__, C); return NDCN_EINVAL; }
    TickGrad tg;
    tg.g_dec = g_dec;
    tg.Wd = Wd;
    tg.C = C;
    tg.g_Wd = g_Wd;
    tg.g_bd = g_bd;
    return fixed_backward(A, At, W, b, H, flags, method, traj, tg, h_dt, n_ticks, g_y0, g_W, g_b, alloc, alloc_ctx, stream);
}

}  // extern "C"
