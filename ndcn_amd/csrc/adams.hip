// explicit_adams: the reference's AdamsBashforth (torchdiffeq/_impl/fixed_adams.py:151-211) - a fixed-grid linear multistep method that
// is warmed up by two RK4 (3/8 rule) steps and then makes ONE right-hand-side evaluation per step.
//
//   ab_step_f32                      out = y + dt * sum_{i<n} a_i f_i, n = 3..11: one streaming pass over the history
//   ndcn_solve_explicit_adams_f32    the whole solve over ODEFunc, enqueued on the caller's stream: history ring, stage panels and both
//                                    state panels in a caller-owned workspace, nothing read back
//   ndcn_solve_fixed_adams_f32       the same loop with the Adams-Moulton corrector of fixed_adams (its two passes: adams_pc.hip) iterated per
//                                    step; one 8-byte read-back per iteration - the host decides whether to iterate again
//   (ab_step_readout_f32             ab_step_f32 that decodes the new state with a Linear(H, C) in the same pass: adams_readout.hip)
//   ndcn_solve_*_adams_readout_f32   the two solves with that decoder: `out` holds decoded ticks, the state never leaves the workspace
//   ndcn_explicit_adams_train_f32    the same loop (adams_run) writing every evaluation and every state into a caller-owned record: the
//                                    forward pass of training (the reverse sweep: adams_bwd.hip, fixed_train.py)
//   ndcn_fixed_adams_train_f32       the corrector loop with that record AND, per corrector evaluation, the pair (iterate, evaluation) in
//                                    caller-owned slots handed out in order - NDCN_ECAPACITY before a slot past `cap` is touched
//
// Rounding follows the reference term by term (fixed_adams.py:182, misc.py:22-25, solvers.py:92): p_i = a_i * f_i, s = ((0 + p_0) + p_1)
// + ..., dy = dt * s, y1 = y + dy - every product and sum rounded on its own.  FP contraction is therefore switched OFF for this
// translation unit, as in rk.hip, and the arithmetic is written with plain operators: hip's __fmul_rn / __fadd_rn are inline functions
// of a header that is compiled under the default mode (contract=fast) - inlined here they fuse (seen in the ISA: v_pk_fma_f32).
#include <stdint.h>

#include <vector>

#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "adams_step.h"

namespace ndcn {

namespace {

// Elements [head, head + 4 n4) by 16 bytes per lane - every panel is 16-byte aligned at element `head` -, the <= 3 elements in front and
// the <= 3 behind by single lanes (n4 = 0: everything, panels that do not share an offset).  A grid-stride loop: the host sizes the
// grid from the compute units, not from the panel.  The N loads of an item are issued before the first use (the loop over j is unrolled:
// N independent global_load_dwordx4, one s_waitcnt per consumer); default cache policy - the next step reads N - 1 of the panels again.
template <int N>
__global__ __launch_bounds__(256) void ab_step_kernel(AbArgs p, int64_t head, int64_t n4, int64_t n) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < n4; i += stride) {
        const int64_t e = head + 4 * i;
        float4 v[N];
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = *reinterpret_cast<const float4 *>(p.f[j] + e);
        const float4 y = *reinterpret_cast<const float4 *>(p.y + e);
        float fx[N], fy[N], fz[N], fw[N];
#pragma unroll
        for (int j = 0; j < N; ++j) { fx[j] = v[j].x; fy[j] = v[j].y; fz[j] = v[j].z; fw[j] = v[j].w; }
        float4 o;
        o.x = ab1(y.x, fx, p.a, N, p.dt);
        o.y = ab1(y.y, fy, p.a, N, p.dt);
        o.z = ab1(y.z, fz, p.a, N, p.dt);
        o.w = ab1(y.w, fw, p.a, N, p.dt);
        *reinterpret_cast<float4 *>(p.out + e) = o;
    }
    const int64_t rest = n - 4 * n4;
    for (int64_t r = tid; r < rest; r += stride) {
        const int64_t e = r < head ? r : r + 4 * n4;
        float f[N];
#pragma unroll
        for (int j = 0; j < N; ++j) f[j] = p.f[j][e];
        p.out[e] = ab1(p.y[e], f, p.a, N, p.dt);
    }
}

}  // namespace

// workgroups of a streaming launch: eight per compute unit (2048 on the whole chip), fewer when the panel is smaller (adams_bwd.hip
// sizes its launches with it too)
int ab_grid(int64_t items) {
    static std::atomic<int> cus_of[64];
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) {
        cus = cus_of[dev].load(std::memory_order_relaxed);
        if (cus == 0 && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            cus_of[dev].store(cus, std::memory_order_relaxed);
    }
    if (cus <= 0) cus = kCus;
    int64_t g = (items + 255) / 256;
    if (g > (int64_t)cus * 8) g = (int64_t)cus * 8;
    return g < 1 ? 1 : (int)g;
}

namespace {

template <int N>
void ab_launch(const AbArgs &p, int64_t head, int64_t n4, int64_t n, hipStream_t st) {
    const int64_t rest = n - 4 * n4;
    hipLaunchKernelGGL(ab_step_kernel<N>, dim3(ab_grid(n4 > rest ? n4 : rest)), dim3(256), 0, st, p, head, n4, n);
}

}  // namespace

int ab_step_f32(float *out, const float *y, const float *const *h_f, const float *h_a, int n_terms, float dt, int64_t n, hipStream_t st) {
    if (n_terms < kAbMinTerms || n_terms > kAbMaxTerms) { set_error("ab_step: %d terms, the orders are %d..%d", n_terms, kAbMinTerms, kAbMaxTerms); return NDCN_EINVAL; }
    if (!out || !y || !h_f || !h_a || n < 0) { set_error("ab_step: null argument"); return NDCN_EINVAL; }
    AbArgs p;
    p.y = y; p.out = out; p.dt = dt;
    const uintptr_t off = reinterpret_cast<uintptr_t>(out) & 15u;
    bool same_offset = (off & 3u) == 0 && (reinterpret_cast<uintptr_t>(y) & 15u) == off;
    for (int j = 0; j < kAbMaxTerms; ++j) {
        p.f[j] = h_f[j < n_terms ? j : 0];
        p.a[j] = j < n_terms ? h_a[j] : 0.f;
        if (j >= n_terms) continue;
        if (!h_f[j]) { set_error("ab_step: term %d is null", j); return NDCN_EINVAL; }
        if (h_f[j] == out) { set_error("ab_step: out aliases history panel %d (only y may be updated in place)", j); return NDCN_EINVAL; }
        same_offset = same_offset && (reinterpret_cast<uintptr_t>(h_f[j]) & 15u) == off;
    }
    if (n == 0) return NDCN_OK;
    int64_t head = 0, n4 = 0;
    if (same_offset) {
        head = (int64_t)((16u - off) & 15u) / 4;
        if (head > n) head = n;
        n4 = (n - head) / 4;
    }
    if (n4 == 0) head = 0;
    ProfScope prof(PROF_COMBINE, st, 4.0 * n * (n_terms + 2), 2.0 * n * (n_terms + 1));
    switch (n_terms) {
        case 3: ab_launch<3>(p, head, n4, n, st); break;
        case 4: ab_launch<4>(p, head, n4, n, st); break;
        case 5: ab_launch<5>(p, head, n4, n, st); break;
        case 6: ab_launch<6>(p, head, n4, n, st); break;
        case 7: ab_launch<7>(p, head, n4, n, st); break;
        case 8: ab_launch<8>(p, head, n4, n, st); break;
        case 9: ab_launch<9>(p, head, n4, n, st); break;
        case 10: ab_launch<10>(p, head, n4, n, st); break;
        default: ab_launch<11>(p, head, n4, n, st); break;
    }
    NDCN_LAUNCH_CHECK();
    return NDCN_OK;
}

namespace {

int64_t gcd64(int64_t a, int64_t b) {
    if (a < 0) a = -a;
    if (b < 0) b = -b;
    while (b) { const int64_t r = a % b; a = b; b = r; }
    return a;
}

// The weights of order k, newest evaluation first.  beta_i = integral_0^1 prod_{j != i, j < k} (u + j) / (j - i) du as an exact rational
// (k <= 11: every intermediate fits 64 bits - the polynomial's coefficients stay below 10!, lcm(1..11) = 27720), all of them over their
// least common denominator div: beta_i = c_i / div.  The reference multiplies each evaluation by (1 / div) * c_i, a Python double that
// torch rounds to the state dtype (fixed_adams.py:182, misc.py:25): a_i = (float)((1.0 / div) * c_i).
void ab_weights(int k, float *a) {
    int64_t num[kAbMaxTerms], den[kAbMaxTerms];
    int64_t L = 1;
    for (int m = 1; m <= k; ++m) L = L / gcd64(L, m) * m;
    for (int i = 0; i < k; ++i) {
        int64_t poly[kAbMaxTerms + 1] = {1};                 // prod_{j != i} (u + j), lowest power first
        int deg = 0;
        int64_t d = 1;
        for (int j = 0; j < k; ++j) {
            if (j == i) continue;
            for (int m = deg + 1; m >= 0; --m) poly[m] = (m ? poly[m - 1] : 0) + (int64_t)j * (m <= deg ? poly[m] : 0);
            ++deg;
            d *= j - i;
        }
        int64_t s = 0;                                       // L * integral of the polynomial
        for (int m = 0; m <= deg; ++m) s += poly[m] * (L / (m + 1));
        int64_t q = L * d;
        if (q < 0) { q = -q; s = -s; }
        const int64_t g = gcd64(s, q);
        num[i] = s / g;
        den[i] = q / g;
    }
    int64_t div = 1;
    for (int i = 0; i < k; ++i) div = div / gcd64(div, den[i]) * den[i];
    for (int i = 0; i < k; ++i) a[i] = (float)((1.0 / (double)div) * (double)(num[i] * (div / den[i])));
}

// The Adams-Moulton weights for a step that holds k evaluations: the formula over the k + 1 points t + dt, t, t - dt, ..,
// mu_i = integral_0^1 prod_{j != i, j <= k} (u + j - 1) / (j - i) du = c_i / div as above (k <= 11: a polynomial of degree 11 with
// coefficients below 11!, lcm(1..12) = 27720, div <= 958003200 - every intermediate fits 64 bits and every c_i a double exactly).
// m[i - 1] = (float)((1.0 / div) * c_i) for the history (fixed_adams.py:188); *lead = c_0 / div, the double the reference multiplies dt
// by (:193).
void am_weights(int k, float *m, double *lead) {
    constexpr int P = kAbMaxTerms + 1;
    int64_t num[P], den[P];
    int64_t L = 1;
    for (int q = 1; q <= k + 1; ++q) L = L / gcd64(L, q) * q;
    for (int i = 0; i <= k; ++i) {
        int64_t poly[P + 1] = {1};                           // prod_{j != i} (u + j - 1), lowest power first
        int deg = 0;
        int64_t d = 1;
        for (int j = 0; j <= k; ++j) {
            if (j == i) continue;
            for (int q = deg + 1; q >= 0; --q) poly[q] = (q ? poly[q - 1] : 0) + (int64_t)(j - 1) * (q <= deg ? poly[q] : 0);
            ++deg;
            d *= j - i;
        }
        int64_t s = 0;
        for (int q = 0; q <= deg; ++q) s += poly[q] * (L / (q + 1));
        int64_t den_i = L * d;
        if (den_i < 0) { den_i = -den_i; s = -s; }
        const int64_t g = gcd64(s, den_i);
        num[i] = s / g;
        den[i] = den_i / g;
    }
    int64_t div = 1;
    for (int i = 0; i <= k; ++i) div = div / gcd64(div, den[i]) * den[i];
    *lead = (double)(num[0] * (div / den[0])) / (double)div;
    for (int i = 1; i <= k; ++i) m[i - 1] = (float)((1.0 / (double)div) * (double)(num[i] * (div / den[i])));
}

// the corrector of fixed_adams: absent (nullptr) in the explicit solves
struct Corrector {
    float rtol, atol;
    int max_iters;
    int *h_iters, *h_converged;
    // with a record (training): corrector evaluation r of a step reads its iterate u_{r-1} from slot s of rec_u and writes F_r to slot s
    // of rec_c, s = h_slot[step] + r - 1; `cap` slots each, handed out in order
    float *rec_u = nullptr, *rec_c = nullptr;
    int64_t cap = 0;
    int64_t *h_slot = nullptr;
};

// the decoder Linear(H, C) of a solve that reports decoded ticks: `out` is then n_ticks panels of n_rows x C and no hidden tick is written
struct Decoder {
    const float *Wd, *bd;
    int C;
};

// an 8-byte pinned mirror of the device counter, owned by one solve
struct PinnedCount {
    unsigned long long *p = nullptr;
    ~PinnedCount() { if (p) (void)hipHostFree(p); }
};

inline size_t up256(size_t v) { return (v + 255u) & ~(size_t)255u; }

// panels of the workspace: k2..k4 of a warm-up step and the stage input - what a solve WITH a record needs besides the record -; a solve
// without one adds the history ring and two state panels
constexpr int kStagePanels = 3 + 1;
inline int solve_panels(int max_order) { return (max_order - 1) + kStagePanels + 2; }
constexpr int kCorrectorPanels = 3;    // dy, delta, the corrector's evaluation (the iterate is the new state's panel)
constexpr int kCorrectorRecPanels = 2; // with a record: dy and delta (iterates and evaluations stand in the caller's slots)
constexpr size_t kCounterBytes = 256;

inline int64_t workspace_need(int64_t n_rows, int H, int panels) {
    const size_t panel = up256((size_t)n_rows * (size_t)H * sizeof(float));
    const int64_t wb = rhs_work_bytes(n_rows, H, NDCN_F_RELU);
    return (int64_t)((size_t)panels * panel + up256((size_t)(wb > 0 ? wb : 0)));
}

// the record of the corrector's evaluations is full: nothing was enqueued for the slot that does not exist; what earlier steps enqueued
// runs to its end inside the caller's panels.  h_iters / h_converged / h_slot from `step` on are not written.
int slots_exhausted(const char *who, int64_t step, int64_t cap) {
    set_error("%s: grid step %lld needs more than the cap = %lld corrector evaluations of rec_u / rec_c; run again with cap = n_steps * max_iters",
              who, (long long)step, (long long)cap);
    return NDCN_ECAPACITY;
}

#define ADAMS_ARG(cond, msg)                                 \
    do {                                                      \
        if (!(cond)) {                                        \
            set_error("%s: %s", who, msg);                    \
            return NDCN_EINVAL;                               \
        }                                                     \
    } while (0)

// FixedGridODESolver.integrate with the AdamsBashforth step: the one loop behind both entry points (`who`: the caller's name in
// messages).  Without a record (rec_f == nullptr) the evaluations live in a ring of max_order - 1 workspace panels and the state
// alternates between two more, or stands in the caller's tick panel.  With one, evaluation i is written to panel i of rec_f and the
// state after step i to panel i of rec_y - the history of a step is then the panels i, i - 1, ... of rec_f and nothing else is kept:
// the same launches on the same values, only the addresses differ.  A corrector with a record (pc->rec_u) keeps every corrector evaluation
// too: the predictor writes the first iterate u_0 straight into the step's first slot of rec_u, evaluation r writes F_r into its slot of
// rec_c, abm_correct writes the new iterate into the state's panel, and only when another iteration follows is that panel copied into the
// next slot of rec_u - a step that iterates once copies nothing.  A slot past pc->cap: NDCN_ECAPACITY, before anything is enqueued for it.
int adams_run(const char *who, const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0, const float *h_dt,
              int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same, const float *h_tick_off, int64_t n_ticks, int max_order,
              float *out, float *rec_f, float *rec_y, void *workspace, int64_t workspace_bytes, hipStream_t st,
              const Corrector *pc = nullptr, const Decoder *dc = nullptr) {
    ADAMS_ARG(A && W && y0 && H > 0 && n_steps >= 0 && n_ticks >= 0, "null argument");
    ADAMS_ARG(A->n_rows >= 0 && A->n_rows < (1ll << 31) - 1 && A->nnz >= 0 && A->rowptr && (A->nnz == 0 || (A->colidx && A->val)), "bad operator");
    ADAMS_ARG(A->n_rows == A->n_cols, "an un-sharded solve: the operator must be square (no halo columns)");
    ADAMS_ARG(flags == NDCN_F_RELU, "flags must be NDCN_F_RELU: no_graph / no_control / packed / accumulate have no form here");
    ADAMS_ARG(max_order >= 2 && max_order <= kAbMaxOrder, "max_order must be 2..12 (fixed_adams.py:162 clamps at 12; below 2 the reference fails)");
    ADAMS_ARG(n_steps == 0 || h_dt, "step sizes missing");
    ADAMS_ARG(n_ticks == 0 || (h_tick_step && h_tick_same && h_tick_off && out), "tick arrays missing");
    for (int64_t j = 0; j < n_ticks; ++j)
        ADAMS_ARG(h_tick_step[j] >= (j ? h_tick_step[j - 1] : 0) && h_tick_step[j] < n_steps, "tick steps must be non-decreasing and below n_steps");
    const bool rec = rec_f != nullptr;
    ADAMS_ARG(!dc || (!rec && dc->Wd && interp_readout_supported(H, dc->C)),
              "the decoder needs 64 <= H <= 512 or H = 16, 20, .. 60, 1 <= C <= 15 and a solve without a record");
    ADAMS_ARG(!rec || n_steps == 0 || rec_y, "the record of the states is missing");
    ADAMS_ARG(!pc || (pc->max_iters >= 1 && (n_steps == 0 || (pc->h_iters && pc->h_converged))),
              "the corrector needs max_iters >= 1 and the two per-step host arrays");
    ADAMS_ARG(!pc || !rec || n_steps == 0 || (pc->rec_u && pc->rec_c && pc->h_slot && pc->cap >= 0),
              "a corrector with a record needs rec_u, rec_c, the per-step slot array and cap >= 0");
    const int64_t need = workspace_need(A->n_rows, H, rec ? kStagePanels + (pc ? kCorrectorRecPanels : 0)
                                                          : solve_panels(max_order) + (pc ? kCorrectorPanels : 0)) +
                         (pc ? (int64_t)kCounterBytes : 0);
    ADAMS_ARG(workspace && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0 && workspace_bytes >= need,
              "workspace of the size its host function returns, 256-byte aligned, required");
    const int64_t n = A->n_rows * (int64_t)H;
    if (n_steps == 0 || n == 0) return NDCN_OK;

    // the workspace: [ring |] k2 k3 k4 | stage input [| two state panels] | rhs scratch
    const size_t panel = up256((size_t)n * sizeof(float));
    char *base = static_cast<char *>(workspace);
    auto take = [&]() { float *p = reinterpret_cast<float *>(base); base += panel; return p; };
    const int ring_n = max_order - 1;
    float *ring[kAbMaxTerms] = {};
    for (int i = 0; i < ring_n && !rec; ++i) ring[i] = take();
    float *k2 = take(), *k3 = take(), *k4 = take(), *ytmp = take();
    float *state[2] = {nullptr, nullptr};
    if (!rec) { state[0] = take(); state[1] = take(); }
    float *dy = nullptr, *delta = nullptr, *fc = nullptr;
    unsigned long long *d_count = nullptr;
    PinnedCount h_count;
    if (pc) {
        dy = take(); delta = take();
        if (!rec) fc = take();
        d_count = reinterpret_cast<unsigned long long *>(base);
        base += kCounterBytes;
        NDCN_HIP(hipHostMalloc(reinterpret_cast<void **>(&h_count.p), sizeof(unsigned long long), hipHostMallocDefault));
    }
    float *work = rhs_work_bytes(A->n_rows, H, flags) > 0 ? reinterpret_cast<float *>(base) : nullptr;
    uint32_t fl = flags;
    if (work && rhs_fused_supported(H, flags) && rhs_fused2_supported(A, H, flags)) {
        // H = 256 on an operator with a row-group plan: the image of W once per solve, every evaluation reads it (rhs.hip)
        int rc = pack_weight_256(W, work, st);
        if (rc) return rc;
        fl |= NDCN_F_PACKED;
    }
    auto eval = [&](const float *x, float *k) { return rhs_f32(A, x, nullptr, A->n_cols, W, b, k, work, H, fl, st); };

    float weights[kAbMaxTerms + 1][kAbMaxTerms];
    for (int k = kAbMinTerms; k <= kAbMaxTerms && k <= ring_n; ++k) ab_weights(k, weights[k]);
    float moulton[kAbMaxTerms + 1][kAbMaxTerms];
    double lead[kAbMaxTerms + 1] = {};
    for (int k = kAbMinTerms; pc && k <= kAbMaxTerms && k <= ring_n; ++k) am_weights(k, moulton[k], &lead[k]);

    const float *y = y0;
    int held = 0, newest = -1;                                 // evaluations held; the ring slot of the newest
    int64_t j = 0;
    int64_t next_slot = 0;                                     // of rec_u / rec_c
    std::vector<float *> outs;
    std::vector<int> zeros;
    const size_t ostride = dc ? (size_t)A->n_rows * (size_t)dc->C : (size_t)n;      // of the caller's tick panels
    for (int64_t i = 0; i < n_steps; ++i) {
        const float dt = h_dt[i];
        int64_t j1 = j;
        while (j1 < n_ticks && h_tick_step[j1] == i) ++j1;
        // where the new state goes: its panel of the record; without one the caller's panel when the step's LAST tick is the state
        // itself (an end of the step; only the last tick of a step can be), else the state panel the step does not read
        // (with a decoder the caller's panels hold decoded ticks: the state stays in the workspace)
        float *dst = rec ? rec_y + (size_t)i * (size_t)n
                         : ((!dc && j1 > j && h_tick_same[j1 - 1]) ? out + (size_t)(j1 - 1) * (size_t)n : (y == state[0] ? state[1] : state[0]));
        int64_t decoded_to = j;                                // ticks [j, decoded_to) were decoded by the step's own launch
        // fixed_adams.py:166-173: the new evaluation takes the place of the oldest one (a record keeps them all)
        int rc;
        newest = (newest + 1) % ring_n;
        float *f_new = rec ? rec_f + (size_t)i * (size_t)n : ring[newest];
        if (held < ring_n) ++held;
        if ((rc = eval(y, f_new))) return rc;
        const int order = held;
        if (order < kAbMinTerms) {
            // rk_common.py:72-78 with k1 = the new evaluation: the un-fused RK4 step of the device solver (solver.hip: enqueue_fixed_stages)
            if ((rc = fixed_stage_f32(2, ytmp, y, f_new, nullptr, nullptr, nullptr, dt, n, st))) return rc;
            if ((rc = eval(ytmp, k2))) return rc;
            if ((rc = fixed_stage_f32(3, ytmp, y, f_new, k2, nullptr, nullptr, dt, n, st))) return rc;
            if ((rc = eval(ytmp, k3))) return rc;
            if ((rc = fixed_stage_f32(4, ytmp, y, f_new, k2, k3, nullptr, dt, n, st))) return rc;
            if ((rc = eval(ytmp, k4))) return rc;
            if ((rc = fixed_stage_f32(5, dst, y, f_new, k2, k3, k4, dt, n, st))) return rc;
            if (pc) { pc->h_iters[i] = 0; pc->h_converged[i] = 1; }
            if (pc && rec) pc->h_slot[i] = next_slot;          // (a warm-up step takes no slot)
        } else if (pc) {
            // fixed_adams.py:180-200: predictor and the corrector's explicit part in one pass, the iterate in the new state's panel;
            // then evaluate / correct / read the count back until no element fails or max_iters passes have run
            const float *f[kAbMaxTerms];
            for (int q = 0; q < order; ++q) f[q] = rec ? rec_f + (size_t)(i - q) * (size_t)n : ring[((newest - q) % ring_n + ring_n) % ring_n];
            if (rec) {
                pc->h_slot[i] = next_slot;
                if (next_slot >= pc->cap) return slots_exhausted(who, i, pc->cap);
            }
            // the iterate the next evaluation reads: the new state's panel, with a record the slot of that evaluation
            float *u = rec ? pc->rec_u + (size_t)next_slot * (size_t)n : dst;
            if ((rc = abm_predict_f32(dy, delta, u, y, f, weights[order], moulton[order], order, dt, n, st))) return rc;
            const float c0 = dt * (float)lead[order];          // torch: the double becomes a float32 scalar, then one float32 product
            int its = 0;
            bool converged = false;
            while (its < pc->max_iters && !converged) {
                float *fr = fc;
                if (rec) {
                    if (its > 0) {                             // another iteration: the iterate abm_correct left in dst enters its slot
                        if (next_slot >= pc->cap) return slots_exhausted(who, i, pc->cap);
                        u = pc->rec_u + (size_t)next_slot * (size_t)n;
                        NDCN_HIP(hipMemcpyAsync(u, dst, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
                    }
                    fr = pc->rec_c + (size_t)next_slot * (size_t)n;
                    ++next_slot;
                }
                if ((rc = eval(u, fr))) return rc;
                if ((rc = abm_correct_f32(dy, dst, fr, delta, y, c0, pc->rtol, pc->atol, n, d_count, st))) return rc;
                NDCN_HIP(hipMemcpyAsync(h_count.p, d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
                NDCN_HIP(hipStreamSynchronize(st));
                ++its;
                converged = *h_count.p == 0;
            }
            pc->h_iters[i] = its;
            pc->h_converged[i] = converged ? 1 : 0;
            if (!converged) --held;                            // :199: the oldest evaluation leaves the history
        } else {
            const float *f[kAbMaxTerms];
            for (int q = 0; q < order; ++q) f[q] = rec ? rec_f + (size_t)(i - q) * (size_t)n : ring[((newest - q) % ring_n + ring_n) % ring_n];
            if (dc && j1 > j) {
                // the step and the decode of its first <= 8 ticks in one launch: a coincident tick decodes the state (offset 0), a tick
                // inside the step the value of tick_emit_f32's expression
                float *decs[kDecMaxTicks];
                float tms[kDecMaxTicks];
                const int m = (int)(j1 - j < kDecMaxTicks ? j1 - j : kDecMaxTicks);
                for (int q = 0; q < m; ++q) {
                    decs[q] = out + (size_t)(j + q) * ostride;
                    tms[q] = h_tick_same[j + q] ? 0.f : h_tick_off[j + q];
                    if (!h_tick_same[j + q] && tms[q] == 0.f) tms[q] = dt;      // (the expression's value does not depend on the offset)
                }
                if ((rc = ab_step_readout_f32(dst, y, f, weights[order], order, dt, A->n_rows, H, dc->Wd, dc->bd, dc->C, decs, tms, m, st)))
                    return rc;
                g_last_readout_path |= NDCN_READOUT_ADAMS | (H < 64 ? NDCN_READOUT_NARROW : 0);
                decoded_to = j + m;
            } else if ((rc = ab_step_f32(dst, y, f, weights[order], order, dt, n, st))) {
                return rc;
            }
        }
        y = dst;
        if (dc) {
            // the ticks the step's launch did not decode (warm-up steps, the corrector's steps, a ninth tick): the state's panel through
            // the Linear - a tick inside the step through tick_emit_f32 into the stage input's panel, which no launch reads before the
            // next warm-up stage writes it
            for (int64_t q = decoded_to; q < j1; ++q) {
                const float *src = dst;
                if (!h_tick_same[q]) {
                    const int zero = 0;
                    float *const o1 = ytmp;
                    if ((rc = tick_emit_f32(dst, dt, &h_tick_off[q], &zero, &o1, 1, n, st))) return rc;
                    src = ytmp;
                }
                if ((rc = linear_f32(src, dc->Wd, dc->bd, out + (size_t)q * ostride, A->n_rows, H, dc->C, 0, st))) return rc;
                g_last_readout_path |= NDCN_READOUT_FIXED;
            }
            j = j1;
            continue;
        }
        // solvers.py:95-97: the ticks this step reports - the coincident one IS dst; the others pass through the reference's expression
        outs.clear();
        std::vector<float> tm;
        for (int64_t q = j; q < j1; ++q) {
            float *o = out + (size_t)q * (size_t)n;
            if (h_tick_same[q]) {
                if (o != dst) NDCN_HIP(hipMemcpyAsync(o, dst, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
            } else {
                outs.push_back(o);
                tm.push_back(h_tick_off[q]);
            }
        }
        if (!outs.empty()) {
            zeros.assign(outs.size(), 0);
            if ((rc = tick_emit_f32(dst, dt, tm.data(), zeros.data(), outs.data(), (int)outs.size(), n, st))) return rc;
        }
        j = j1;
    }
    return NDCN_OK;
}

#undef ADAMS_ARG

}  // namespace

}  // namespace ndcn

using namespace ndcn;

extern "C" {

int ndcn_ab_step_f32(float *out, const float *y, const float *const *h_f, const float *h_a, int n, float dt, int64_t n_elem, void *stream) {
    return ab_step_f32(out, y, h_f, h_a, n, dt, n_elem, static_cast<hipStream_t>(stream));
}

int ndcn_ab_step_readout_f32(float *out, const float *y, const float *const *h_f, const float *h_a, int n, float dt, int64_t n_rows, int H,
                             const float *Wd, const float *bd, int C, float *dec, float emit_off, void *stream) {
    return ab_step_readout_f32(out, y, h_f, h_a, n, dt, n_rows, H, Wd, bd, C, &dec, &emit_off, 1, static_cast<hipStream_t>(stream));
}

int ndcn_solve_explicit_adams_readout_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0,
                                          const float *h_dt, int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same,
                                          const float *h_tick_off, int64_t n_ticks, int max_order, const float *Wd, const float *bd, int C,
                                          float *out, void *workspace, int64_t workspace_bytes, void *stream) {
    g_last_readout_path = 0;
    const Decoder dc = {Wd, bd, C};
    return adams_run(__func__, A, W, b, H, flags, y0, h_dt, n_steps, h_tick_step, h_tick_same, h_tick_off, n_ticks, max_order, out, nullptr,
                     nullptr, workspace, workspace_bytes, static_cast<hipStream_t>(stream), nullptr, &dc);
}

int ndcn_solve_fixed_adams_readout_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0,
                                       const float *h_dt, int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same,
                                       const float *h_tick_off, int64_t n_ticks, int max_order, float rtol, float atol, int max_iters,
                                       const float *Wd, const float *bd, int C, float *out, int *h_iters, int *h_converged, void *workspace,
                                       int64_t workspace_bytes, void *stream) {
    g_last_readout_path = 0;
    const Corrector pc = {rtol, atol, max_iters, h_iters, h_converged};
    const Decoder dc = {Wd, bd, C};
    return adams_run(__func__, A, W, b, H, flags, y0, h_dt, n_steps, h_tick_step, h_tick_same, h_tick_off, n_ticks, max_order, out, nullptr,
                     nullptr, workspace, workspace_bytes, static_cast<hipStream_t>(stream), &pc, &dc);
}

int64_t ndcn_explicit_adams_workspace_bytes(int64_t n_rows, int H, int max_order) {
    if (n_rows < 0 || H <= 0 || max_order < 2 || max_order > kAbMaxOrder) return NDCN_EINVAL;
    return workspace_need(n_rows, H, solve_panels(max_order));
}

int64_t ndcn_explicit_adams_train_workspace_bytes(int64_t n_rows, int H) {
    if (n_rows < 0 || H <= 0) return NDCN_EINVAL;
    return workspace_need(n_rows, H, kStagePanels);
}

int ndcn_solve_explicit_adams_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0,
                                  const float *h_dt, int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same,
                                  const float *h_tick_off, int64_t n_ticks, int max_order, float *out, void *workspace,
                                  int64_t workspace_bytes, void *stream) {
    return adams_run(__func__, A, W, b, H, flags, y0, h_dt, n_steps, h_tick_step, h_tick_same, h_tick_off, n_ticks, max_order, out, nullptr,
                     nullptr, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int64_t ndcn_fixed_adams_workspace_bytes(int64_t n_rows, int H, int max_order) {
    if (n_rows < 0 || H <= 0 || max_order < 2 || max_order > kAbMaxOrder) return NDCN_EINVAL;
    return workspace_need(n_rows, H, solve_panels(max_order) + kCorrectorPanels) + (int64_t)kCounterBytes;
}

int ndcn_solve_fixed_adams_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0, const float *h_dt,
                               int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same, const float *h_tick_off,
                               int64_t n_ticks, int max_order, float rtol, float atol, int max_iters, float *out, int *h_iters,
                               int *h_converged, void *workspace, int64_t workspace_bytes, void *stream) {
    const Corrector pc = {rtol, atol, max_iters, h_iters, h_converged};
    return adams_run(__func__, A, W, b, H, flags, y0, h_dt, n_steps, h_tick_step, h_tick_same, h_tick_off, n_ticks, max_order, out, nullptr,
                     nullptr, workspace, workspace_bytes, static_cast<hipStream_t>(stream), &pc);
}

int64_t ndcn_fixed_adams_train_workspace_bytes(int64_t n_rows, int H) {
    if (n_rows < 0 || H <= 0) return NDCN_EINVAL;
    return workspace_need(n_rows, H, kStagePanels + kCorrectorRecPanels) + (int64_t)kCounterBytes;
}

int ndcn_fixed_adams_train_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0, const float *h_dt,
                               int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same, const float *h_tick_off,
                               int64_t n_ticks, int max_order, float rtol, float atol, int max_iters, float *out, int *h_iters,
                               int *h_converged, float *rec_f, float *rec_y, float *rec_u, float *rec_c, int64_t cap, int64_t *h_slot,
                               void *workspace, int64_t workspace_bytes, void *stream) {
    if (n_steps > 0 && (!rec_f || !rec_u || !rec_c || !h_slot || cap < 0)) {
        set_error("%s: the records (rec_f, rec_u, rec_c), the slot array and cap >= 0 are required", __func__);
        return NDCN_EINVAL;
    }
    Corrector pc = {rtol, atol, max_iters, h_iters, h_converged};
    pc.rec_u = rec_u; pc.rec_c = rec_c; pc.cap = cap; pc.h_slot = h_slot;
    return adams_run(__func__, A, W, b, H, flags, y0, h_dt, n_steps, h_tick_step, h_tick_same, h_tick_off, n_ticks, max_order, out, rec_f, rec_y,
                     workspace, workspace_bytes, static_cast<hipStream_t>(stream), &pc);
}

int ndcn_explicit_adams_train_f32(const ndcn_csr *A, const float *W, const float *b, int H, uint32_t flags, const float *y0,
                                  const float *h_dt, int64_t n_steps, const int64_t *h_tick_step, const int *h_tick_same,
                                  const float *h_tick_off, int64_t n_ticks, int max_order, float *out, float *rec_f, float *rec_y,
                                  void *workspace, int64_t workspace_bytes, void *stream) {
    if (!rec_f && n_steps > 0) { set_error("%s: the record of the evaluations is missing", __func__); return NDCN_EINVAL; }
    return adams_run(__func__, A, W, b, H, flags, y0, h_dt, n_steps, h_tick_step, h_tick_same, h_tick_off, n_ticks, max_order, out, rec_f, rec_y,
                     workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
