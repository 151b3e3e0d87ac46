"""fixed_adams under a gradient, on the host: the reverse sweep of a predictor-corrector solve restated in float64 and driven by
core.abm_adjoint_terms (which adjoints the gradient of an evaluation gathers from, with which weights, for any pattern of converged
and failed steps) against torch autograd through a float64 restatement of the forward with the iteration counts fixed; the terms
against core.ab_adjoint_terms; the C ABI's new calls and the ISA of the paired gather kernel (csrc/adams_bwd.hip).  CPU-only.

A step i that holds n >= 3 evaluations:  dy_0 = sum_q wP_q f_{i-q},  delta = sum_q wD_q f_{i-q},  u_0 = y_i + dy_0,
u_r = y_i + c0 F(u_{r-1}) + delta (r = 1..R),  y_{i+1} = u_R.  Its reverse:  G_R = lam_{i+1},  G_{r-1} = J(u_{r-1})^T (c0 G_r),
P_i = G_0,  D_i = sum_{r>=1} G_r,  lam_i = P_i + D_i + J(y_i)^T gf_i,  gf_i = sum over the later steps that hold f_i of wP P + wD D."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _adams_bashforth as ab
import _adams_moulton as am
from conftest import ROOT

torch.set_num_threads(1)
f32 = np.float32
NEW_CALLS = ('ndcn_abm_adjoint_f32', 'ndcn_fixed_adams_train_workspace_bytes', 'ndcn_fixed_adams_train_f32')
TOL = 1e-10                                  # tests/test_adams_train_host.py: the bound of the explicit sweep


# ------------------------------------------------------------------------------------------------------- the float64 restatement

def problem(seed=0, n=5, H=3):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(n, n, generator=g, dtype=torch.float64) / 2
    W = torch.randn(H, H, generator=g, dtype=torch.float64) / 2
    b = torch.randn(H, generator=g, dtype=torch.float64) / 2
    y0 = torch.randn(n, H, generator=g, dtype=torch.float64)
    return A, W, b, y0


def rhs(A, W, b, y):
    return torch.relu((A @ y) @ W.t() + b)


def rk4(fun, y, dt, k1):
    k2 = fun(y + dt * k1 / 3)
    k3 = fun(y + dt * (k1 / -3 + k2))
    k4 = fun(y + dt * (k1 - k2 + k3))
    return y + (k1 + 3 * k2 + 3 * k3 + k4) * (dt / 8)


def lengths_of(S, m, converged):
    """the evaluations each step holds, restated: one more per step up to m - 1, one fewer after a predictor-corrector step that failed"""
    out, held = [], 0
    for i in range(S):
        n = min(held + 1, m - 1)
        out.append(n)
        held = n - 1 if (n >= 3 and not converged[i]) else n
    return out


def forward(A, W, b, y0, dts, m, iters, converged, wP, wD, lead):
    """(the states y_0 .. y_S, per step the iterates [u_0 .. u_{R-1}] the corrector evaluated at).  wP / wD(i, n, q, dt): the factors of
    f_{i-q} in dy_0 / delta of step i, which holds n evaluations; lead(i, n, dt): c0"""
    fun = lambda x: rhs(A, W, b, x)
    ns = lengths_of(len(dts), m, converged)
    ys, fs, us = [y0], [], []
    for i, dt in enumerate(dts):
        fs.append(fun(ys[i]))
        n = ns[i]
        if n < 3:
            ys.append(rk4(fun, ys[i], dt, fs[i]))
            us.append([])
            continue
        dy = sum(wP(i, n, q, dt) * fs[i - q] for q in range(n))
        delta = sum(wD(i, n, q, dt) * fs[i - q] for q in range(n))
        u, mine = ys[i] + dy, []
        for _ in range(iters[i]):
            mine.append(u)
            u = ys[i] + lead(i, n, dt) * fun(u) + delta
        ys.append(u)
        us.append(mine)
    return ys, us


def sweep(A, W, b, ys, us, G, dts, m, iters, converged, coefficient, lead):
    """The reverse sweep the training node runs, restated in float64 over core.abm_adjoint_terms.  coefficient(i, step, cP, cD) -> the
    two weights to use for the term of evaluation i in `step`.  -> (g_y0, g_W, g_b)"""
    from ndcn_amd.torchdiffeq._impl import core
    S = len(dts)
    ns = lengths_of(S, m, converged)
    gW, gb = torch.zeros_like(W), torch.zeros_like(b)
    lam = G[S]
    P, D = {}, {}

    def vjp(x, g):
        """J(x)^T g and the parameter gradients, accumulated"""
        with torch.enable_grad():
            x_, W_, b_ = (v.detach().requires_grad_(True) for v in (x, W, b))
            gx, dW, db = torch.autograd.grad((rhs(A, W_, b_, x_) * g).sum(), (x_, W_, b_))
        gW.add_(dW)
        gb.add_(db)
        return gx

    for i in range(S - 1, -1, -1):
        if ns[i] >= 3:
            c0 = lead(i, ns[i], float(dts[i]))
            Gr, Di = lam, torch.zeros_like(lam)
            for u in reversed(us[i]):
                Di = Di + Gr
                Gr = vjp(u, c0 * Gr)
            P[i], D[i] = Gr, Di
            assert len(us[i]) == iters[i] >= 1
        terms = core.abm_adjoint_terms(i, dts, m, converged)
        gf = None
        for step, cP, cD in terms:
            wp, wd = coefficient(i, step, cP, cD)
            gf = (0 if gf is None else gf) + wp * P[step] + wd * D[step]
        if ns[i] >= 3:
            lam = P[i] + D[i] + vjp(ys[i], gf)
        else:
            with torch.enable_grad():
                y_, W_, b_ = (v.detach().requires_grad_(True) for v in (ys[i], W, b))
                fun = lambda x: rhs(A, W_, b_, x)
                fi = fun(y_)
                total = (rk4(fun, y_, float(dts[i]), fi) * lam).sum()
                if gf is not None:
                    total = total + (fi * gf).sum()
                lam, dW, db = torch.autograd.grad(total, (y_, W_, b_))
            gW += dW
            gb += db
        lam = lam + G[i]
    return lam, gW, gb


def grid_steps(S, nonuniform):
    if not nonuniform:
        return np.full(S, 1.0 / 128, dtype=f32)
    return (np.random.RandomState(4).uniform(0.004, 0.012, S)).astype(f32)


def pattern(S, m, kind):
    """(iterations, converged) per step: 0 / True on the warm-up steps; `kind` decides the predictor-corrector steps"""
    iters, conv, ns_held = [], [], 0
    for i in range(S):
        n = min(ns_held + 1, m - 1)
        if n < 3:
            it, ok = 0, True
        elif kind == 'once':
            it, ok = 1, True
        elif kind == 'twice_on_some':
            it, ok = (2 if i % 3 == 0 else 1), True
        elif kind == 'all_fail':
            it, ok = 2, False
        else:                                                    # 'one_fails': step 8, after three iterations
            it, ok = (3, False) if i == 8 else (1, True)
        iters.append(it)
        conv.append(ok)
        ns_held = n - 1 if (n >= 3 and not ok) else n
    return iters, conv


# name: (steps, max_order, non-uniform grid, pattern)
CASES = {'S15_m12': (15, 12, False, 'once'), 'S15_m4': (15, 4, False, 'once'), 'warm_up_only': (2, 12, False, 'once'),
         'm3_never_leaves_rk4': (5, 3, False, 'once'), 'nonuniform': (15, 12, True, 'once'), 'twice_on_some': (15, 12, True, 'twice_on_some'),
         'all_fail': (9, 12, False, 'all_fail'), 'one_fails': (15, 12, False, 'one_fails')}


@pytest.mark.parametrize('case', sorted(CASES))
def test_abm_adjoint_terms_drive_a_sweep_that_equals_autograd(case):
    from ndcn_amd.torchdiffeq._impl import core
    S, m, nonuniform, kind = CASES[case]
    dts = grid_steps(S, nonuniform)
    iters, conv = pattern(S, m, kind)
    ns = lengths_of(S, m, conv)
    assert core.abm_history_lengths(S, m, conv) == ns
    A, W, b, y0 = problem()
    G = [torch.randn(5, 3, generator=torch.Generator().manual_seed(10 + j), dtype=torch.float64) for j in range(S + 1)]
    rel = lambda got, ref: float((got - ref).abs().max() / ref.abs().max())

    def truth(wP, wD, lead):
        y_, W_, b_ = (v.clone().requires_grad_(True) for v in (y0, W, b))
        ys, us = forward(A, W_, b_, y_, [float(d) for d in dts], m, iters, conv, wP, wD, lead)
        sum((y * g).sum() for y, g in zip(ys, G)).backward()
        return [y.detach() for y in ys], [[u.detach() for u in mine] for mine in us], (y_.grad, W_.grad, b_.grad)

    all_terms = [core.abm_adjoint_terms(i, dts, m, conv) for i in range(S)]
    # (i) the structure: exact rational weights in the recursion, the sweep's coefficients in float64 from the same rationals - and the
    # float32 coefficients the function returns within two float32 roundings (the weight, the product) of them
    def exact(i, step, cP, cD):
        n, q = ns[step], step - i
        p64, d64 = float(dts[step]) * float(ab.betas(n)[q]), float(dts[step]) * float(am.mus(n)[q + 1])
        assert isinstance(cP, np.float32) and abs(float(cP) - p64) <= 2.0 ** -23 * abs(p64)
        assert isinstance(cD, np.float32) and abs(float(cD) - d64) <= 2.0 ** -23 * abs(d64)
        return p64, d64
    exact_lead = lambda i, n, dt: dt * float(am.mus(n)[0])
    ys, us, want = truth(lambda i, n, q, dt: dt * float(ab.betas(n)[q]), lambda i, n, q, dt: dt * float(am.mus(n)[q + 1]), exact_lead)
    got = sweep(A, W, b, ys, us, G, dts, m, iters, conv, exact, exact_lead)
    assert all(rel(g, w) < TOL for g, w in zip(got, want)), [rel(g, w) for g, w in zip(got, want)]
    # (ii) the coefficients as they are returned, and c0 as the node forms it, as float64 numbers: against the recursion that steps with
    # those very numbers
    c32 = {(step, step - i): (float(cP), float(cD)) for i, terms in enumerate(all_terms) for step, cP, cD in terms}
    lead32 = lambda i, n, dt: float(core.abm_lead(dts[i], n))
    ys32, us32, want32 = truth(lambda i, n, q, dt: c32[(i, q)][0], lambda i, n, q, dt: c32[(i, q)][1], lead32)
    got32 = sweep(A, W, b, ys32, us32, G, dts, m, iters, conv, lambda i, step, cP, cD: (float(cP), float(cD)), lead32)
    assert all(rel(g, w) < TOL for g, w in zip(got32, want32)), [rel(g, w) for g, w in zip(got32, want32)]
    # the shape of the bookkeeping: step `step` gathers into exactly the ns[step] newest evaluations
    assert all([s for s, _, _ in terms] == sorted(s for s, _, _ in terms) and all(i <= s < S for s, _, _ in terms)
               for i, terms in enumerate(all_terms))
    users = {s: sorted(i for i, terms in enumerate(all_terms) for st, _, _ in terms if st == s) for s in range(S)}
    for s in range(S):
        assert users[s] == (list(range(s - ns[s] + 1, s + 1)) if ns[s] >= 3 else []), (s, users[s])
    if case == 'S15_m12':
        assert max(ns) == 11 and max(len(t) for t in all_terms) == 11
    if case == 'S15_m4':
        assert max(ns) == 3
    if case in ('warm_up_only', 'm3_never_leaves_rk4'):
        assert all(t == [] for t in all_terms)
    if case == 'all_fail':
        assert ns == [1, 2] + [3] * (S - 2)                      # the history never grows past three
    if case == 'one_fails':
        assert ns[:12] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 10, 11] and ns[12:] == [11] * 3      # the lengths dip after step 8 and recover


def test_terms_agree_with_the_explicit_ones_when_every_step_converges():
    from ndcn_amd.torchdiffeq._impl import core
    for S, m, nonuniform in ((15, 12, False), (15, 12, True), (9, 5, True), (6, 4, False), (5, 3, False), (4, 2, False)):
        dts = grid_steps(S, nonuniform)
        for i in range(S):
            got = core.abm_adjoint_terms(i, dts, m, [True] * S)
            want = core.ab_adjoint_terms(i, dts, m)
            assert [(s + 1, float(cP)) for s, cP, _ in got] == [(j, float(c)) for j, c in want], (S, m, i)
            assert all(isinstance(cP, np.float32) and isinstance(cD, np.float32) for _, cP, cD in got)


def test_terms_of_a_hand_worked_grid_with_a_failed_step():
    """S = 5, max_order = 12, step 2 fails: steps 0, 1 are RK4, step 2 holds (f_2, f_1, f_0), step 3 - the oldest evaluation gone -
    (f_3, f_2, f_1), step 4 (f_4 .. f_1)"""
    from ndcn_amd.torchdiffeq._impl import core
    dts = np.asarray([0.5, 0.25, 0.125, 2.0, 1.0], dtype=f32)
    conv = [True, True, False, True, True]
    a3, a4, m3, m4 = ab.weights(3), ab.weights(4), am.weights(3)[1], am.weights(4)[1]
    term = lambda s, a, m, q: (s, f32(dts[s] * a[q]), f32(dts[s] * m[q]))
    want = [[term(2, a3, m3, 2)],
            [term(2, a3, m3, 1), term(3, a3, m3, 2), term(4, a4, m4, 3)],
            [term(2, a3, m3, 0), term(3, a3, m3, 1), term(4, a4, m4, 2)],
            [term(3, a3, m3, 0), term(4, a4, m4, 1)],
            [term(4, a4, m4, 0)]]
    for i in range(5):
        got = core.abm_adjoint_terms(i, dts, 12, conv)
        assert [(s, float(p), float(d)) for s, p, d in got] == [(s, float(p), float(d)) for s, p, d in want[i]], i


# ------------------------------------------------------------------------------------------------------------------------------ the ABI

def test_header_exports_and_binding_carry_the_new_calls():
    from ndcn_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()
    declared = set(re.findall(r'NDCN_API[^;(]*?\b(ndcn_\w+)\s*\(', text))
    assert set(NEW_CALLS) <= declared and set(NEW_CALLS) <= set(_lib.SIGNATURES)
    assert re.search(r'#define NDCN_ABI_VERSION 29\b', text) and _lib.ABI_VERSION == 29
    assert re.search(r'#define NDCN_ECAPACITY\s+-7\b', text) and _lib.ECAPACITY == -7
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NEW_CALLS) <= set(re.findall(r' T (ndcn_\w+)', out))
    lib = _lib.load()
    assert lib.ndcn_abi_version() == 29
    # the training workspace: 3 stage panels, a stage input, dy, delta (256-byte granules), the counter, the rhs scratch - no ring, no
    # state pair; the solve's formula is unchanged
    panel = (1600 * 20 * 4 + 255) // 256 * 256
    work = (int(lib.ndcn_rhs_work_bytes(1600, 20, _lib.F_RELU)) + 255) // 256 * 256
    assert int(lib.ndcn_fixed_adams_train_workspace_bytes(1600, 20)) == 6 * panel + work + 256
    assert int(lib.ndcn_fixed_adams_workspace_bytes(1600, 20, 12)) == (11 + 6 + 3) * panel + work + 256
    assert int(lib.ndcn_fixed_adams_train_workspace_bytes(-1, 20)) < 0 and int(lib.ndcn_fixed_adams_train_workspace_bytes(4, 0)) < 0


def test_isa_of_the_paired_gather_kernel_has_no_contraction_and_loads_before_use(tmp_path):
    """every product and sum is rounded on its own: no fused multiply-add anywhere in the translation unit; nothing spills; for every
    n, with and without a base, the 2 n (+ 1) 16-byte panel loads of an item are issued before the first wait, the aligned body stores 16
    bytes per lane, and the kernel stays within the 128 registers that keep four waves per SIMD"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    path = str(tmp_path / 'adams_bwd.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-S', '--cuda-device-only', '-o', path,
                    os.path.join(ROOT, 'ndcn_amd', 'csrc', 'adams_bwd.hip')], check=True, stderr=subprocess.DEVNULL)
    text = open(path).read()
    assert not re.search(r'\bv_(pk_)?(fma|fmac|mad|mac)\w*', text)
    assert 'scratch_' not in text
    for n in range(1, 12):
        for base in (0, 1):
            m = re.search(r'^(_ZN\w*abm_adjoint_kernelILi%dELb%dE\w*):[^\n]*\n(.*?)s_endpgm' % (n, base), text, re.S | re.M)
            assert m, (n, base)
            lines = m.group(2).split('\n')
            first_load = next(i for i, l in enumerate(lines) if 'global_load_dwordx4' in l)
            first_wait = next(i for i, l in enumerate(lines) if i > first_load and 's_waitcnt vmcnt' in l)
            assert sum('global_load_dwordx4' in l for l in lines[:first_wait]) >= 2 * n + base, (n, base)
            assert sum('global_store_dwordx4' in l for l in lines) >= 1
            regs = re.search(r'\.amdhsa_kernel %s\b.*?\.amdhsa_next_free_vgpr (\d+)' % re.escape(m.group(1)), text, re.S)
            assert regs and int(regs.group(1)) <= 128, (n, base, regs and regs.group(1))
