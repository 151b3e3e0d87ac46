"""explicit_adams under a gradient, on the host: the bookkeeping of the reverse sweep (core.ab_adjoint_terms: which adjoints the
gradient of an evaluation gathers from, with which weights) against torch autograd through a float64 restatement of the solve, the C
ABI's new calls, and the ISA of the gather kernel (csrc/adams_bwd.hip).  CPU-only."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _adams_bashforth as ab
from conftest import ROOT

torch.set_num_threads(1)
f32 = np.float32
NEW_CALLS = ('ndcn_ab_adjoint_f32', 'ndcn_explicit_adams_train_workspace_bytes', 'ndcn_explicit_adams_train_f32')


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


def held(i, m):
    return min(i + 1, m - 1)


def forward(A, W, b, y0, dts, m, weight):
    """the states y_0 .. y_S of the forward recursion; weight(i, k, q, dt): the factor of f_{i-q} in step i, which has k terms"""
    fun = lambda x: rhs(A, W, b, x)
    ys, fs = [y0], []
    for i, dt in enumerate(dts):
        fs.append(fun(ys[i]))
        k = held(i, m)
        if k < 3:
            ys.append(rk4(fun, ys[i], dt, fs[i]))
        else:
            ys.append(ys[i] + sum(weight(i, k, q, dt) * fs[i - q] for q in range(k)))
    return ys


def exact_weight(i, k, q, dt):
    return dt * float(ab.betas(k)[q])


def sweep(A, W, b, ys, G, dts, m, coefficient):
    """The reverse sweep the training node runs, restated in float64: lam_j the full adjoint of y_j, gf_i gathered over
    core.ab_adjoint_terms, one reverse evaluation per Adams-Bashforth step, the RK4 warm-up step with gf_i one more gradient of its k1.
    coefficient(i, j, c): the weight to use for the term (j, c) of evaluation i.  -> (g_y0, g_W, g_b)"""
    from ndcn_amd.torchdiffeq._impl import core
    S = len(dts)
    gW, gb = torch.zeros_like(W), torch.zeros_like(b)
    lam = {S: G[S]}
    for i in range(S - 1, -1, -1):
        terms = core.ab_adjoint_terms(i, dts, m)
        gf = sum(coefficient(i, j, c) * lam[j] for j, c in terms) if terms else None
        with torch.enable_grad():
            y_, W_, b_ = (v.detach().requires_grad_(True) for v in (ys[i], W, b))
            fun = lambda x: rhs(A, W_, b_, x)
            fi = fun(y_)
            if held(i, m) >= 3:
                total = (fi * gf).sum()                          # the step itself is linear in f_i: it is one of the terms
                gy, dW, db = torch.autograd.grad(total, (y_, W_, b_))
                a = lam[i + 1] + gy
            else:
                total = (rk4(fun, y_, float(dts[i]), fi) * lam[i + 1]).sum()
                if gf is not None:
                    total = total + (fi * gf).sum()
                a, dW, db = torch.autograd.grad(total, (y_, W_, b_))
        gW += dW
        gb += db
        lam[i] = a + G[i]
    return lam[0], gW, gb


CASES = {'S15_m12': (15, 12, False), 'S15_m5': (15, 5, False), 'S4_m12': (4, 12, False), 'S5_m3': (5, 3, False), 'nonuniform': (15, 12, True)}


def grid_steps(S, nonuniform):
    if not nonuniform:
        return np.full(S, 1.0 / 128, dtype=f32)
    return (np.random.RandomState(4).uniform(0.004, 0.012, S)).astype(f32)


@pytest.mark.parametrize('case', sorted(CASES))
def test_ab_adjoint_terms_drive_a_sweep_that_equals_autograd(case):
    from ndcn_amd.torchdiffeq._impl import core
    S, m, nonuniform = CASES[case]
    dts = grid_steps(S, nonuniform)
    A, W, b, y0 = problem()
    G = [torch.randn(5, 3, generator=torch.Generator().manual_seed(10 + j), dtype=torch.float64) for j in range(S + 1)]
    rel = lambda got, ref: float((got - ref).abs().max() / ref.abs().max())

    def truth(weight):
        y_, W_, b_ = (v.clone().requires_grad_(True) for v in (y0, W, b))
        ys = forward(A, W_, b_, y_, [float(d) for d in dts], m, weight)
        sum((y * g).sum() for y, g in zip(ys, G)).backward()
        return [y.detach() for y in ys], (y_.grad, W_.grad, b_.grad)

    all_terms = [core.ab_adjoint_terms(i, dts, m) for i in range(S)]
    # (i) the structure, to 1e-10: the exact rational weights in the recursion, every coefficient of the sweep taken in float64 from the
    # same rationals - and the float32 coefficient the function returns within two float32 roundings (the weight, the product) of it
    def exact(i, j, c):
        step = j - 1
        c64 = float(dts[step]) * float(ab.betas(held(step, m))[step - i])
        assert isinstance(c, np.float32) and abs(float(c) - c64) <= 2.0 ** -23 * abs(c64)
        return c64
    ys, want = truth(exact_weight)
    got = sweep(A, W, b, ys, G, dts, m, exact)
    assert all(rel(g, w) < 1e-10 for g, w in zip(got, want)), [rel(g, w) for g, w in zip(got, want)]
    # (ii) the coefficients as they are returned, as float64 numbers: against the recursion that steps with those very numbers, to 1e-10
    # again.  (Against the exact-weight recursion they are another function - the order-11 weights alternate in sign with magnitudes in
    # the hundreds, which amplifies their float32 rounding - so that comparison has no bound of its own; (i) bounds each coefficient.)
    c32 = {(j - 1, j - 1 - i): float(c) for i, terms in enumerate(all_terms) for j, c in terms}
    ys32, want32 = truth(lambda i, k, q, dt: c32[(i, q)])
    got32 = sweep(A, W, b, ys32, G, dts, m, lambda i, j, c: float(c))
    assert all(rel(g, w) < 1e-10 for g, w in zip(got32, want32))
    # the shape of the bookkeeping
    sizes = [len(t) for t in all_terms]
    assert all(j > i and j <= S for i, terms in enumerate(all_terms) for j, _ in terms)
    assert all([j for j, _ in terms] == sorted(j for j, _ in terms) for terms in all_terms)
    if m < 4:
        assert sizes == [0] * S                                  # every step is RK4: no evaluation is a history term
    else:
        n_ab = sum(held(i, m) >= 3 for i in range(S))
        assert sum(sizes) == sum(held(i, m) for i in range(S) if held(i, m) >= 3) and n_ab > 0
        assert max(sizes) == min(m - 1, n_ab)                    # S15_m12: an evaluation with all eleven terms
    if case == 'S15_m12':
        assert max(sizes) == 11 and sum(held(i, m) == 11 for i in range(S)) == 5


def test_terms_of_a_hand_worked_grid():
    """S = 4, max_order = 12: steps 0, 1 are RK4, step 2 has 3 terms (AB3 weights 23/12, -16/12, 5/12), step 3 has 4"""
    from ndcn_amd.torchdiffeq._impl import core
    dts = np.asarray([0.5, 0.25, 0.125, 2.0], dtype=f32)
    w3, w4 = ab.weights(3), ab.weights(4)
    want = [[(3, f32(dts[2] * w3[2])), (4, f32(dts[3] * w4[3]))],
            [(3, f32(dts[2] * w3[1])), (4, f32(dts[3] * w4[2]))],
            [(3, f32(dts[2] * w3[0])), (4, f32(dts[3] * w4[1]))],
            [(4, f32(dts[3] * w4[0]))]]
    for i in range(4):
        got = core.ab_adjoint_terms(i, dts, 12)
        assert [(j, float(c)) for j, c in got] == [(j, float(c)) for j, c in want[i]]
        assert all(isinstance(c, np.float32) for _, c in got)
    assert core.ab_adjoint_terms(3, dts, 4) == [(4, f32(dts[3] * w3[0]))]      # max_order 4: three terms for good


# ------------------------------------------------------------------------------------------------------------------ ABI and routing

def test_header_exports_and_binding_carry_the_new_calls():
    from ndcn_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()
    declared = set(re.findall(r'NDCN_API[^;(]*?\b(ndcn_\w+)\s*\(', text))
    assert set(NEW_CALLS) <= declared and set(NEW_CALLS) <= set(_lib.SIGNATURES)
    assert re.search(r'#define NDCN_ABI_VERSION 29\b', text) and _lib.ABI_VERSION == 29
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NEW_CALLS) <= set(re.findall(r' T (ndcn_\w+)', out))
    lib = _lib.load()
    assert lib.ndcn_abi_version() == 29
    # the training workspace: 3 stage panels + a stage input (256-byte granules) + the rhs scratch; the solve's formula is unchanged
    panel = (1600 * 20 * 4 + 255) // 256 * 256
    work = (int(lib.ndcn_rhs_work_bytes(1600, 20, _lib.F_RELU)) + 255) // 256 * 256
    assert int(lib.ndcn_explicit_adams_train_workspace_bytes(1600, 20)) == 4 * panel + work
    assert int(lib.ndcn_explicit_adams_workspace_bytes(1600, 20, 12)) == (11 + 6) * panel + work
    assert int(lib.ndcn_explicit_adams_train_workspace_bytes(-1, 20)) < 0 and int(lib.ndcn_explicit_adams_train_workspace_bytes(4, 0)) < 0


def test_the_switch_is_off_by_default_and_read_through_the_shared_reader(monkeypatch):
    import inspect
    from ndcn_amd.torchdiffeq._impl import fixed_train
    assert "env_str('NDCN_ADAMS_TRAIN', '0')" in inspect.getsource(fixed_train.adams_train_enabled)
    monkeypatch.delenv('NDCN_ADAMS_TRAIN', raising=False)
    assert not fixed_train.adams_train_enabled()
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '0')
    assert not fixed_train.adams_train_enabled()
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '1')
    assert fixed_train.adams_train_enabled()


def test_isa_of_the_gather_kernel_has_no_contraction_and_loads_before_use(tmp_path):
    """every product and sum is rounded on its own: no fused multiply-add anywhere in the translation unit; nothing spills; for every
    n, with and without a base, the n (+ 1) 16-byte panel loads of an item are issued before the first wait and the aligned body
    stores 16 bytes per lane"""
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
            m = re.search(r'^(_ZN\w*ab_adjoint_kernelILi%dELb%dE\w*):[^\n]*\n(.*?)s_endpgm' % (n, base), text, re.S | re.M)
            assert m, (n, base)
            lines = m.group(2).split('\n')
            first_load = next(i for i, l in enumerate(lines) if 'global_load_dwordx4' in l)
            first_wait = next(i for i, l in enumerate(lines) if i > first_load and 's_waitcnt vmcnt' in l)
            assert sum('global_load_dwordx4' in l for l in lines[:first_wait]) >= n + base, (n, base)
            assert sum('global_store_dwordx4' in l for l in lines) >= 1
