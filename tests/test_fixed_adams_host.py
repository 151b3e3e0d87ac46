"""fixed_adams on the host: the derivation of the Adams-Moulton coefficients (three ways: the package, the numpy restatement
tests/_adams_moulton.py, and - through the fixtures - the reference), the restatement against the trajectories, iteration counts and
flags captured from the reference (tests/golden/moulton_*.npz, tools/gen_golden.py gen_moulton), the package's control flow driven with
numpy ops, its options handling, and the C ABI's new calls.  CPU-only."""
import contextlib
import fractions
import glob
import io
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import _adams_bashforth as ab
import _adams_moulton as am
from conftest import GOLDEN, ROOT, load_golden
from oracle import ndcn_oracle as orc

torch.set_num_threads(1)
TOL = 1e-6            # tests/test_oracle_golden.py: the bound of the fixed-grid restatements against the reference
NEW_CALLS = ('ndcn_abm_predict_f32', 'ndcn_abm_correct_f32', 'ndcn_fixed_adams_workspace_bytes', 'ndcn_solve_fixed_adams_f32')
F = fractions.Fraction


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'moulton_*.npz')))


def case_options(d):
    """(solver options as the caller passes them, rtol, atol) of a fixture"""
    opts = {k[4:]: (int(v) if k[4:] in ('max_order', 'max_iters') else float(v)) for k, v in d.items() if k.startswith('opt_')}
    return opts, float(d['rtol']), float(d['atol'])


def test_the_fixture_family_is_complete():
    assert names() == ['moulton_default', 'moulton_iterate', 'moulton_never', 'moulton_one_iter', 'moulton_order4', 'moulton_stepsize',
                       'moulton_warmup']


@pytest.mark.parametrize('order', range(4, 13))
def test_moulton_coefficients_are_exact_rationals_that_integrate_polynomials(order):
    """the Adams-Moulton formula of order `order`: order points t + dt, t, .. - what a step holding order - 1 evaluations uses"""
    n = order - 1
    ms = am.mus(n)
    assert len(ms) == order and all(isinstance(m, F) and m != 0 for m in ms)
    assert sum(ms) == 1
    # point i sits at 1 - i (in units of dt, the step being [0, 1]): exact for every polynomial up to degree order - 1 ...
    for k in range(order):
        assert sum(m * F(1 - i) ** k for i, m in enumerate(ms)) == F(1, k + 1)
    # ... and not for degree `order`: the formula's order is exactly that
    assert sum(m * F(1 - i) ** order for i, m in enumerate(ms)) != F(1, order + 1)
    cs, div = am.integer_form(n)
    assert [F(c, div) for c in cs] == ms
    lead, w = am.weights(n)
    assert lead == cs[0] / div and all(x.dtype == np.float32 for x in w)
    assert [float(x) for x in w] == [float(np.float32((1 / div) * c)) for c in cs[1:]]
    # the package derives the same rationals and the same float32 weights on its own
    from ndcn_amd.torchdiffeq._impl import core
    assert core.moulton_rationals(n) == ms and core.moulton_integers(n) == (cs, div)
    plead, pw = core.am_weights(n)
    assert plead == lead and [float(x) for x in pw] == [float(x) for x in w]
    for dt in (0.01, 1.0 / 128, 0.3):
        assert float(core.abm_lead(np.float32(dt), n)) == float(am.lead(np.float32(dt), n)) == \
            float(np.float32(np.float32(dt) * np.float32(lead)))


def test_known_low_orders():
    assert am.integer_form(2) == ([5, 8, -1], 12)                 # Adams-Moulton 3 and 4 of every textbook
    assert am.integer_form(3) == ([9, 19, -5, 1], 24)
    from ndcn_amd.torchdiffeq._impl import core
    assert core.moulton_integers(2) == ([5, 8, -1], 12) and core.moulton_integers(3) == ([9, 19, -5, 1], 24)


def oracle_rhs(d):
    A = orc.coo_from_csr(d['indptr'], d['indices'], d['data'], d['shape'])
    W, b = torch.from_numpy(d['W']), torch.from_numpy(d['b'])
    return lambda x: orc.odefunc_rhs(A, torch.from_numpy(x), W, b, no_control=False).numpy()


def restated(d):
    opts, rtol, atol = case_options(d)
    return am.solve(oracle_rhs(d), d['x0'], d['t'], rtol=rtol, atol=atol, max_order=opts.get('max_order', 12),
                    max_iters=opts.get('max_iters', 4), step_size=opts.get('step_size'))


@pytest.mark.parametrize('name', names())
def test_restatement_reproduces_the_reference(name):
    d = load_golden(name)
    y, nfe, log, _ = restated(d)
    assert y.shape == d['traj'].shape and np.array_equal(y[0], d['x0'])
    assert np.abs(y - d['traj']).max() <= TOL * max(1.0, np.abs(d['traj']).max())
    assert [l[0] for l in log] == d['iters'].tolist()
    assert [int(l[1]) for l in log] == d['converged'].tolist()
    assert nfe == int(d['nfe']) == int(d['n_steps']) + 6 + int(d['iters'].sum())
    assert int(d['n_warnings']) == int((d['converged'] == 0).sum())
    # the generator's conditions: a trajectory that blows up proves nothing
    assert np.isfinite(d['traj']).all() and np.abs(d['traj']).max() <= 10 * np.abs(d['x0']).max()


def test_every_recorded_decision_has_a_margin():
    """replayed with the restatement: a converged iteration has max(err / tol) <= 0.5, a failed one an element with err >= 2 tol or
    tol == 0 - a last-bit difference between two machines cannot flip a decision"""
    for name in names():
        d = load_golden(name)
        opts, rtol, atol = case_options(d)
        seen = []
        real = am.correct

        def spy(f, delta, y, dy, c0, rt, at):
            new, u, bad = real(f, delta, y, dy, c0, rt, at)
            tol = np.float32(at) + np.float32(rt) * np.maximum(np.abs(dy), np.abs(new))
            err = np.abs(dy - new)
            seen.append(bad == 0)
            if bad == 0:
                assert (err / tol).max() <= 0.5, name
            else:
                assert (tol == 0).all() or (err >= 2 * tol).any(), name
            return new, u, bad
        am.correct = spy
        try:
            restated(d)
        finally:
            am.correct = real
        assert len(seen) == int(d['iters'].sum())


def test_what_the_cases_cover():
    d = load_golden('moulton_default')
    assert len(d['t']) - 1 >= 16 and d['iters'][2:].tolist() == [1] * (len(d['t']) - 3) and d['converged'].all()
    assert (float(d['rtol']), float(d['atol'])) == (0.01, 0.001)                   # the drivers' tolerances
    d = load_golden('moulton_iterate')
    assert d['iters'].max() >= 2 and d['converged'].all()
    d = load_golden('moulton_never')
    assert float(d['rtol']) == float(d['atol']) == 0.0
    assert d['iters'][2:].tolist() == [4] * (len(d['iters']) - 2) and not d['converged'][2:].any()
    d = load_golden('moulton_one_iter')
    assert int(d['opt_max_iters']) == 1 and d['iters'].max() == 1 and int(d['n_warnings']) >= 1
    assert int(load_golden('moulton_order4')['opt_max_order']) == 4
    d = load_golden('moulton_stepsize')
    g = ab.grid_of(d['t'], float(d['opt_step_size']))
    on_grid = [bool((g == tj).any()) for tj in d['t'][1:]]
    assert len(g) - 1 >= 14 and any(on_grid) and not all(on_grid)
    assert load_golden('moulton_warmup')['iters'].tolist() == [0, 0]


class NumpyOps:
    """the panel-ops interface of core.integrate_fixed over numpy float32: the restatement's arithmetic"""

    @staticmethod
    def fixed_stage(op, y, k1, k2=None, k3=None, k4=None, dt=0.0):
        y, dt = y.numpy(), np.float32(dt)
        k = [None if q is None else q.numpy() for q in (k1, k2, k3, k4)]
        f32 = np.float32
        out = {2: lambda: y + dt * k[0] / f32(3), 3: lambda: y + dt * (k[0] / f32(-3) + k[1]), 4: lambda: y + dt * (k[0] - k[1] + k[2]),
               5: lambda: y + (k[0] + f32(3) * k[1] + f32(3) * k[2] + k[3]) * (dt / f32(8))}[op]()
        return torch.from_numpy(out.astype(np.float32))

    @staticmethod
    def ab_step(y, fs, coeffs, dt):
        return torch.from_numpy(ab.ab_step(y.numpy(), [f.numpy() for f in fs], coeffs, dt))

    @staticmethod
    def abm_predict(y, fs, a, m, dt):
        fs = [f.numpy() for f in fs]
        dy, delta = am.dot(fs, a, dt), am.dot(fs, m, dt)
        return torch.from_numpy(dy), torch.from_numpy(delta), torch.from_numpy((y.numpy() + dy).astype(np.float32))

    @staticmethod
    def abm_correct(f, delta, y, dy, c0, rtol, atol):
        new, u, bad = am.correct(f.numpy(), delta.numpy(), y.numpy(), dy.numpy(), c0, rtol, atol)
        return torch.from_numpy(new), torch.from_numpy(u), bad

    @staticmethod
    def tick_emit(y, dt, tms):
        v = y.numpy()
        with np.errstate(all='ignore'):
            return [torch.from_numpy((v + ((v - v) / np.float32(dt)) * np.float32(tm)).astype(np.float32)) for tm in tms]


def core_solve(d, method='fixed_adams', **override):
    from ndcn_amd.torchdiffeq._impl import core
    rhs = oracle_rhs(d)
    calls = []

    def f(t, y):
        calls.append(1)
        return (torch.from_numpy(rhs(y[0].numpy())),)
    raw, rtol, atol = case_options(d)
    raw.update(override)
    opts = core.fixed_options(method, raw)
    plan = core.fixed_plan(d['t'], opts['step_size']) if 'step_size' in opts else None
    log = []
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        sol = core.integrate_fixed(NumpyOps, f, (torch.from_numpy(d['x0']),), torch.from_numpy(d['t']), method, plan=plan,
                                   max_order=opts['max_order'], max_iters=opts.get('max_iters', 4), rtol=rtol, atol=atol, step_log=log)
    return np.stack([s[0].numpy() for s in sol]), len(calls), log, err.getvalue()


@pytest.mark.parametrize('name', names())
def test_core_control_flow_equals_the_restatement_bit_for_bit(name):
    """core.integrate_fixed's fixed_adams branch (history, order, warm-up, iterations, the dropped evaluation, ticks) driven with numpy
    ops and the oracle's f"""
    d = load_golden(name)
    got, n_calls, log, err = core_solve(d)
    want, nfe, wlog, _ = restated(d)
    assert got.tobytes() == want.tobytes()
    assert n_calls == nfe == int(d['nfe'])
    assert log[-1] == ('nfe', nfe) and log[:-1] == wlog
    assert [l[0] for l in wlog] == d['iters'].tolist() and [int(l[1]) for l in wlog] == d['converged'].tolist()
    lines = err.splitlines()
    assert lines == ['Warning: Functional iteration did not converge. Solution may be incorrect.'] * int(d['n_warnings'])


def test_implicit_false_is_explicit_adams_bit_for_bit():
    """options={'implicit': False}: fixed_adams.py:185 skips the corrector - odeint hands the solve to the explicit_adams route (on the
    device: tests/test_gpu_fixed_adams.py); here the option's parsing and the explicit branch on this family's inputs"""
    from ndcn_amd.torchdiffeq._impl import core
    opts = core.fixed_options('fixed_adams', {'implicit': False, 'max_order': 6})
    assert opts == {'implicit': False, 'max_iters': 4, 'max_order': 6}
    d = load_golden('moulton_default')
    expl, n_expl, _, _ = core_solve(d, method='explicit_adams')
    want, nfe, _ = ab.solve(oracle_rhs(d), d['x0'], d['t'])
    assert expl.tobytes() == want.tobytes() and n_expl == nfe


def test_methods_and_options():
    from ndcn_amd.torchdiffeq._impl import core
    from ndcn_amd.torchdiffeq._impl.odeint import SOLVERS
    assert 'fixed_adams' in core.METHODS and 'fixed_adams' in core.GRID_METHODS and 'fixed_adams' in SOLVERS
    assert core.UNSUPPORTED == ('tsit5',) and core.FIXED_SOLVER_NAMES['fixed_adams'] == 'AdamsBashforthMoulton'
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        assert core.fixed_options('fixed_adams', None) == {'implicit': True, 'max_iters': 4, 'max_order': 12}
        assert core.fixed_options('fixed_adams', {'max_order': 40, 'step_size': 0.5, 'max_iters': 2, 'implicit': True}) == \
            {'implicit': True, 'max_iters': 2, 'max_order': 12, 'step_size': 0.5}
        assert not w
        core.fixed_options('fixed_adams', {'max_order': 5, 'bogus': 1})
    assert [str(x.message) for x in w] == ["AdamsBashforthMoulton: Unexpected arguments {'bogus': 1}"]
    with pytest.raises(ValueError):
        core.fixed_options('fixed_adams', {'grid_constructor': lambda f, y, t: t})
    for name in ('rtol', 'atol'):                                  # odeint.py:74 passes both by keyword already
        with pytest.raises(TypeError, match="multiple values for keyword argument '%s'" % name):
            core.fixed_options('fixed_adams', {name: 1e-3})


def test_orders_and_iteration_limits_the_reference_fails_on_fail_the_same_way():
    from ndcn_amd.torchdiffeq._impl import core
    f = lambda t, y: (-y[0],)
    t = torch.linspace(0., 0.5, 6)
    y0 = (torch.ones(4),)
    with pytest.raises(IndexError):                                # deque(maxlen=0): prev_f[0] of the first step
        core.integrate_fixed(NumpyOps, f, y0, t, 'fixed_adams', max_order=1)
    with pytest.raises(ValueError):                                # deque(maxlen=-1)
        core.integrate_fixed(NumpyOps, f, y0, t, 'fixed_adams', max_order=0)
    err = io.StringIO()
    with contextlib.redirect_stderr(err), pytest.raises(UnboundLocalError):   # :200 reads the evaluation of a loop that never ran
        core.integrate_fixed(NumpyOps, f, y0, t, 'fixed_adams', max_iters=0)
    assert err.getvalue().count('did not converge') == 1           # ... after the warning of the third step
    with pytest.raises(TypeError):                                 # range(2.5)
        core.integrate_fixed(NumpyOps, f, y0, t, 'fixed_adams', max_iters=2.5)
    # max_order 2 and 3 never leave the warm-up: the bits of rk4, no corrector
    for mo in (2, 3):
        log = []
        a = core.integrate_fixed(NumpyOps, f, y0, t, 'fixed_adams', max_order=mo, step_log=log)
        b = core.integrate_fixed(NumpyOps, f, y0, t, 'rk4')
        assert all(torch.equal(x[0], y[0]) for x, y in zip(a, b))
        assert log == [(0, True)] * 5 + [('nfe', 20)]


def test_host_state_is_refused_with_both_exception_types():
    from ndcn_amd import _lib
    from ndcn_amd import torchdiffeq as ode
    assert issubclass(_lib.NdcnHostStateError, _lib.NdcnHipError) and issubclass(_lib.NdcnHostStateError, NotImplementedError)
    with pytest.raises(_lib.NdcnHostStateError, match='no CPU fallback') as info:
        ode.odeint(lambda t, y: -y, torch.ones(3), torch.tensor([0., 1.]), method='fixed_adams')
    assert isinstance(info.value, NotImplementedError) and isinstance(info.value, _lib.NdcnHipError) and info.value.code == _lib.EINVAL
    with pytest.raises(NotImplementedError):
        ode.odeint(lambda t, y: -y, torch.ones(3), torch.tensor([0., 1.]), method='tsit5')
    # the reference's argument errors still come first
    with pytest.raises(TypeError):
        ode.odeint(lambda t, y: -y, torch.ones(3, dtype=torch.int64), torch.tensor([0., 1.]), method='fixed_adams')


def test_sharded_odeint_declines():
    from ndcn_amd import sharding
    with pytest.raises(NotImplementedError, match='fixed_adams'):
        sharding.sharded_odeint(None, None, None, 4, torch.zeros(4, 2), torch.tensor([0., 1.]), method='fixed_adams')


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
    # the explicit solve's workspace + dy, delta, the corrector's evaluation (256-byte granules) + the counter's 256 bytes
    panel = (1600 * 20 * 4 + 255) // 256 * 256
    for mo in (2, 4, 12):
        assert int(lib.ndcn_fixed_adams_workspace_bytes(1600, 20, mo)) == \
            int(lib.ndcn_explicit_adams_workspace_bytes(1600, 20, mo)) + 3 * panel + 256
    assert int(lib.ndcn_fixed_adams_workspace_bytes(1600, 20, 1)) < 0 and int(lib.ndcn_fixed_adams_workspace_bytes(1600, 20, 13)) < 0
    # the header says what differs from the explicit solve
    assert re.search(r'read-back', text[text.index('ndcn_solve_fixed_adams_f32:'):][:2500])


FUSED = r'\bv_(pk_)?(fma|fmac|mad|mac)(mk|ak)?(_legacy|_mix\w*)?_(f16|f32|f64|bf16)\b'


def test_isa_of_the_two_kernels_has_no_contraction_and_moves_16_bytes_per_lane(tmp_path):
    """every product and sum is rounded on its own: no floating-point fused multiply-add in either kernel; the aligned body moves 16 bytes
    per lane (predict: n + 1 loads issued before the first wait, three stores; correct: four loads, two stores); nothing spills, no
    scratch; the count leaves a workgroup through one 64-bit integer atomic"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    path = str(tmp_path / 'adams_pc.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-S', '--cuda-device-only', '-o', path,
                    os.path.join(ROOT, 'ndcn_amd', 'csrc', 'adams_pc.hip')], check=True, stderr=subprocess.DEVNULL)
    text = open(path).read()
    assert not re.search(FUSED, text)
    assert re.search(FUSED, 'v_fma_f32 v1, v2, v3, v4') and re.search(FUSED, 'v_pk_fma_f32 v[0:1]') and re.search(FUSED, 'v_fmac_f32 v1, v2')
    assert 'scratch_' not in text
    assert re.findall(r'\.vgpr_spill_count:\s+(\d+)', text) and set(re.findall(r'\.vgpr_spill_count:\s+(\d+)', text)) == {'0'}
    assert set(re.findall(r'\.private_segment_fixed_size:\s+(\d+)', text)) == {'0'}
    assert max(int(v) for v in re.findall(r'\.vgpr_count:\s+(\d+)', text)) <= 128
    for n in range(3, 12):
        m = re.search(r'^(_ZN\w*abm_predict_kernelILi%dE\w*):[^\n]*\n(.*?)s_endpgm' % n, text, re.S | re.M)
        assert m, n
        lines = m.group(2).split('\n')
        first = next(i for i, l in enumerate(lines) if 'global_load_dwordx4' in l)
        first_wait = next(i for i, l in enumerate(lines) if i > first and 's_waitcnt vmcnt' in l)
        assert sum('global_load_dwordx4' in l for l in lines[:first_wait]) >= n + 1, n
        assert sum('global_store_dwordx4' in l for l in lines) >= 3, n
    m = re.search(r'^(_ZN\w*abm_correct_kernel\w*):[^\n]*\n(.*?)s_endpgm', text, re.S | re.M)
    assert m
    body = m.group(2)
    assert body.count('global_load_dwordx4') >= 4 and body.count('global_store_dwordx4') >= 2
    assert len(re.findall(r'global_atomic_add_x2', body)) == 1
