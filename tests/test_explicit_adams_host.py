"""explicit_adams on the host: the coefficient derivation, the numpy restatement (tests/_adams_bashforth.py) against the trajectories
captured from the reference (tests/golden/bashforth_*.npz, tools/gen_golden.py gen_bashforth), the package's own derivation and options
handling, and the C ABI's new calls.  CPU-only."""
import fractions
import glob
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import _adams_bashforth as ab
from conftest import GOLDEN, ROOT, load_golden
from oracle import ndcn_oracle as orc

torch.set_num_threads(1)
TOL = 1e-6            # tests/test_oracle_golden.py: the bound of the fixed-grid restatements against the reference
NEW_CALLS = ('ndcn_ab_step_f32', 'ndcn_explicit_adams_workspace_bytes', 'ndcn_solve_explicit_adams_f32')


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'bashforth_*.npz')))


def test_the_fixture_family_is_complete():
    assert names() == ['bashforth_default', 'bashforth_no_control', 'bashforth_order4', 'bashforth_stepsize', 'bashforth_warmup']


@pytest.mark.parametrize('order', range(3, 12))
def test_coefficients_are_exact_rationals_that_sum_to_one(order):
    bs = ab.betas(order)
    assert len(bs) == order and all(isinstance(b, fractions.Fraction) and b != 0 for b in bs)
    assert sum(bs) == 1                                           # the step integrates a constant exactly
    # ... and every polynomial up to degree order - 1: sum_i beta_i (-i)^m = 1 / (m + 1)
    for m in range(order):
        assert sum(b * fractions.Fraction(-i) ** m for i, b in enumerate(bs)) == fractions.Fraction(1, m + 1)
    cs, div = ab.integer_form(order)
    assert [fractions.Fraction(c, div) for c in cs] == bs
    w = ab.weights(order)
    assert all(x.dtype == np.float32 for x in w)
    assert [float(x) for x in w] == [float(np.float32((1 / div) * c)) for c in cs]
    # the package derives the same float32 weights on its own
    from ndcn_amd.torchdiffeq._impl import core
    assert core.bashforth_rationals(order) == bs
    assert [float(x) for x in core.ab_weights(order)] == [float(x) for x in w]


def test_known_low_orders():
    assert ab.integer_form(3) == ([23, -16, 5], 12)               # Adams-Bashforth 3 and 4 of every textbook
    assert ab.integer_form(4) == ([55, -59, 37, -9], 24)


def oracle_rhs(d):
    A = orc.coo_from_csr(d['indptr'], d['indices'], d['data'], d['shape'])
    W, b = torch.from_numpy(d['W']), torch.from_numpy(d['b'])
    no_control = bool(int(d['no_control']))
    return lambda x: orc.odefunc_rhs(A, torch.from_numpy(x), W, b, no_control=no_control).numpy()


@pytest.mark.parametrize('name', names())
def test_restatement_reproduces_the_reference(name):
    d = load_golden(name)
    y, nfe, _ = ab.solve(oracle_rhs(d), d['x0'], d['t'], max_order=int(d.get('opt_max_order', 12)),
                         step_size=float(d['opt_step_size']) if 'opt_step_size' in d else None)
    assert y.shape == d['traj'].shape
    assert np.array_equal(y[0], d['x0'])
    assert np.abs(y - d['traj']).max() <= TOL * max(1.0, np.abs(d['traj']).max())
    assert nfe == int(d['nfe']) == int(d['n_steps']) + 6
    # the generator's stability condition: a trajectory that blows up proves nothing
    assert np.isfinite(d['traj']).all() and np.abs(d['traj']).max() <= 10 * np.abs(d['x0']).max()


def test_the_default_case_reaches_order_eleven_and_the_grid_case_has_loose_and_coincident_ticks():
    assert len(load_golden('bashforth_default')['t']) - 1 >= 13               # 2 warm-up steps, orders 3 .. 11, two more: the ring wraps
    d = load_golden('bashforth_stepsize')
    g = ab.grid_of(d['t'], float(d['opt_step_size']))
    assert len(g) - 1 >= 14
    on_grid = [bool((g == tj).any()) for tj in d['t'][1:]]
    assert any(on_grid) and not all(on_grid)


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
    # the workspace: max_order - 1 history panels + 3 stage panels + a stage input + 2 state panels (256-byte granules) + the rhs scratch
    panel = (1600 * 20 * 4 + 255) // 256 * 256
    work = (int(lib.ndcn_rhs_work_bytes(1600, 20, _lib.F_RELU)) + 255) // 256 * 256
    for mo in (2, 4, 12):
        assert int(lib.ndcn_explicit_adams_workspace_bytes(1600, 20, mo)) == (mo - 1 + 6) * panel + work
    assert int(lib.ndcn_explicit_adams_workspace_bytes(1600, 20, 1)) < 0 and int(lib.ndcn_explicit_adams_workspace_bytes(1600, 20, 13)) < 0


def test_isa_of_the_step_kernel_has_no_contraction_and_loads_before_use(tmp_path):
    """every product and sum is rounded on its own: the step kernels hold no fused multiply-add (hip's __fmul_rn / __fadd_rn, inlined
    from a header compiled with contraction on, produced v_pk_fma_f32 here); the n panel loads and the state's are issued before the
    first wait; the aligned body moves 16 bytes per lane; nothing spills"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    path = str(tmp_path / 'adams.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-S', '--cuda-device-only', '-o', path,
                    os.path.join(ROOT, 'ndcn_amd', 'csrc', 'adams.hip')], check=True, stderr=subprocess.DEVNULL)
    text = open(path).read()
    assert not re.search(r'\bv_(pk_)?(fma|fmac|mad|mac)\w*', text)
    assert 'scratch_' not in text
    for n in range(3, 12):
        m = re.search(r'^(_ZN\w*ab_step_kernelILi%dE\w*):[^\n]*\n(.*?)s_endpgm' % n, text, re.S | re.M)
        assert m, n
        lines = m.group(2).split('\n')
        first_wait = next(i for i, l in enumerate(lines) if 'global_load_dwordx4' in l)
        first_wait = next(i for i, l in enumerate(lines) if i > first_wait and 's_waitcnt vmcnt' in l)
        # (the compiler may keep two items of the grid-stride loop in flight: then twice as many)
        assert sum('global_load_dwordx4' in l for l in lines[:first_wait]) >= n + 1, n
        assert sum('global_store_dwordx4' in l for l in lines) >= 1


def test_methods_and_options():
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.torchdiffeq._impl import core
    from ndcn_amd.torchdiffeq._impl.odeint import SOLVERS
    assert 'explicit_adams' in core.METHODS and 'explicit_adams' in SOLVERS and 'explicit_adams' not in core.UNSUPPORTED
    f, y0, t = (lambda t, y: -y), torch.ones(3), torch.tensor([0., 1.])
    for method in ('tsit5', 'fixed_adams'):
        with pytest.raises(NotImplementedError):
            ode.odeint(f, y0, t, method=method)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        assert core.fixed_options('explicit_adams', {'max_order': 40, 'step_size': 0.5, 'rtol': 1., 'max_iters': 2}) == \
            {'max_order': 12, 'step_size': 0.5}
        assert core.fixed_options('explicit_adams', None) == {'max_order': 12}
        assert core.fixed_options('rk4', {'step_size': torch.tensor(0.25)}) == {'step_size': 0.25}
        assert core.fixed_options('euler', {}) == {}
        assert not w
        core.fixed_options('explicit_adams', {'max_order': 5, 'bogus': 1})
        core.fixed_options('rk4', {'max_order': 5})
    assert [str(x.message) for x in w] == ["AdamsBashforth: Unexpected arguments {'bogus': 1}", "RK4: Unexpected arguments {'max_order': 5}"]
    with pytest.raises(ValueError):
        core.fixed_options('explicit_adams', {'grid_constructor': lambda f, y, t: t})
    with pytest.raises(TypeError):
        core.fixed_options('explicit_adams', {'implicit': True})


def test_host_tensors_are_refused():
    from ndcn_amd import _lib, hip
    from ndcn_amd import torchdiffeq as ode
    with pytest.raises(_lib.NdcnHipError):
        ode.odeint(lambda t, y: -y, torch.ones(4), torch.tensor([0., .1, .2, .3, .4]), method='explicit_adams')
    with pytest.raises(_lib.NdcnHipError):
        hip.ab_step(torch.ones(4), [torch.ones(4)] * 3, [1., 1., 1.], 0.1)


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
    def tick_emit(y, dt, tms):
        v = y.numpy()
        with np.errstate(all='ignore'):
            return [torch.from_numpy((v + ((v - v) / np.float32(dt)) * np.float32(tm)).astype(np.float32)) for tm in tms]


@pytest.mark.parametrize('name', names())
def test_core_control_flow_equals_the_restatement_bit_for_bit(name):
    """core.integrate_fixed's explicit_adams branch (history, order, warm-up, ticks) driven with numpy ops and the oracle's f"""
    from ndcn_amd.torchdiffeq._impl import core
    d = load_golden(name)
    rhs = oracle_rhs(d)
    calls = []

    def f(t, y):
        calls.append(1)
        return (torch.from_numpy(rhs(y[0].numpy())),)
    opts = core.fixed_options('explicit_adams', {k[4:]: float(v) for k, v in d.items() if k.startswith('opt_')})
    t = torch.from_numpy(d['t'])
    plan = core.fixed_plan(d['t'], opts['step_size']) if 'step_size' in opts else None
    sol = core.integrate_fixed(NumpyOps, f, (torch.from_numpy(d['x0']),), t, 'explicit_adams', plan=plan, max_order=opts['max_order'])
    want, nfe, _ = ab.solve(rhs, d['x0'], d['t'], max_order=opts['max_order'], step_size=opts.get('step_size'))
    got = np.stack([s[0].numpy() for s in sol])
    assert got.tobytes() == want.tobytes()
    assert len(calls) == nfe == int(d['nfe'])


@pytest.mark.parametrize('max_order,steps,evals', [(2, 5, 20), (3, 5, 20), (4, 5, 11), (12, 5, 11)])
def test_orders_that_never_leave_the_warm_up(max_order, steps, evals):
    from ndcn_amd.torchdiffeq._impl import core
    calls = []

    def f(t, y):
        calls.append(1)
        return (-y[0],)
    t = torch.linspace(0., 0.5, steps + 1)
    a = core.integrate_fixed(NumpyOps, f, (torch.ones(4),), t, 'explicit_adams', max_order=max_order)
    assert len(calls) == evals
    if max_order < 4:                                              # every step is the RK4 step: the bits of method='rk4'
        b = core.integrate_fixed(NumpyOps, f, (torch.ones(4),), t, 'rk4')
        assert all(torch.equal(x[0], y[0]) for x, y in zip(a, b))


def test_orders_the_reference_fails_on_fail_the_same_way():
    from ndcn_amd.torchdiffeq._impl import core
    f = lambda t, y: (-y[0],)
    t = torch.linspace(0., 0.5, 4)
    with pytest.raises(IndexError):                                # deque(maxlen=0): prev_f[0] of the first step
        core.integrate_fixed(NumpyOps, f, (torch.ones(4),), t, 'explicit_adams', max_order=1)
    with pytest.raises(ValueError):                                # deque(maxlen=-1)
        core.integrate_fixed(NumpyOps, f, (torch.ones(4),), t, 'explicit_adams', max_order=0)
