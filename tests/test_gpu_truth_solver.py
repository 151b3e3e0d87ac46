"""The drivers' ground-truth solves inside the device solver (ABI 26): the modules of ndcn_amd.truth, the launch that carries the
Runge-Kutta algebra in the epilogue of the truth right-hand sides (ndcn_dyn_rk_f32 / hip.dyn_rk) and the solver descriptor's `dyn`
field.  The contract is bits: K equals the stand-alone operation, everything after K the separate stage kernels of the generic
path, a module solve the solve of a closure over the stand-alone operation (which steps from Python through core.py)."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

KINDS = {'heat': ('heat', (0.7,)), 'gene': ('gene', (1.0, 1.0, 2.0)), 'gene_pow': ('gene', (0.8, 2.0, 1.5)),
         'mutual': ('mutual', (0.1, 5.0, 1.0, 5.0, 0.9, 0.1))}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.asarray(a))


def names(pattern):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, pattern)))


def last_path():
    from ndcn_amd import _lib
    return int(_lib.load().ndcn_debug_last_rhs_path())


def ran_dyn():
    from ndcn_amd import _lib
    return bool(last_path() & _lib.PATH_DYN)


def clear_path(dev):
    """the report names the LAST right-hand-side launch with a stage epilogue of the thread: an ODEFunc one on two nodes replaces it"""
    from ndcn_amd import CsrOperator, hip
    A = CsrOperator.from_arrays([0, 1, 2], [0, 1], [1.0, 1.0], (2, 2), dev)
    X = torch.ones(2, 4, device=dev)
    hip.rhs_rk(A, X, torch.eye(4, device=dev), torch.zeros(4, device=dev), 'combine', X, [], [0.5])
    assert not ran_dyn()


def standalone(kind, params, A, x):
    from ndcn_amd import hip
    if kind == 'heat':
        return hip.spmm(A, x, alpha=-params[0])
    if kind == 'gene':
        return hip.gene_rhs(A, x, b=params[0], f=params[1], h=params[2])
    return hip.mutual_rhs(A, x, *params)


def module_and_closure(kind, A, L, **kw):
    from ndcn_amd import hip, HeatDiffusion, GeneDynamics, MutualDynamics
    if kind == 'heat':
        return HeatDiffusion(L, 1), lambda t, x: hip.spmm(L, x, alpha=-1.0)
    if kind == 'gene':
        b = kw.get('b', 1.0)
        return GeneDynamics(A, b, 1.0, 2.0), lambda t, x: hip.gene_rhs(A, x, b=b, f=1.0, h=2.0)
    return MutualDynamics(A), lambda t, x: hip.mutual_rhs(A, x)


# ------------------------------------------------------------------------------------------------------------------ a. kernel alone
_CASE = {}


def kernel_case(n, dev):
    """rows of 0, 1, 7, 8, 9 and 65 entries (cycled, capped at n distinct columns) and one hub row of about 300; a ~ N(0, 1) / 8,
    x in [0.05, 1.05): positive, so that x ** 1.5 and the mutualistic denominators are defined"""
    if n not in _CASE:
        from ndcn_amd import CsrOperator
        rng = np.random.RandomState(n % 1000)
        deg = np.array([0, 1, 7, 8, 9, 65], np.int64)[np.arange(n) % 6]
        deg[min(3, n - 1)] = 301
        deg = np.minimum(deg, n)
        indptr = np.zeros(n + 1, np.int64)
        np.cumsum(deg, out=indptr[1:])
        start = rng.randint(0, n, size=n).astype(np.int64)
        rowid = np.repeat(np.arange(n), deg)
        within = np.arange(indptr[-1]) - indptr[rowid]
        # deg distinct columns per row, ascending: a window of consecutive columns from a random start, wrapped and sorted
        cols = (start[rowid] + within) % n
        order = np.lexsort((cols, rowid))
        cols = cols[order]
        data = (rng.randn(indptr[-1]) / 8).astype(np.float32)
        A = CsrOperator.from_arrays(indptr, cols, data, (n, n), dev)
        g = torch.Generator().manual_seed(n)
        x = (0.05 + torch.rand(n, 1, generator=g)).to(dev)
        panels = [(torch.rand(n, 1, generator=g) - 0.5).to(dev) for _ in range(7)]      # y0, five earlier stages, y1
        _CASE.clear()
        _CASE[n] = (A, indptr, cols, x, panels)
    return _CASE[n]


COEF = [0.3125, -0.171875, 0.0625, 0.44140625, -0.09765625, 0.2421875]
COEF2 = [-0.0546875, 0.125, 0.21875, -0.3203125, 0.0390625, 0.15625]


@pytest.mark.parametrize('name', sorted(KINDS))
@pytest.mark.parametrize('n', [1, 31, 33, 4096 * 32 - 1, 4096 * 32 + 1])
def test_kernel_alone(dev, n, name):
    """hip.dyn_rk in every mode with 0..5 earlier stages, coefficients by value and from device memory: K is the stand-alone
    operation, y_next / y_aux the separate stage kernels, the error record an fp64 sum of the float32 z * z (relative 1e-10: double
    accumulation of n <= 2^18 terms is bounded by n 2^-53 < 3e-11), the non-finite count exact."""
    from ndcn_amd import hip
    kind, params = KINDS[name]
    A, indptr, cols, x, panels = kernel_case(n, dev)
    y0, kp, y1 = panels[0], panels[1:6], panels[6]
    K_ref = standalone(kind, params, A, x)
    assert torch.equal(hip.dyn_rk(kind, params, A, x), K_ref)
    rtol, atol = 1e-3, 1e-4
    for by_dev in (False, True):
        def coefs(cs):
            if not by_dev:
                return dict(cs=cs)
            return dict(c_dev=torch.tensor(cs + [0.0] * (8 - len(cs)), dtype=torch.float32, device=dev))
        for m in range(6):
            cs = COEF[:m + 1]
            # ---- COMBINE (and, by value, the second combination)
            K, y_next = hip.dyn_rk(kind, params, A, x, 'combine', y0, kp[:m], **coefs(cs))
            assert torch.equal(K, K_ref), ('combine', m, by_dev)
            assert torch.equal(y_next, hip.combine(y0, kp[:m] + [K_ref], cs)), ('combine', m, by_dev)
            if not by_dev:
                K, y_next2, y_aux = hip.dyn_rk(kind, params, A, x, 'combine', y0, kp[:m], cs=cs, aux_cs=COEF2[:m + 1])
                assert torch.equal(K, K_ref) and torch.equal(y_next2, y_next), ('aux', m)
                assert torch.equal(y_aux, hip.lincomb(kp[:m] + [K_ref], COEF2[:m + 1])), ('aux', m)
            # ---- ERROR
            K, (s, bad) = hip.dyn_rk(kind, params, A, x, 'error', y0, kp[:m], rtol=rtol, atol=atol, y1=y1, **coefs(cs))
            assert torch.equal(K, K_ref), ('error', m, by_dev)
            sm = hip.lincomb(kp[:m] + [K_ref], cs).cpu().numpy().astype(np.float32)
            a0, a1 = np.abs(y0.cpu().numpy()), np.abs(y1.cpu().numpy())
            tol = (np.float32(atol) + np.float32(rtol) * np.maximum(a0, a1)).astype(np.float32)
            z = (sm / tol).astype(np.float32)
            want = float((z * z).astype(np.float32).astype(np.float64).sum())
            assert bad == 0 and abs(s - want) <= 1e-10 * want, ('error', m, by_dev, s, want)
            # ---- RK4 (stages 0..3 of the 3/8 rule)
            if m <= 3:
                dt = 0.0625
                K, y_next = hip.dyn_rk(kind, params, A, x, 'rk4', y0, kp[:m], **coefs([dt]))
                ks = kp[:m] + [K_ref]
                assert torch.equal(K, K_ref), ('rk4', m, by_dev)
                assert torch.equal(y_next, hip.fixed_stage(2 + m, y0, *ks, dt=dt)), ('rk4', m, by_dev)
    # the error state defaults to the evaluation's input
    K, (s, bad) = hip.dyn_rk(kind, params, A, x, 'error', y0, [], cs=[0.25], rtol=rtol, atol=atol)
    K2, (s2, _) = hip.dyn_rk(kind, params, A, x, 'error', y0, [], cs=[0.25], rtol=rtol, atol=atol, y1=x)
    assert s == s2 and bad == 0
    # non-finite elements of y1 are counted, one each (a single-element state has room for one)
    y1b = y1.clone()
    y1b[0, 0] = float('inf')
    if n > 1:
        y1b[n // 2, 0] = float('nan')
    _, (_, bad) = hip.dyn_rk(kind, params, A, x, 'error', y0, kp[:5], cs=COEF, rtol=rtol, atol=atol, y1=y1b)
    assert bad == min(n, 2)
    # a NaN in x comes out as a NaN in K - of every row that reads it - and raises nothing
    row = int(np.argmax(np.diff(indptr) > 0))
    xn = x.clone()
    xn[int(cols[indptr[row]]), 0] = float('nan')
    Kn, _ = hip.dyn_rk(kind, params, A, xn, 'combine', y0, [], cs=[0.5])
    ref = standalone(kind, params, A, xn)
    assert bool(torch.isnan(Kn[row, 0])) and torch.equal(torch.isnan(Kn), torch.isnan(ref))
    assert torch.equal(torch.nan_to_num(Kn), torch.nan_to_num(ref))


def test_heat_past_the_error_record_cap(dev):
    """heat walks one row per lane and an ERROR launch has at most 2048 workgroups: 2048 * 256 + 1 rows take a second pass of the
    row loop with the record accumulating across passes (rows of 0, 1 and 2 entries keep the case small)"""
    from ndcn_amd import CsrOperator, hip
    n = 2048 * 256 + 1
    rng = np.random.RandomState(5)
    deg = (np.arange(n) % 3).astype(np.int64)
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=indptr[1:])
    rowid = np.repeat(np.arange(n), deg)
    cols = (rowid + 7 + 11 * (np.arange(indptr[-1]) - indptr[rowid])) % n
    cols = cols[np.lexsort((cols, rowid))]
    A = CsrOperator.from_arrays(indptr, cols, rng.randn(indptr[-1]).astype(np.float32), (n, n), dev)
    g = torch.Generator().manual_seed(9)
    x, y0, k1, y1 = [(torch.rand(n, 1, generator=g) - 0.25).to(dev) for _ in range(4)]
    K_ref = hip.spmm(A, x, alpha=-0.7)
    cs = COEF[:2]
    K, y_next = hip.dyn_rk('heat', (0.7,), A, x, 'combine', y0, [k1], cs=cs)
    assert torch.equal(K, K_ref) and torch.equal(y_next, hip.combine(y0, [k1, K_ref], cs))
    rtol, atol = 1e-3, 1e-4
    K, (s, bad) = hip.dyn_rk('heat', (0.7,), A, x, 'error', y0, [k1], cs=cs, rtol=rtol, atol=atol, y1=y1)
    sm = hip.lincomb([k1, K_ref], cs).cpu().numpy()
    tol = (np.float32(atol) + np.float32(rtol) * np.maximum(np.abs(y0.cpu().numpy()), np.abs(y1.cpu().numpy()))).astype(np.float32)
    z = (sm / tol).astype(np.float32)
    want = float((z * z).astype(np.float32).astype(np.float64).sum())
    # n 2^-53 = 5.9e-11 for these 2^19 + 1 terms
    assert torch.equal(K, K_ref) and bad == 0 and abs(s - want) <= 1e-10 * want, (s, want)


def test_kernel_refuses_what_it_does_not_carry(dev):
    from ndcn_amd import _lib, hip
    A, _, _, x, panels = kernel_case(33, dev)
    with pytest.raises(_lib.NdcnHipError):          # a second combination with the coefficients in device memory
        hip.dyn_rk('gene', (1.0, 1.0, 2.0), A, x, 'combine', panels[0], [], aux_cs=[1.0], c_dev=torch.ones(8, device=dev))
    with pytest.raises(_lib.NdcnHipError):          # an RK4 stage past the fourth
        hip.dyn_rk('heat', (1.0,), A, x, 'rk4', panels[0], panels[1:5], cs=[0.1])
    with pytest.raises(_lib.NdcnHipError):
        hip.dyn_rk(7, (1.0,), A, x)


# ------------------------------------------------------------------------------------------------------------------ b. goldens
_GOLD = {}


def golden_case(name, dev):
    """operators, inputs and - computed once - the closure solve (the generic path: core.integrate_dopri5) with its step log"""
    if name not in _GOLD:
        from ndcn_amd import CsrOperator
        from ndcn_amd import torchdiffeq as ode
        d = load_golden(name)
        n = int(d['n'])
        A = CsrOperator.from_arrays(d['A_indptr'], d['A_indices'], d['A_data'], (n, n), dev)
        L = CsrOperator.from_arrays(d['L_indptr'], d['L_indices'], d['L_data'], (n, n), dev)
        kind = name.split('_')[1]
        x0, t = T(d['x0']).to(dev), T(d['t']).to(dev)
        _, f = module_and_closure(kind, A, L)
        clear_path(dev)
        log = []
        with torch.no_grad():
            y = ode.odeint(f, x0, t, method='dopri5', step_log=log)
        assert not ran_dyn()
        _GOLD[name] = dict(d=d, n=n, A=A, L=L, kind=kind, x0=x0, t=t, y=y, log=log)
    return _GOLD[name]


def check_traj(y, ref, l1, mx):
    err = np.abs(y - ref)
    scale = max(1.0, np.abs(ref).max())
    assert err.mean() < l1 * scale, 'L1 %.3e' % err.mean()
    assert err.max() < mx * scale, 'max %.3e' % err.max()


@pytest.mark.parametrize('name', names('truth_*_coo.npz'))
def test_truth_goldens(dev, name):
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver
    from oracle import ndcn_oracle as orc
    c = golden_case(name, dev)
    d, n, x0, t = c['d'], c['n'], c['x0'], c['t']
    mod, _ = module_and_closure(c['kind'], c['A'], c['L'])
    # as odeint runs it: one captured graph replayed per attempted step
    log_g = []
    with torch.no_grad():
        y_g = ode.odeint(mod, x0, t, method='dopri5', step_log=log_g)
    assert ran_dyn()
    # and with eager launches
    s = DeviceSolver(mod, n, 'dopri5', use_graph=False)
    y_e = torch.empty((len(t), n, 1), dtype=torch.float32, device=dev)
    y_e[0].copy_(x0)
    s.begin(y_e[0], float(t[0]), borrow=True)
    s.advance_many(t.double().tolist()[1:], y_e[1:])
    torch.cuda.synchronize()
    log_e = s.steplog() + [('nfe', int(s.stats()['nfe']))]
    s.close()
    assert ran_dyn()
    assert torch.equal(y_g, c['y']) and torch.equal(y_e, c['y'])
    ref_log = list(c['log'])
    nfe_ref = dict([ref_log.pop()])['nfe']
    for log in (log_g, log_e):
        log = list(log)
        nfe = dict([log.pop()])['nfe']
        assert len(log) == len(ref_log) and [r[2] for r in log] == [r[2] for r in ref_log]
        assert nfe == nfe_ref == 2 + 6 * len(log)
    check_traj(y_g.cpu().numpy(), d['traj'], l1=2e-5, mx=2e-4)
    Ao = orc.coo_from_csr(d['A_indptr'], d['A_indices'], d['A_data'], (n, n))
    Lo = orc.coo_from_csr(d['L_indptr'], d['L_indices'], d['L_data'], (n, n))
    fo = {'heat': lambda tt, x: orc.heat_rhs(Lo, x), 'gene': lambda tt, x: orc.gene_rhs(Ao, x),
          'mutual': lambda tt, x: orc.mutual_rhs(Ao, x)}[c['kind']]
    lo = []
    orc.odeint(fo, T(d['x0']), T(d['t']), method='dopri5', step_log=lo)
    assert [r[2] for r in log_g[:-1]] == [r[2] for r in lo if r[0] != 'nfe']


# ------------------------------------------------------------------------------------------------------------------ c. fixed grids
@pytest.mark.parametrize('step_size', [None, 0.03])
@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('name', ['truth_gene_coo', 'truth_heat_coo'])
def test_fixed_grids(dev, name, method, step_size):
    """five ticks 0.125 apart; the step size 0.03 does not divide the spacing: ticks fall inside grid steps"""
    from ndcn_amd import torchdiffeq as ode
    c = golden_case(name, dev)
    mod, f = module_and_closure(c['kind'], c['A'], c['L'])
    t = torch.linspace(0., 0.5, 5).to(dev)
    opts = None if step_size is None else {'step_size': step_size}
    with torch.no_grad():
        clear_path(dev)
        want = ode.odeint(f, c['x0'], t, method=method, options=opts)
        assert not ran_dyn()
        got = ode.odeint(mod, c['x0'], t, method=method, options=opts)
    assert ran_dyn()
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------------------------ d. past the grid cap
def test_power_law_past_the_grid_cap(dev):
    """131073 rows: more than the launch's workgroups cover in one pass, hub rows of a power-law graph"""
    from ndcn_amd import graphs, hip, MutualDynamics
    from ndcn_amd import torchdiffeq as ode
    n = 131073
    A = graphs.to_device(graphs.make_graph('power_law', n, seed=0), dev)
    x0 = torch.from_numpy(graphs.x0_blocks(int(np.ceil(np.sqrt(n))))[:n]).to(dev)
    t = torch.tensor([0., 0.005, 0.01]).to(dev)
    logs = [[], []]
    with torch.no_grad():
        clear_path(dev)
        want = ode.odeint(lambda tt, x: hip.mutual_rhs(A, x), x0, t, rtol=1e-5, atol=1e-7, method='dopri5', step_log=logs[0])
        assert not ran_dyn()
        got = ode.odeint(MutualDynamics(A), x0, t, rtol=1e-5, atol=1e-7, method='dopri5', step_log=logs[1])
    assert ran_dyn()
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert [tuple(r) for r in logs[0]] == [tuple(r) for r in logs[1]]


# ------------------------------------------------------------------------------------------------------------------ e. declines
@pytest.mark.parametrize('case', ['decreasing', 'tuple', 'requires_grad', 'two_columns', 'adams', 'first_step'])
def test_declined_solves_call_the_module_back(dev, case):
    from ndcn_amd import torchdiffeq as ode
    c = golden_case('truth_heat_coo' if case == 'two_columns' else 'truth_gene_coo', dev)
    mod, f = module_and_closure(c['kind'], c['A'], c['L'])
    x0 = c['x0'].clone()
    t = torch.linspace(0., 0.2, 3).to(dev)
    kw = dict(method='dopri5', rtol=1e-5, atol=1e-7)
    grad = torch.no_grad()
    if case == 'decreasing':
        t = t.flip(0).contiguous()
    elif case == 'tuple':
        x0 = (x0,)
        one = f
        f = lambda tt, y: tuple(one(tt, y_) for y_ in y)          # (a tuple state is handed over as a tuple)
    elif case == 'requires_grad':
        x0.requires_grad_()
        grad = torch.enable_grad()
    elif case == 'two_columns':
        x0 = torch.cat([x0, 0.5 * x0], dim=1).contiguous()
    elif case == 'adams':
        kw['method'] = 'adams'
    else:
        kw['options'] = {'first_step': 0.01}
    with grad:
        want = ode.odeint(f, x0, t, **kw)
        clear_path(dev)
        got = ode.odeint(mod, x0, t, **kw)
    assert not ran_dyn()
    if case == 'tuple':
        got, want = got[0], want[0]
    assert got.shape == want.shape and torch.equal(got.detach(), want.detach())


def test_operator_that_requires_grad_is_declined(dev):
    """a gradient asked of the operator tensor is a gradient needed: such a solve is not handed to the device solver"""
    from ndcn_amd import HeatDiffusion
    from ndcn_amd.torchdiffeq._impl.odeint import _device_resident_ok
    c = golden_case('truth_heat_coo', dev)
    d, n = c['d'], c['n']
    from oracle import ndcn_oracle as orc
    Ld = orc.dense_from_csr(d['L_indptr'], d['L_indices'], d['L_data'], (n, n)).to(dev)
    ask = lambda L: _device_resident_ok(HeatDiffusion(L, 1), True, (c['x0'],), c['t'], 'dopri5', {}, allow_truth=True)
    with torch.enable_grad():
        assert ask(Ld) is True
        assert ask(Ld.clone().requires_grad_()) is False


# ------------------------------------------------------------------------------------------------------------------ f. cache
def test_kept_solver_follows_parameters_and_operator(dev):
    from ndcn_amd import CsrOperator, GeneDynamics
    from ndcn_amd import torchdiffeq as ode
    c = golden_case('truth_gene_coo', dev)
    d, n, x0 = c['d'], c['n'], c['x0']
    t = torch.linspace(0., 0.3, 4).to(dev)
    A2 = CsrOperator.from_arrays(d['A_indptr'], d['A_indices'], 0.5 * d['A_data'], (n, n), dev)

    def both(mod, A, b):
        _, f = module_and_closure('gene', A, None, b=b)
        with torch.no_grad():
            want = ode.odeint(f, x0, t, method='dopri5')
            got = ode.odeint(mod, x0, t, method='dopri5')
        assert ran_dyn() and torch.equal(got, want)
        return got

    y1 = both(GeneDynamics(c['A'], 1.), c['A'], 1.)
    mod = GeneDynamics(c['A'], 2.)
    y2 = both(mod, c['A'], 2.)
    mod.A = A2
    y3 = both(mod, A2, 2.)
    assert not torch.equal(y1, y2) and not torch.equal(y2, y3)
    assert torch.equal(both(GeneDynamics(c['A'], 1.), c['A'], 1.), y1)        # (a fresh module on the first operator: the kept solver)


# ------------------------------------------------------------------------------------------------------------------ g. errors
def test_nan_state_raises_as_for_odefunc(dev):
    from ndcn_amd import torchdiffeq as ode
    c = golden_case('truth_gene_coo', dev)
    mod, _ = module_and_closure('gene', c['A'], c['L'])
    x0 = c['x0'].clone()
    x0[5, 0] = float('nan')
    with pytest.raises(AssertionError), torch.no_grad():
        ode.odeint(mod, x0, c['t'], method='dopri5')


@pytest.mark.parametrize('what', ['H2', 'shard'])
def test_solver_create_refuses_wide_or_sharded_dynamics(dev, what):
    from ndcn_amd import _lib
    c = golden_case('truth_gene_coo', dev)
    lib = _lib.load()
    dyn = _lib.dynamics(_lib.DYN_GENE, (1.0, 1.0, 2.0))
    shard = _lib.ShardView()
    desc = _lib.SolverDesc(_lib.M_DOPRI5, 2 if what == 'H2' else 1, 0, 0, c['A'].view(), None, None, 1e-7, 1e-9, 2 ** 31 - 1, 0.0, 0.0, 0.0,
                           ctypes.pointer(shard) if what == 'shard' else None, ctypes.pointer(dyn))
    handle = ctypes.c_void_p()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.ndcn_solver_create(ctypes.byref(desc), _lib.ptr(ws), ws.numel(), ctypes.byref(handle))
    assert rc == _lib.EINVAL and not handle.value
    assert lib.ndcn_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------ h. driver
def test_driver_truth_solve_runs_in_the_device_solver(dev, monkeypatch, capsys):
    from ndcn_amd.drivers import dynamics
    from ndcn_amd.truth import GeneDynamics
    seen = []
    real = dynamics.ode.odeint

    def spy(func, *a, **kw):
        out = real(func, *a, **kw)
        if type(func) is GeneDynamics:
            seen.append(ran_dyn())
        return out

    monkeypatch.setattr(dynamics.ode, 'odeint', spy)
    clear_path(dev)
    res = dynamics.main('gene', ['--niters', '2', '--test_freq', '1', '--sampled_time', 'equal'])
    assert seen == [True] and np.isfinite(res['loss'])
