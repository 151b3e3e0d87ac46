"""The fixed-grid `step_size` option (FixedGridODESolver, solvers.py:39-108) on a real MI355X: the reference's fixtures
(tests/golden/substep_*.npz), exact self-consistency with this library's own solve on the explicit grid on every route, the
tick_emit kernels on bit patterns, gradients of the two training routes and of odeint_adjoint, memory as conditions, and the
hipGraph replay form against the eager one."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.asarray(a))


def trajectory_fixtures():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'substep_*.npz')))
    return [n for n in names if n not in ('substep_grids', 'substep_adjoint_rk4')]


def make_func(d, dev, as_module=True, **kw):
    from ndcn_amd import CsrOperator, hip
    from ndcn_amd.neural_dynamics import ODEFunc
    A = CsrOperator.from_arrays(d['indptr'], d['indices'], d['data'], d['shape'], dev)
    H = d['W'].shape[0]
    if as_module:
        f = ODEFunc(H, A, **kw).to(dev)
        f.load_state_dict({'wt.weight': T(d['W']), 'wt.bias': T(d['b'])})
        return f.eval()
    W, b = T(d['W']).to(dev), T(d['b']).to(dev)
    return lambda t, x: hip.rhs(A, x, W, b, no_graph=kw.get('no_graph', False), no_control=kw.get('no_control', False))


def check_traj(y, ref, l1, mx):
    """tests/test_gpu_odeint.py: check_traj"""
    err = np.abs(y - ref)
    scale = max(1.0, np.abs(ref).max())
    print('L1 %.3e  max %.3e  (bars %.1e / %.1e of %.3g)' % (err.mean(), err.max(), l1, mx, scale))
    assert err.mean() < l1 * scale, 'L1 %.3e' % err.mean()
    assert err.max() < mx * scale, 'max %.3e' % err.max()


@pytest.mark.parametrize('as_module', [True, False], ids=['device_resident', 'generic'])
@pytest.mark.parametrize('name', trajectory_fixtures())
def test_substep_golden(dev, name, as_module):
    """every fixture the reference wrote with options={'step_size': h}, within the bar of the plain fixed-grid fixtures"""
    from ndcn_amd import torchdiffeq as ode
    d = load_golden(name)
    f = make_func(d, dev, as_module, no_control=bool(d['no_control']))
    with torch.no_grad():
        y = ode.odeint(f, T(d['x0']).to(dev), T(d['t']).to(dev), method=name.split('_')[1], options={'step_size': float(d['h'])})
    assert y.shape == d['traj'].shape
    assert np.array_equal(y[0].cpu().numpy(), d['x0'])
    check_traj(y.cpu().numpy(), d['traj'], l1=1e-5, mx=1e-4)


# ---------------------------------------------------------------------------------------------------------- self-consistency, exact
TICK_SETS = {'irregular': ([0., .13, .5, .55, .57, 1.0], 0.1), 'multiples': ([0., .25, .5, 1.0], 0.125)}


def _route_case(dev, route):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    if route == 'sweep':
        op = graphs.normalized_laplacian(graphs.make_graph('random', 9000, seed=0)).tocsr()
        op.sort_indices()
        H = 256
    else:
        S, H = {'small': (20, 20), 'graph': (60, 64), 'eager': (370, 64), 'fused3': (64, 256)}[route]
        op = graphs.normalized_laplacian(graphs.grid_8_neighbor(S))
    torch.manual_seed(3)
    A = graphs.to_device(op, dev)
    f = ODEFunc(H, A).to(dev).eval()
    x0 = torch.rand(op.shape[0], H, generator=torch.Generator().manual_seed(4)).to(dev)
    return f, A, x0


@pytest.mark.parametrize('ticks', sorted(TICK_SETS))
@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('route', ['small', 'graph', 'eager', 'fused3', 'sweep'])
def test_substep_equals_the_explicit_grid(dev, route, method, ticks):
    """the sub-stepped solve is the SAME library's solve on the explicit grid, taken at the emitting rows: same kernels, same order,
    same float32 step sizes - torch.equal (value equality: a tick strictly inside a step has -0.0 turned into +0.0), no tolerance"""
    from ndcn_amd import _lib
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.torchdiffeq._impl import core
    from ndcn_amd.torchdiffeq._impl.odeint import GRAPH_MAX_ELEMS
    f, A, x0 = _route_case(dev, route)
    lib = _lib.load()
    small = bool(lib.ndcn_solve_small_supported(A.view_ref(), f.hidden_size, _lib.F_RELU, _lib.METHODS[method], 0))
    assert small == (route == 'small')
    assert (x0.numel() > GRAPH_MAX_ELEMS) == (route == 'eager')
    tt, h = TICK_SETS[ticks]
    t = torch.tensor(tt)
    plan = core.fixed_plan(t.numpy(), h)
    with torch.no_grad():
        y = ode.odeint(f, x0, t.to(dev), method=method, options={'step_size': h})
        path = int(lib.ndcn_debug_last_rhs_path())
        fine = ode.odeint(f, x0, torch.from_numpy(plan.grid).to(dev), method=method)
    if route == 'fused3':
        assert path & _lib.PATH_FUSED3
    if route == 'sweep':
        assert A.sweep is not None and path == (_lib.PATH_FUSED3 | _lib.PATH_SWEEP)
    assert y.shape[0] == len(tt) and torch.isfinite(y).all()
    assert torch.equal(y[0], x0)
    for j in range(1, len(tt)):
        assert torch.equal(y[j], fine[plan.tick_step[j] + 1]), (j, float((y[j] - fine[plan.tick_step[j] + 1]).abs().max()))


# ---------------------------------------------------------------------------------------------------------- the kernels
def _emit_expected(y, dt, tms, same):
    """solvers.py:107-108 with y0 = y1, as torch evaluates it on the device in float32; a coincident tick is y itself"""
    dt_t = torch.tensor(dt, dtype=torch.float32, device=y.device)
    return [y.clone() if s else y + ((y - y) / dt_t) * torch.tensor(tm, dtype=torch.float32, device=y.device) for tm, s in zip(tms, same)]


def _same_bits(a, b):
    nan = torch.isnan(a)
    return bool((nan == torch.isnan(b)).all()) and torch.equal(a[~nan].view(torch.int32), b[~nan].view(torch.int32))


def _special(n, dev, seed):
    y = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    for pos, v in ((n - 1, -0.0), (n // 2, 0.0), (n // 3, 1e-42), (0, -0.0), (1, float('inf')), (2, float('-inf')), (3, float('nan'))):
        y[pos % n] = v                                        # (the first four positions last: the checks below name them)
    return y.to(dev)


@pytest.mark.parametrize('n', [4096, 1001, 7, 400 * 20])
@pytest.mark.parametrize('nt', [1, 8, 9])
def test_tick_emit_on_bit_patterns(dev, n, nt):
    """ndcn_tick_emit_f32 against the reference's expression: -0.0 -> +0.0, Inf -> NaN, NaN stays, a coincident tick is a copy with
    its sign bit; 9 ticks are two launches; sizes that are not a multiple of 4 take the scalar form"""
    from ndcn_amd import _lib, hip
    y = _special(n, dev, n + nt)
    dt = float(np.float32(0.1))
    tms = [float(np.float32(0.1 * (q + 1) / (nt + 1))) for q in range(nt)]
    same = [0] * nt
    same[-1] = 1                                                         # the last tick of the step coincides with its end
    outs = [torch.full((n,), 7.0, device=dev) for _ in range(nt)]
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.ndcn_tick_emit_f32(_lib.ptr(y), dt, (ctypes.c_float * nt)(*tms), (ctypes.c_int * nt)(*same),
                                          (ctypes.c_void_p * nt)(*[o.data_ptr() for o in outs]), nt, n, _lib.stream_ptr()))
    for got, ref, s in zip(outs, _emit_expected(y, dt, tms, same), same):
        assert _same_bits(got, ref)
        if not s:
            assert not bool(torch.signbit(got[0])) and bool(torch.isnan(got[1])) and bool(torch.isnan(got[2])) and bool(torch.isnan(got[3]))
        else:
            assert bool(torch.signbit(got[0])) and bool(torch.isinf(got[1]))
    # the op the generic path calls (every tick through the expression)
    for got, ref in zip(hip.tick_emit(y, dt, tms), _emit_expected(y, dt, tms, [0] * nt)):
        assert _same_bits(got, ref)


@pytest.mark.parametrize('n', [4096, 1001])
@pytest.mark.parametrize('op', [0, 5])
@pytest.mark.parametrize('nt', [1, 3, 9])
def test_emitting_final_stage_equals_stage_then_emit(dev, op, n, nt):
    """ndcn_fixed_stage_emit_f32 = ndcn_fixed_stage_f32 followed by ndcn_tick_emit_f32, bit for bit - state and ticks, in place too"""
    from ndcn_amd import _lib, hip
    gen = torch.Generator().manual_seed(n + op + nt)
    y = torch.randn(n, generator=gen).to(dev)
    ks = [torch.randn(n, generator=gen).to(dev) for _ in range(4)]
    ks[0][5] = float('inf')
    dt = float(np.float32(0.37))
    tms = [float(np.float32(0.37 * (q + 1) / (nt + 1))) for q in range(nt)]
    same = [0] * (nt - 1) + [1]
    y1 = hip.fixed_stage(op, y, *ks[:1 if op == 0 else 4], dt=dt)
    ref = _emit_expected(y1, dt, tms, same)
    lib = _lib.load()
    for in_place in (False, True):
        state = y.clone() if in_place else torch.empty_like(y)
        src = state if in_place else y
        outs = [torch.empty_like(y) for _ in range(nt)]
        with torch.cuda.device(dev):
            _lib.check(lib.ndcn_fixed_stage_emit_f32(op, _lib.ptr(state), _lib.ptr(src), _lib.ptr(ks[0]), _lib.ptr(ks[1]), _lib.ptr(ks[2]),
                                                     _lib.ptr(ks[3]), dt, (ctypes.c_float * nt)(*tms), (ctypes.c_int * nt)(*same),
                                                     (ctypes.c_void_p * nt)(*[o.data_ptr() for o in outs]), nt, n, _lib.stream_ptr()))
        assert _same_bits(state, y1)
        for got, want in zip(outs, ref):
            assert _same_bits(got, want)


@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4'])
def test_substep_hipgraph_replay_equals_eager(dev, method):
    """ndcn_solver_advance_grid: one replay of the captured step per grid step (step size through the pinned ring, ticks read from the
    solver's panel) gives the bits of the eager launches (emitting final stage / destination = the tick panel)"""
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    from ndcn_amd.torchdiffeq._impl import core
    from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver
    op = graphs.normalized_laplacian(graphs.grid_8_neighbor(60))
    torch.manual_seed(5)
    f = ODEFunc(20, graphs.to_device(op, dev)).to(dev).eval()
    x0 = torch.rand(3600, 20, generator=torch.Generator().manual_seed(6)).to(dev)
    outs = []
    for tt, h in TICK_SETS.values():
        plan = core.fixed_plan(np.array(tt, dtype=np.float32), h)
        for use_graph in (False, True):
            s = DeviceSolver(f, 3600, method, use_graph=use_graph)
            s.begin(x0, tt[0])
            o = torch.empty((len(tt) - 1, 3600, 20), device=dev)
            s.advance_grid(plan, o)
            torch.cuda.synchronize()
            assert s.stats()['nfe'] == {'euler': 1, 'midpoint': 2, 'rk4': 4}[method] * (len(plan.grid) - 1)
            s.close()
            outs.append(o)
        assert torch.equal(outs[-2], outs[-1]) and torch.isfinite(outs[-1]).all()


# ---------------------------------------------------------------------------------------------------------- gradients
def _train_pair(dev, f, x0, tt, h, method, flags=None):
    """(sub-stepped, explicit grid with the loss on the emitting rows): trajectories at the ticks and gradients of y0, W, b"""
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.torchdiffeq._impl import core
    plan = core.fixed_plan(np.array(tt, dtype=np.float32), h)
    rows = [0] + [int(r) + 1 for r in plan.tick_step[1:]]
    wts = torch.randn((len(tt),) + tuple(x0.shape), generator=torch.Generator().manual_seed(7)).to(dev)
    res = []
    os.environ.update(flags or {})
    try:
        for sub in (True, False):
            f.zero_grad()
            y0 = x0.clone().requires_grad_(True)
            if sub:
                y = ode.odeint(f, y0, torch.tensor(tt).to(dev), method=method, options={'step_size': h})
            else:
                y = ode.odeint(f, y0, torch.from_numpy(plan.grid).to(dev), method=method)[rows]
            (y * wts).sum().backward()
            res.append((y.detach().cpu(), y0.grad.cpu(), f.wt.weight.grad.cpu().clone(), f.wt.bias.grad.cpu().clone()))
    finally:
        for k in (flags or {}):
            del os.environ[k]
    return res


def _close(a, b, what):
    """tests/test_gpu_small_solve.py, test_fixed_grid_training_through_fused_launches_...: 1e-4 of the tensor's scale"""
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    print('%s: max |difference| %.3e (bar %.1e)' % (what, err, 1e-4 * scale))
    assert err <= 1e-4 * scale, (what, err, scale)


@pytest.mark.parametrize('ticks', sorted(TICK_SETS))
@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('shape', [(45, 20), (30, 256), (20, 20)], ids=['fused_launches', 'fused3', 'one_launch'])
def test_substep_training_equals_training_on_the_explicit_grid(dev, shape, method, ticks):
    """loss.backward() through the sub-stepped solve - checkpointed per tick interval (_SubstepSolve) or, for a state that fits one
    compute unit, the one-launch pair on the explicit grid - against the same library's training on the explicit grid"""
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    S, H = shape
    op = graphs.normalized_laplacian(graphs.grid_8_neighbor(S))
    torch.manual_seed(11)
    f = ODEFunc(H, graphs.to_device(op, dev)).to(dev)
    x0 = torch.rand(S * S, H, generator=torch.Generator().manual_seed(12)).to(dev)
    tt, h = TICK_SETS[ticks]
    (ya, gya, gWa, gba), (yb, gyb, gWb, gbb) = _train_pair(dev, f, x0, tt, h, method)
    assert torch.equal(ya, yb) or float((ya - yb).abs().max()) <= 1e-5 * max(1.0, float(yb.abs().max()))
    _close(gya, gyb, 'g_y0')
    _close(gWa, gWb, 'g_W')
    _close(gba, gbb, 'g_b')


def test_substep_training_takes_the_checkpointed_route(dev):
    from ndcn_amd import graphs
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.neural_dynamics import ODEFunc
    op = graphs.normalized_laplacian(graphs.grid_8_neighbor(45))
    f = ODEFunc(20, graphs.to_device(op, dev)).to(dev)
    y = ode.odeint(f, torch.rand(2025, 20, device=dev), torch.tensor([0., .5, 1.], device=dev), method='rk4', options={'step_size': .1})
    assert type(y.grad_fn).__name__ == '_SubstepSolveBackward'


def test_odeint_adjoint_with_step_size_against_reference_gradients(dev):
    """odeint_adjoint hands `options` to the forward solve and to every backward interval solve (adjoint.py): against the gradients
    the REFERENCE's odeint_adjoint produced (substep_adjoint_rk4.npz), at the bars of test_odeint_adjoint_against_reference_gradients"""
    from ndcn_amd import CsrOperator
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.neural_dynamics import ODEFunc
    d = load_golden('substep_adjoint_rk4')
    f = ODEFunc(8, CsrOperator.from_arrays(d['indptr'], d['indices'], d['data'], d['shape'], dev)).to(dev)
    f.load_state_dict({'wt.weight': T(d['W']), 'wt.bias': T(d['b'])})
    x0 = T(d['x0']).to(dev).requires_grad_(True)
    y = ode.odeint_adjoint(f, x0, T(d['t']).to(dev), method='rk4', options={'step_size': float(d['h'])})
    print('trajectory: max |difference| %.3e' % np.abs(y.detach().cpu().numpy() - d['traj']).max())
    assert np.abs(y.detach().cpu().numpy() - d['traj']).max() < 1e-5
    loss = torch.nn.functional.l1_loss(y, T(d['target']).to(dev))
    assert abs(float(loss.detach()) - float(d['loss'])) < 1e-6
    loss.backward()
    rel = lambda a, b: float((a - b).abs().max() / (b.abs().max() + 1e-12))
    figs = (rel(x0.grad.cpu(), T(d['g_x0'])), rel(f.wt.weight.grad.cpu(), T(d['g_W'])), rel(f.wt.bias.grad.cpu(), T(d['g_b'])))
    print('relative gradient differences (y0, W, b): %.3e %.3e %.3e (bar 2e-3)' % figs)
    assert max(figs) < 2e-3


# ---------------------------------------------------------------------------------------------------------- memory, as conditions
def _big_case(dev):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    op = graphs.normalized_laplacian(graphs.grid_8_neighbor(370))              # 136 900 x 64 floats: 35 MB per panel
    torch.manual_seed(1)
    f = ODEFunc(64, graphs.to_device(op, dev)).to(dev)
    x0 = torch.rand(370 * 370, 64, generator=torch.Generator().manual_seed(2)).to(dev)
    return f, x0


def test_inference_memory_does_not_grow_with_the_grid(dev):
    """T = 4 ticks over 256 grid steps: the peak stays below the solver's workspace + (T + 2) panels - the explicit grid would
    allocate 257"""
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver
    f, x0 = _big_case(dev)
    f.eval()
    panel = x0.numel() * 4
    assert panel >= 32 << 20
    s = DeviceSolver(f, x0.shape[0], 'rk4')
    ws = s.workspace.numel()
    s.close()
    del s
    t = torch.tensor([0., 64., 128., 256.]) / 1024.0
    h = 1.0 / 1024.0
    with torch.no_grad():
        ode.odeint(f, x0, torch.tensor([0., h]).to(dev), method='rk4')       # operator plans, packed weights: built before measuring
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        y = ode.odeint(f, x0, t.to(dev), method='rk4', options={'step_size': h})
        torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    print('peak %.1f MB = %.2f panels beyond the workspace (%.1f MB); bound: T + 2 = 6 panels' % (peak / 2 ** 20, (peak - ws) / panel, ws / 2 ** 20))
    assert y.shape[0] == 4 and torch.isfinite(y).all()
    assert peak < ws + (4 + 2) * panel


def test_training_memory_is_below_the_explicit_grid(dev):
    """one training step with 8 ticks x 8 sub-steps against the same step on the explicit 64-step grid: strictly less memory"""
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.torchdiffeq._impl import core
    f, x0 = _big_case(dev)
    h = 1.0 / 64.0
    t = torch.arange(9, dtype=torch.float32) / 8.0
    plan = core.fixed_plan(t.numpy(), h)
    assert len(plan.grid) == 65 and plan.tick_coincident[1:].all()
    rows = [0] + [int(r) + 1 for r in plan.tick_step[1:]]
    peaks = {}
    for sub in (True, False):
        f.zero_grad()
        y0 = x0.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        if sub:
            y = ode.odeint(f, y0, t.to(dev), method='euler', options={'step_size': h})
        else:
            y = ode.odeint(f, y0, torch.from_numpy(plan.grid).to(dev), method='euler')[rows]
        y.sum().backward()
        torch.cuda.synchronize()
        peaks[sub] = torch.cuda.max_memory_allocated(dev) - base
        del y, y0
    print('training peak: sub-stepped %.1f MB, explicit grid %.1f MB, ratio %.3f' % (peaks[True] / 2 ** 20, peaks[False] / 2 ** 20,
                                                                                    peaks[True] / peaks[False]))
    assert peaks[True] < peaks[False]
