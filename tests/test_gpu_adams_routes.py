"""Which explicit_adams / fixed_adams solves run inside the library and which step through the generic path, on a real MI355X: the
admission table of odeint for the two multistep methods, without a gradient (ndcn_solve_*_adams[_readout]_f32, observed at
odeint._explicit_adams_solve / _fixed_adams_solve) and under one with NDCN_ADAMS_TRAIN=1 (the nodes of fixed_train).  A 6 x 6
eight-neighbour lattice with the normalised Laplacian, H = 8 and H = 16 (the smallest width the in-solve decoder takes), C = 1.
Every comparison is torch.equal against the same solve through a lambda around the ODEFunc, which no library route admits."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

WARNING = 'Warning: Functional iteration did not converge. Solution may be incorrect.'
METHODS = ('explicit_adams', 'fixed_adams')
NODE = {'explicit_adams': '_ExplicitAdamsSolveBackward', 'fixed_adams': '_FixedAdamsSolveBackward'}
SOLVE = {'explicit_adams': '_explicit_adams_solve', 'fixed_adams': '_fixed_adams_solve'}
SIDE = 6
T13 = torch.arange(13) / 128.0
# h = 1 / 128: 4.5 / 128 lies strictly inside step 4, which also ends at the tick 5 / 128 - two ticks in one step
SUB_T, SUB_H = torch.tensor([0., 4.5 / 128, 5.0 / 128, 14.0 / 128]), 1.0 / 128
GRIDS = {'one_tick': (T13[:1], {}), 'two_ticks': (T13[:2], {}), 'three_ticks': (T13[:3], {}), 'max_order_4': (T13, {'max_order': 4}),
         'max_order_12': (T13, {'max_order': 12}), 'step_size': (SUB_T, {'step_size': SUB_H, 'max_order': 6})}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


_LAPLACIAN = {}


def laplacian(dev, extra_rows=0):
    """the lattice's operator on the device; extra_rows: its first rows once more below it - more rows than the state has"""
    from ndcn_amd import graphs
    if extra_rows not in _LAPLACIAN:
        L = graphs.normalized_laplacian(graphs.grid_8_neighbor(SIDE))
        if extra_rows:
            L = sp.vstack([L, L[:extra_rows]]).tocsr()
        _LAPLACIAN[extra_rows] = graphs.to_device(L, dev)
    return _LAPLACIAN[extra_rows]


def make_func(dev, H, extra_rows=0, **kw):
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(3)
    f = ODEFunc(H, laplacian(dev, extra_rows), **kw).to(dev).eval()
    x0 = torch.rand(SIDE * SIDE, H, generator=torch.Generator().manual_seed(4)).to(dev)
    return f, x0


def solve(dev, monkeypatch, capfd, method, func, x0, t, grad, opts=None, rtol=1e-3, atol=1e-4, readout=None, tuple_state=False):
    """one odeint call -> dict: `sol` (detached) or `raised` (type, message); `asked`: what the wrapped library route answered, call by
    call (no-grad solves); `node`: the name of the solution's grad_fn (solves under a gradient); `log`; `warnings`"""
    from ndcn_amd import torchdiffeq as ode
    impl = importlib.import_module('ndcn_amd.torchdiffeq._impl.odeint')
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '1')
    asked = []
    real = getattr(impl, SOLVE[method])
    monkeypatch.setattr(impl, SOLVE[method], lambda *a: asked.append(real(*a)) or asked[-1])
    res = dict(asked=asked, node=None, log=[])
    x = x0.clone().requires_grad_(True) if grad else x0
    torch.manual_seed(11)                                          # (the seed of an active dropout is drawn per solve)
    capfd.readouterr()
    try:
        with torch.enable_grad() if grad else torch.no_grad():
            y = ode.odeint(func, (x,) if tuple_state else x, t.to(dev), rtol=rtol, atol=atol, method=method, options=dict(opts) if opts else None,
                           step_log=res['log'], readout=readout)
            if tuple_state:
                y = y[0]
        torch.cuda.synchronize()
        res['node'] = type(y.grad_fn).__name__
        res['sol'] = y.detach()
    except Exception as e:                                         # (a declined solve gets the generic path's own exception)
        res['raised'] = (type(e), str(e))
    finally:
        monkeypatch.setattr(impl, SOLVE[method], real)
    res['warnings'] = capfd.readouterr().err.splitlines().count(WARNING)
    return res


def same_outcome(a, b):
    if 'raised' in a or 'raised' in b:
        return a.get('raised') == b.get('raised')
    return torch.equal(a['sol'], b['sol'])


def in_library(res, method, grad):
    if grad:
        return res['node'] == NODE[method]
    return len(res['asked']) == 1 and res['asked'][0] is not None


def test_the_step_size_grid_has_a_tick_inside_a_step_and_two_ticks_in_one_step():
    from ndcn_amd.torchdiffeq._impl import core
    plan = core.fixed_plan(SUB_T.numpy(), SUB_H)
    assert not plan.tick_coincident[1] and plan.tick_coincident[2] and plan.tick_step[1] == plan.tick_step[2] and len(plan.dts) == 14


# ----------------------------------------------------------------------------------------------------------------------------- routes

@pytest.mark.parametrize('grad', [False, True], ids=['no_grad', 'grad'])
@pytest.mark.parametrize('method', METHODS)
def test_a_plain_odefunc_takes_the_library_route_on_every_grid(dev, monkeypatch, capfd, method, grad):
    f, x0 = make_func(dev, 8)
    wrapped = lambda tt, y: f(tt, y)
    for name, (t, opts) in GRIDS.items():
        lib = solve(dev, monkeypatch, capfd, method, f, x0, t, grad, opts)
        gen = solve(dev, monkeypatch, capfd, method, wrapped, x0, t, grad, opts)
        # (the training nodes decline a grid of fewer than two ticks; the inference route answers it itself)
        assert in_library(lib, method, grad) == (not (grad and name == 'one_tick')), name
        assert not gen['asked'] and gen['node'] != NODE[method]
        assert lib['sol'].shape == (len(t), SIDE * SIDE, 8) and torch.equal(lib['sol'][0], x0)
        assert same_outcome(lib, gen), name
        assert lib['log'] == gen['log'] and lib['warnings'] == gen['warnings'], name
        if method == 'fixed_adams':
            assert lib['log'][-1][0] == 'nfe' and len(lib['log']) == len(gen['log'])
        if name == 'one_tick':
            assert lib['log'] == ([('nfe', 0)] if method == 'fixed_adams' else [])


def decline_cases(dev, method, grad):
    """name -> (func, the callable whose solve it must equal, keywords of solve()): one reason at a time"""
    f, _ = make_func(dev, 8)
    f_ng, f_nc, f_rows = make_func(dev, 8, no_graph=True)[0], make_func(dev, 8, no_control=True)[0], make_func(dev, 8, extra_rows=4)[0]
    around = lambda g: (lambda tt, y: g(tt, y))
    cases = {'no_graph': (f_ng, around(f_ng), {}), 'no_control': (f_nc, around(f_nc), {}), 'operator_rows': (f_rows, around(f_rows), {}),
             'tuple_state': (lambda tt, ys: (f(tt, ys[0]),), around(f), {'tuple_state': True})}
    if grad:
        f_drop = make_func(dev, 8, dropout=0.5)[0].train()
        cases['active_dropout'] = (f_drop, around(f_drop), {})
    if method == 'fixed_adams':
        cases['max_iters_true'] = (f, around(f), {'opts': {'max_iters': True}})
        cases['rtol_0d_tensor'] = (f, around(f), {'rtol': torch.tensor(1e-3)})
    return cases


@pytest.mark.parametrize('grad', [False, True], ids=['no_grad', 'grad'])
@pytest.mark.parametrize('method', METHODS)
def test_each_decline_reason_takes_the_generic_route(dev, monkeypatch, capfd, method, grad):
    _, x0 = make_func(dev, 8)
    for name, (func, partner, kw) in decline_cases(dev, method, grad).items():
        res = solve(dev, monkeypatch, capfd, method, func, x0, T13, grad, **kw)
        assert not in_library(res, method, grad), name
        assert all(v is None for v in res['asked']) and res['node'] != NODE[method], name
        kw = {k: v for k, v in kw.items() if k != 'tuple_state'}
        gen = solve(dev, monkeypatch, capfd, method, partner, x0, T13, grad, **kw)
        assert not gen['asked'] and gen['node'] != NODE[method], name
        assert same_outcome(res, gen), (name, res.get('raised'), gen.get('raised'))
        assert res['log'] == gen['log'] and res['warnings'] == gen['warnings'], name
        if name not in ('operator_rows', 'rtol_0d_tensor'):            # (these two may fail as the generic path fails)
            assert 'sol' in res, (name, res.get('raised'))


# ---------------------------------------------------------------------------------------------------------------- step_log and stderr

def test_fixed_adams_reports_the_same_on_every_route(dev, monkeypatch, capfd):
    """rtol = atol = 0, max_iters = 2: no step converges - the same step_log and as many warning lines from the library solve, the node
    and the generic path"""
    f, x0 = make_func(dev, 8)
    kw = dict(opts={'max_iters': 2}, rtol=0.0, atol=0.0)
    lib = solve(dev, monkeypatch, capfd, 'fixed_adams', f, x0, T13, False, **kw)
    node = solve(dev, monkeypatch, capfd, 'fixed_adams', f, x0, T13, True, **kw)
    gen = solve(dev, monkeypatch, capfd, 'fixed_adams', lambda tt, y: f(tt, y), x0, T13, False, **kw)
    assert in_library(lib, 'fixed_adams', False) and in_library(node, 'fixed_adams', True) and not gen['asked']
    want = [(0, True)] * 2 + [(2, False)] * 10 + [('nfe', 12 + 3 * 2 + 2 * 10)]
    for res in (lib, node, gen):
        assert res['log'] == want and res['warnings'] == 10
        assert all(type(i) is int and type(c) is bool for i, c in res['log'][:-1])
        assert torch.equal(res['sol'], lib['sol'])
    for grad in (False, True):
        one = solve(dev, monkeypatch, capfd, 'fixed_adams', f, x0, T13[:1], grad, **kw)
        assert one['log'] == [('nfe', 0)] and one['warnings'] == 0 and torch.equal(one['sol'], x0[None])


# ---------------------------------------------------------------------------------------------------------------------------- readout

@pytest.mark.parametrize('grad', [False, True], ids=['no_grad', 'grad'])
@pytest.mark.parametrize('H', [16, 8])
@pytest.mark.parametrize('method', METHODS)
def test_the_decoded_solution_is_linear_of_the_hidden_one(dev, monkeypatch, capfd, method, H, grad):
    """H = 16: without a gradient the decoder runs inside the library's solve; H = 8: it has no form there and odeint decodes after.
    Under a gradient the node holds the decoder at both widths.  The same bits every time."""
    from ndcn_amd import _lib, hip
    f, x0 = make_func(dev, H)
    g = torch.Generator().manual_seed(5)
    Wd, bd = ((torch.rand(1, H, generator=g) - .5) / 2).to(dev), (torch.rand(1, generator=g) - .5).to(dev)
    for name, (t, opts) in GRIDS.items():
        dec = solve(dev, monkeypatch, capfd, method, f, x0, t, grad, opts, readout=(Wd, bd))
        bits = int(_lib.load().ndcn_last_readout_path())
        hid = solve(dev, monkeypatch, capfd, method, f, x0, t, grad, opts)
        assert in_library(dec, method, grad) == in_library(hid, method, grad) == (not (grad and name == 'one_tick')), name
        assert dec['sol'].shape == (len(t), SIDE * SIDE, 1)
        assert torch.equal(dec['sol'], hip.linear(hid['sol'], Wd, bd)), name
        assert dec['log'] == hid['log'] and dec['warnings'] == hid['warnings'], name
        if not grad and len(t) == 13:
            assert (bits != 0) == (H == 16), (name, bits)
