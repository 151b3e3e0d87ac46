"""explicit_adams (the reference's AdamsBashforth, torchdiffeq/_impl/fixed_adams.py:151-211) on a real MI355X: the step kernel
ndcn_ab_step_f32 bit for bit against the numpy restatement (tests/_adams_bashforth.py), the generic path (core.integrate_fixed over the
panel ops) and the device-resident solve (ndcn_solve_explicit_adams_f32) against the trajectories captured from the reference
(tests/golden/bashforth_*.npz) and against each other, the evaluation count, gradients against fp64 autograd, and NDCN."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import _adams_bashforth as ab
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = (1, 3, 4, 5, 255, 256, 257, 4099)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.asarray(a))


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'bashforth_*.npz')))


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def at_offset(a, off, dev):
    """a copy of the 1-d array on the device that starts `off` elements behind a 16-byte boundary"""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.size]
    v.copy_(T(a))
    return v


# ------------------------------------------------------------------------------------------------------------------ the step kernel

@pytest.mark.parametrize('offsets', ['aligned', 'all_plus_one', 'mixed', 'in_place'])
@pytest.mark.parametrize('n', range(3, 12))
def test_ab_step_bit_for_bit(dev, n, offsets):
    """every order at the sizes around the 16-byte lane and the workgroup, panels on / one element off / differently off a 16-byte
    boundary, and the state updated in place"""
    from ndcn_amd import hip
    rng = np.random.RandomState(100 + n)
    a = ab.weights(n)
    for size in SIZES:
        y = rng.randn(size).astype(f32)
        fs = [rng.randn(size).astype(f32) for _ in range(n)]
        dt = f32(0.0371)
        want = ab.ab_step(y, fs, a, dt)
        oy = {'aligned': 0, 'all_plus_one': 1, 'mixed': 0, 'in_place': 0}[offsets]
        of = [(1 if offsets == 'all_plus_one' else (q % 4 if offsets == 'mixed' else 0)) for q in range(n)]
        yd = at_offset(y, oy, dev)
        fd = [at_offset(f, o, dev) for f, o in zip(fs, of)]
        if offsets == 'in_place':
            got = hip.ab_step(yd, fd, a, dt, out=yd)
            assert got.data_ptr() == yd.data_ptr()
        else:
            out = at_offset(np.full(size, 7.0, dtype=f32), oy, dev)
            got = hip.ab_step(yd, fd, a, dt, out=out)
            assert np.array_equal(bits(yd.cpu().numpy()), bits(y))            # the state is only read
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (n, size, offsets)
        for f, d in zip(fs, fd):
            assert np.array_equal(bits(d.cpu().numpy()), bits(f))             # ... and so is the history


def test_ab_step_signed_zero_and_non_finite_values(dev):
    from ndcn_amd import hip
    n = 5
    a = ab.weights(n)
    # every product is -0.0: Python's sum() starts from an exact 0, so the sum is +0.0 and -0.0 + dt * (+0.0) = +0.0
    fs = [np.full(8, -0.0 if float(c) > 0 else 0.0, dtype=f32) for c in a]
    y = np.full(8, -0.0, dtype=f32)
    want = ab.ab_step(y, fs, a, f32(0.5))
    assert not np.signbit(want).any()
    got = hip.ab_step(T(y).to(dev), [T(f).to(dev) for f in fs], a, 0.5).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    # NaN and the infinities pass through as IEEE arithmetic has them (Inf - Inf and 0 * Inf are NaN; a NaN's payload is the machine's)
    rng = np.random.RandomState(5)
    y = rng.randn(64).astype(f32)
    fs = [rng.randn(64).astype(f32) for _ in range(n)]
    fs[0][3], fs[1][4], fs[2][5], fs[4][6] = np.nan, np.inf, -np.inf, np.inf
    fs[0][7], fs[1][7] = np.inf, np.inf                           # a[0] > 0 > a[1]: Inf - Inf
    y[8], y[9] = np.inf, np.nan
    fs[3][10] = np.inf
    want = ab.ab_step(y, fs, a, f32(0.25))
    assert np.isnan(want[[3, 7, 9]]).all() and np.isinf(want[[4, 5, 6, 8, 10]]).all()
    got = hip.ab_step(T(y).to(dev), [T(f).to(dev) for f in fs], a, 0.25).cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))
    # dt = 0 against an infinite sum: 0 * Inf = NaN, as the reference's dt * sum
    got0 = hip.ab_step(T(y).to(dev), [T(f).to(dev) for f in fs], a, 0.0).cpu().numpy()
    want0 = ab.ab_step(y, fs, a, f32(0))
    assert np.array_equal(np.isnan(got0), np.isnan(want0)) and np.isnan(got0[4])


def test_ab_step_refuses_bad_arguments_before_any_launch(dev):
    from ndcn_amd import _lib
    lib = _lib.load()
    size = 260
    y = torch.randn(size, device=dev)
    fs = [torch.randn(size, device=dev) for _ in range(12)]
    out = torch.full((size,), 7.0, device=dev)
    coef = (ctypes.c_float * 12)(*([0.5] * 12))

    def call(n, ptrs, o=out):
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        with torch.cuda.device(dev):
            return lib.ndcn_ab_step_f32(_lib.ptr(o), _lib.ptr(y), arr, coef, n, 0.1, size, _lib.stream_ptr())
    good = [f.data_ptr() for f in fs]
    for n in (0, 2, 12):
        assert call(n, good[:max(n, 1)]) == _lib.EINVAL
    assert call(3, [good[0], None, good[2]]) == _lib.EINVAL                       # a null term
    assert call(3, [good[0], out.data_ptr(), good[2]]) == _lib.EINVAL            # out aliases a history panel
    assert b'aliases' in lib.ndcn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                               # nothing was written
    assert call(3, good[:3]) == 0 and call(3, good[:3], o=y) == 0                 # ... and out == y is allowed
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------ the solves

def make_func(d, dev):
    from ndcn_amd import CsrOperator
    from ndcn_amd.neural_dynamics import ODEFunc
    A = CsrOperator.from_arrays(d['indptr'], d['indices'], d['data'], d['shape'], dev)
    f = ODEFunc(d['W'].shape[0], A, no_control=bool(int(d['no_control']))).to(dev)
    f.load_state_dict({'wt.weight': T(d['W']), 'wt.bias': T(d['b'])})
    return f.eval()


def options_of(d):
    o = {}
    if 'opt_max_order' in d:
        o['max_order'] = int(d['opt_max_order'])
    if 'opt_step_size' in d:
        o['step_size'] = float(d['opt_step_size'])
    return o


def check_traj(y, ref, l1=1e-5, mx=1e-4):
    """the bound tests/test_gpu_odeint.py::test_fixed_grid_golden applies to fixed_*.npz"""
    err = np.abs(y - ref)
    scale = max(1.0, np.abs(ref).max())
    assert err.mean() < l1 * scale, 'L1 %.3e' % err.mean()
    assert err.max() < mx * scale, 'max %.3e' % err.max()


@pytest.mark.parametrize('name', names())
def test_golden_on_both_paths(dev, name, monkeypatch):
    """generic path (a lambda around the ODEFunc: the device path declines) and device path (the ODEFunc itself) against the reference's
    trajectory; the two bit for bit equal to each other on every grid step; the warm-up the bits of method='rk4' on the same path"""
    from ndcn_amd import torchdiffeq as ode
    import importlib
    from ndcn_amd.torchdiffeq._impl import core
    impl = importlib.import_module('ndcn_amd.torchdiffeq._impl.odeint')       # (the package attribute of that name is the function)
    d = load_golden(name)
    f = make_func(d, dev)
    x0, t, opts = T(d['x0']).to(dev), T(d['t']).to(dev), options_of(d)
    taken = []
    real = impl._explicit_adams_solve
    monkeypatch.setattr(impl, '_explicit_adams_solve', lambda *a: taken.append(real(*a)) or taken[-1])
    with torch.no_grad():
        gen = ode.odeint(lambda tt, y: f(tt, y), x0, t, method='explicit_adams', options=dict(opts) or None)
        assert not taken
        res = ode.odeint(f, x0, t, method='explicit_adams', options=dict(opts) or None)
    # the library's solve ran for the plain ODEFunc (no_control has no form there: the generic path serves it)
    assert len(taken) == 1 and (taken[0] is None) == bool(int(d['no_control']))
    for y in (gen, res):
        assert y.shape == d['traj'].shape and np.array_equal(y[0].cpu().numpy(), d['x0'])
        check_traj(y.cpu().numpy(), d['traj'])
    assert torch.equal(gen, res)
    # every grid step: the solves on the explicit grid (each grid point a tick), again on both paths
    grid = T(ab.grid_of(d['t'], opts.get('step_size'))).to(dev)
    o2 = {k: v for k, v in opts.items() if k != 'step_size'}
    with torch.no_grad():
        gen_g = ode.odeint(lambda tt, y: f(tt, y), x0, grid, method='explicit_adams', options=dict(o2) or None)
        res_g = ode.odeint(f, x0, grid, method='explicit_adams', options=dict(o2) or None)
        rk_gen = ode.odeint(lambda tt, y: f(tt, y), x0, grid[:3], method='rk4')
        rk_res = ode.odeint(f, x0, grid[:3], method='rk4')
    assert torch.equal(gen_g, res_g)
    assert torch.equal(gen_g[:3], rk_gen) and torch.equal(res_g[:3], rk_res)
    # ... and the ticks of the step_size solve are the states at the steps that report them
    plan = core.fixed_plan(d['t'], opts.get('step_size'))
    for j in range(1, len(d['t'])):
        if plan.tick_coincident[j]:
            assert torch.equal(res[j], res_g[plan.tick_step[j] + 1])
        else:
            assert torch.equal(res[j], res_g[plan.tick_step[j] + 1] + 0.0)        # strictly inside: -0.0 becomes +0.0, finite values stay


def lattice_func(side, H, dev, seed=0):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(seed)
    f = ODEFunc(H, graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(side)), dev)).to(dev).eval()
    return f, torch.rand(side * side, H).to(dev)


@pytest.mark.parametrize('mid', [0, 2], ids=['composed', 'rhs_mid'])
@pytest.mark.parametrize('H', [20, 64])
def test_larger_graph_device_path_equals_generic_path(dev, H, mid):
    """a 40 x 40 lattice - beyond the one-launch solves - with the right-hand side dispatched to the composed launches and to rhs_mid"""
    from ndcn_amd import _lib
    from ndcn_amd import torchdiffeq as ode
    lib = _lib.load()
    f, x0 = lattice_func(40, H, dev)
    t = (torch.arange(15) / 128.0).to(dev)
    prev = lib.ndcn_set_rhs_mid(mid)
    try:
        with torch.no_grad():
            res = ode.odeint(f, x0, t, method='explicit_adams')
            torch.cuda.synchronize()
            path = int(lib.ndcn_debug_last_rhs_path())
            gen = ode.odeint(lambda tt, y: f(tt, y), x0, t, method='explicit_adams')
            sub = ode.odeint(f, x0, t[[0, 5, 14]], method='explicit_adams', options={'step_size': 1.0 / 128, 'max_order': 6})
            sub_gen = ode.odeint(lambda tt, y: f(tt, y), x0, t[[0, 5, 14]], method='explicit_adams', options={'step_size': 1.0 / 128, 'max_order': 6})
    finally:
        lib.ndcn_set_rhs_mid(prev)
    assert bool(path & _lib.PATH_MID) == (mid == 2)
    assert bool(torch.isfinite(res).all()) and torch.equal(res, gen)
    assert torch.equal(sub, sub_gen)


@pytest.mark.parametrize('max_order', [12, 4])
def test_evaluation_count(dev, max_order):
    from ndcn_amd import torchdiffeq as ode
    f, x0 = lattice_func(6, 8, dev)
    calls = []

    def counting(tt, y):
        calls.append(1)
        return f(tt, y)
    n_steps = 15
    with torch.no_grad():
        ode.odeint(counting, x0, torch.linspace(0., 0.15, n_steps + 1).to(dev), method='explicit_adams', options={'max_order': max_order})
    assert len(calls) == n_steps + 6
    del calls[:]
    with torch.no_grad():
        ode.odeint(counting, x0, torch.tensor([0., 9.5 / 128, 40 / 128]).to(dev), method='explicit_adams',
                   options={'max_order': max_order, 'step_size': 1 / 128})
    assert len(calls) == 40 + 6                                   # the reference's count on a step_size grid of 40 steps


# --------------------------------------------------------------------------------------------------------------------------- gradients

def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def fp64_solve(A, W, b, y0, t):
    """explicit_adams in float64 torch on the CPU with the exact rational weights: the function whose autograd is the truth"""
    f = lambda x: torch.relu((A @ x) @ W.t() + b)
    hist, y, sol = [], y0, [y0]
    for i in range(len(t) - 1):
        dt = t[i + 1] - t[i]
        hist.insert(0, f(y))
        del hist[11:]
        k = len(hist)
        if k < 3:
            k1 = hist[0]
            k2 = f(y + dt * k1 / 3)
            k3 = f(y + dt * (k1 / -3 + k2))
            k4 = f(y + dt * (k1 - k2 + k3))
            y = y + (k1 + 3 * k2 + 3 * k3 + k4) * (dt / 8)
        else:
            y = y + dt * sum(float(bi) * fi for bi, fi in zip(ab.betas(k), hist))
        sol.append(y)
    return torch.stack(sol)


def ea_steps(fun, y, dts):
    """explicit_adams over the step sizes `dts` (negative: backwards in time) on a list state in float64; fun: list -> list"""
    hist = []
    for dt in dts:
        hist.insert(0, fun(y))
        del hist[11:]
        k = len(hist)
        if k < 3:
            k1 = hist[0]
            k2 = fun([v + dt * a / 3 for v, a in zip(y, k1)])
            k3 = fun([v + dt * (a / -3 + b) for v, a, b in zip(y, k1, k2)])
            k4 = fun([v + dt * (a - b + c) for v, a, b, c in zip(y, k1, k2, k3)])
            y = [v + (a + 3 * b + 3 * c + d) * (dt / 8) for v, a, b, c, d in zip(y, k1, k2, k3, k4)]
        else:
            bs = [float(x) for x in ab.betas(k)]
            y = [v + dt * sum(bi * f[q] for bi, f in zip(bs, hist)) for q, v in enumerate(y)]
    return y


def fp64_adjoint(A, W, b, traj, g, t, substeps=1):
    """What odeint_adjoint computes (adjoint.py:34-103), restated in float64: per tick interval, last first, ONE solve of the augmented
    system (y, a, a_W, a_b)' = (f, -a^T df/dy, -a^T df/dW, -a^T df/db) from t[i] back to t[i-1] by the same method - a solve of its own,
    with its own warm-up, in `substeps` equal steps -, the vector-Jacobian products by torch autograd; then the tick's gradient enters."""
    def aug(s):
        y, a = s[0], s[1]
        with torch.enable_grad():
            y_, W_, b_ = (v.detach().requires_grad_(True) for v in (y, W, b))
            fe = torch.relu((A @ y_) @ W_.t() + b_)
            vy, vW, vb = torch.autograd.grad(fe, (y_, W_, b_), -a)
        return [fe.detach(), vy, vW, vb]
    a, aW, ab_ = g[-1], torch.zeros_like(W), torch.zeros_like(b)
    for i in range(len(t) - 1, 0, -1):
        dts = [(t[i - 1] - t[i]) / substeps] * substeps
        _, a, aW, ab_ = ea_steps(aug, [traj[i], a, aW, ab_], dts)
        a = a + g[i - 1]
    return a, aW, ab_


@pytest.mark.parametrize('mode', ['odeint', 'odeint_adjoint', 'odeint_adjoint_step_size'])
def test_gradients_against_fp64_autograd(dev, mode):
    """6 x 6 lattice, H = 8, 12 steps: the gradients of y0, W and b.
      odeint                     backpropagation through the solve (core.integrate_fixed over autograd_ops: ab_step is a linear map with
                                 the weights (1, dt a_0, ...)) against torch autograd through the float64 restatement of the solve;
      odeint_adjoint             the adjoint method is not the discrete gradient (it differs from it by the discretisation of the adjoint
                                 system: 8e-3 of the maximum here, measured) - the truth is the float64 restatement of the adjoint
                                 method itself, its vector-Jacobian products by torch autograd.  Every backward interval is a solve of
                                 its own on the augmented TUPLE state (the generic path): one RK4 step on the default grid;
      odeint_adjoint_step_size   the same with options={'step_size': a fifth of the tick spacing}: two RK4 and three Adams-Bashforth
                                 steps per interval, forward and backward.
    Tolerances of tests/test_gpu_autograd.py: 2e-4 of the tensor's maximum for backpropagation through a fixed grid
    (test_backprop_through_solver), 2e-3 for odeint_adjoint on one (test_odeint_adjoint_against_reference_gradients)."""
    from ndcn_amd import graphs
    from ndcn_amd import torchdiffeq as ode
    f, x0 = lattice_func(6, 8, dev, seed=3)
    x = x0.clone().requires_grad_(True)
    sub = 5 if mode == 'odeint_adjoint_step_size' else 1
    t = torch.arange(13) * ((5.0 if sub > 1 else 1.0) / 128)      # binary fractions: every step_size grid ends on its tick exactly
    opts = {'step_size': 1.0 / 128} if sub > 1 else None
    target = torch.rand(13, 36, 8, generator=torch.Generator().manual_seed(9))
    solve = ode.odeint if mode == 'odeint' else ode.odeint_adjoint
    y = solve(f, x, t.to(dev), method='explicit_adams', options=opts)
    loss = torch.nn.functional.l1_loss(y, target.to(dev))
    loss.backward()
    L = graphs.normalized_laplacian(graphs.grid_8_neighbor(6))
    A = torch.from_numpy(np.asarray(L.todense())).double()
    W = f.wt.weight.detach().cpu().double().requires_grad_(True)
    b = f.wt.bias.detach().cpu().double().requires_grad_(True)
    xc = x0.detach().cpu().double().requires_grad_(True)
    grid = torch.arange(12 * sub + 1).double() / 128 if sub > 1 else t.double()
    yo = fp64_solve(A, W, b, xc, grid)[::sub]
    lo = torch.nn.functional.l1_loss(yo, target.double())
    assert float((y.detach().cpu().double() - yo.detach()).abs().max()) < 1e-5
    assert abs(float(loss.detach()) - float(lo.detach())) < 1e-5
    if mode == 'odeint':
        lo.backward()
        want, tol = (xc.grad, W.grad, b.grad), 2e-4
    else:
        g = torch.autograd.grad(lo, yo)[0]
        want, tol = fp64_adjoint(A, W.detach(), b.detach(), yo.detach(), g, t.double(), substeps=sub), 2e-3
    for got, ref in zip((x.grad, f.wt.weight.grad, f.wt.bias.grad), want):
        assert rel(got.cpu().double(), ref) < tol


# -------------------------------------------------------------------------------------------------------------------------------- NDCN

def test_ndcn_forward_is_the_decoder_applied_to_the_hidden_solve(dev):
    from ndcn_amd import graphs, hip
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.neural_dynamics import NDCN
    S, H = 6, 8
    torch.manual_seed(1)
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(S)), dev)
    m = NDCN(input_size=1, hidden_size=H, A=A, num_classes=1, method='explicit_adams').to(dev).eval()
    x0 = torch.from_numpy(graphs.x0_blocks(S)[:S * S]).to(dev)
    t = torch.linspace(0., 0.12, 13).to(dev)
    with torch.no_grad():
        out = m(t, x0)
        hidden = ode.odeint(m.neural_dynamic_layer.odefunc, m.input_layer(x0), t, method='explicit_adams')
        want = hip.linear(hidden, m.output_layer.weight, m.output_layer.bias)
    assert out.shape == (13, S * S, 1) and bool(torch.isfinite(out).all())
    assert torch.equal(out, want)


def test_sharded_odeint_says_that_it_has_no_such_form(dev):
    from ndcn_amd import hip, sharding
    with pytest.raises(NotImplementedError, match='explicit_adams'):
        sharding.sharded_odeint(hip, None, None, 4, torch.zeros(4, 2, device=dev), torch.tensor([0., 1.], device=dev), method='explicit_adams')
