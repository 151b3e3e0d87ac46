"""Training through explicit_adams on one autograd node (NDCN_ADAMS_TRAIN=1), on a real MI355X: the gather kernel ndcn_ab_adjoint_f32
bit for bit against the numpy float32 chain, the forward pass with a record (ndcn_explicit_adams_train_f32) against the
un-differentiated solve and against its own definition, the gradients of the node (fixed_train._ExplicitAdamsSolve) against torch
autograd through a float64 restatement of the solve, and which solves take the node."""
import ctypes

import numpy as np
import pytest
import torch

import _adams_bashforth as ab

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = (1, 3, 7, 1027)                     # below a 16-byte lane, head + tail only, one lane + tail, several workgroups
TOL = 2e-4                                  # tests/test_gpu_autograd.py: backpropagation through a fixed grid, of each tensor's maximum


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.asarray(a))


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def at_offset(a, off, dev):
    """a copy of the 1-d array on the device that starts `off` elements behind a 16-byte boundary"""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.size]
    v.copy_(T(a))
    return v


# ---------------------------------------------------------------------------------------------------------------- the gather kernel

def chain(gs, cs, base=None):
    """[base +] (((0 + c_0 g_0) + c_1 g_1) + ...) in numpy float32: every product and sum rounded on its own, the base added last"""
    with np.errstate(all='ignore'):
        s = (f32(0) + (f32(cs[0]) * gs[0]).astype(f32)).astype(f32)
        for c, g in zip(cs[1:], gs[1:]):
            s = (s + (f32(c) * g).astype(f32)).astype(f32)
        return s if base is None else (base + s).astype(f32)


@pytest.mark.parametrize('offsets', ['aligned', 'all_plus_one', 'mixed', 'out_is_base'])
@pytest.mark.parametrize('n', range(1, 12))
def test_ab_adjoint_bit_for_bit(dev, n, offsets):
    """every term count at sizes around the 16-byte lane, with and without a base, panels on / one element off / differently off a
    16-byte boundary, and the base updated in place"""
    from ndcn_amd import hip
    rng = np.random.RandomState(200 + n)
    for size in SIZES:
        for with_base in ((True,) if offsets == 'out_is_base' else (False, True)):
            gs = [rng.randn(size).astype(f32) for _ in range(n)]
            cs = (rng.randn(n) * 0.05).astype(f32)
            base = rng.randn(size).astype(f32) if with_base else None
            want = chain(gs, cs, base)
            oo = 1 if offsets == 'all_plus_one' else 0
            og = [(1 if offsets == 'all_plus_one' else (q % 4 if offsets == 'mixed' else 0)) for q in range(n)]
            gd = [at_offset(g, o, dev) for g, o in zip(gs, og)]
            bd = at_offset(base, 2 if offsets == 'mixed' else oo, dev) if with_base else None
            if offsets == 'out_is_base':
                got = hip.ab_adjoint(gd, cs, base=bd, out=bd)
                assert got.data_ptr() == bd.data_ptr()
            else:
                out = at_offset(np.full(size, 7.0, dtype=f32), oo, dev)
                got = hip.ab_adjoint(gd, cs, base=bd, out=out)
                if with_base:
                    assert np.array_equal(bits(bd.cpu().numpy()), bits(base))     # the base is only read
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (n, size, offsets, with_base)
            for g, d in zip(gs, gd):
                assert np.array_equal(bits(d.cpu().numpy()), bits(g))             # ... and so are the terms


def test_ab_adjoint_signed_zero_and_non_finite_values(dev):
    from ndcn_amd import hip
    n = 4
    cs = np.asarray([0.5, -0.25, 2.0, -1.0], dtype=f32)
    # every product is -0.0: the sum starts from an exact +0, so it is +0.0 - and a -0.0 base plus +0.0 is +0.0
    gs = [np.full(8, -0.0 if c > 0 else 0.0, dtype=f32) for c in cs]
    base = np.full(8, -0.0, dtype=f32)
    for bb in (None, base):
        want = chain(gs, cs, bb)
        assert not np.signbit(want).any()
        got = hip.ab_adjoint([T(g).to(dev) for g in gs], cs, base=None if bb is None else T(bb).to(dev)).cpu().numpy()
        assert np.array_equal(bits(got), bits(want))
    one = hip.ab_adjoint([T(gs[0]).to(dev)], cs[:1]).cpu().numpy()                 # a lone -0 product
    assert np.array_equal(bits(one), bits(np.zeros(8, dtype=f32)))
    # NaN and the infinities pass through as IEEE arithmetic has them (a NaN's payload is the machine's)
    rng = np.random.RandomState(6)
    gs = [rng.randn(64).astype(f32) for _ in range(n)]
    base = rng.randn(64).astype(f32)
    gs[0][3], gs[1][4], gs[2][5], gs[3][6] = np.nan, np.inf, -np.inf, np.inf
    gs[0][7], gs[1][7] = np.inf, np.inf                           # c[0] > 0 > c[1]: Inf - Inf
    base[8], base[9], base[10] = np.inf, np.nan, -np.inf
    gs[2][10] = np.inf                                            # +Inf from the sum onto a -Inf base
    for bb in (None, base):
        want = chain(gs, cs, bb)
        assert np.isnan(want[[3, 7]]).all() and np.isinf(want[[4, 5, 6]]).all()
        if bb is not None:
            assert np.isinf(want[8]) and np.isnan(want[[9, 10]]).all()
        got = hip.ab_adjoint([T(g).to(dev) for g in gs], cs, base=None if bb is None else T(bb).to(dev)).cpu().numpy()
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


def test_ab_adjoint_refuses_bad_arguments_before_any_launch(dev):
    from ndcn_amd import _lib
    lib = _lib.load()
    size = 260
    gs = [torch.randn(size, device=dev) for _ in range(12)]
    base = torch.randn(size, device=dev)
    out = torch.full((size,), 7.0, device=dev)
    coef = (ctypes.c_float * 12)(*([0.5] * 12))

    def call(n, ptrs, o=out, bb=None, n_elem=size):
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        with torch.cuda.device(dev):
            return lib.ndcn_ab_adjoint_f32(_lib.ptr(o), _lib.ptr(bb), arr, coef, n, n_elem, _lib.stream_ptr())
    good = [g.data_ptr() for g in gs]
    for n in (0, 12, -1):
        assert call(n, good[:max(n, 1)]) == _lib.EINVAL
    assert call(3, [good[0], None, good[2]]) == _lib.EINVAL                       # a null term
    assert call(3, [good[0], out.data_ptr(), good[2]]) == _lib.EINVAL            # out aliases a term
    assert b'aliases' in lib.ndcn_last_error()
    assert call(2, good[:2], n_elem=0) == 0                                       # nothing to do: no launch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                               # nothing was written
    keep = base.clone()
    assert call(1, good[:1]) == 0 and call(3, good[:3], o=base, bb=base) == 0     # one term; out == base is allowed
    torch.cuda.synchronize()
    assert torch.equal(out, 0.0 + 0.5 * gs[0])
    assert torch.equal(base, keep + (((0.0 + 0.5 * gs[0]) + 0.5 * gs[1]) + 0.5 * gs[2]))


# ----------------------------------------------------------------------------------------------------------- the forward with a record

def lattice_func(side, H, dev, seed=0):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(seed)
    f = ODEFunc(H, graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(side)), dev)).to(dev).eval()
    return f, torch.rand(side * side, H).to(dev)


T15 = torch.arange(15) / 128.0
# the issue's step_size plan (ticks on the grid, most steps report none) and one with a tick strictly inside a step
PLANS = {'default': (T15, None, 12), 'step_size': (T15[[0, 5, 14]], 1.0 / 128, 6),
         'step_size_loose': (torch.tensor([0., 4.5 / 128, 14.0 / 128]), 1.0 / 128, 6)}


def options_of(step_size, max_order):
    opts = {'max_order': max_order}
    if step_size is not None:
        opts['step_size'] = step_size
    return opts


@pytest.mark.parametrize('grid', sorted(PLANS))
@pytest.mark.parametrize('H', [20, 64])
def test_forward_record(dev, H, grid):
    """out is the un-differentiated solve bit for bit; rec_f[i] is the right-hand side at the state step i starts from; on the default
    grid the record of the states is the solution itself"""
    from ndcn_amd import _lib, hip
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.csr import as_csr
    from ndcn_amd.torchdiffeq._impl import core, fixed_train
    lib = _lib.load()
    f, x0 = lattice_func(40, H, dev)
    t, step_size, max_order = PLANS[grid]
    with torch.no_grad():
        want = ode.odeint(f, x0, t.to(dev), method='explicit_adams', options=options_of(step_size, max_order))
    plan = core.fixed_plan(t.numpy(), step_size)
    assert plan.default == (step_size is None)
    if grid == 'step_size_loose':
        assert not plan.tick_coincident[1] and plan.tick_coincident[2]
    dts, n_steps, steps, same, offs, n_emit = fixed_train.plan_arrays(plan)
    assert n_steps == 14
    csr = as_csr(f.A)
    csr.ensure_plans(H)
    W, b = f.wt.weight.detach().contiguous(), f.wt.bias.detach().contiguous()
    out = torch.full((n_emit + 1,) + tuple(x0.shape), 7.0, device=dev)
    out[0].copy_(x0)
    rec_f = torch.full((n_steps,) + tuple(x0.shape), 7.0, device=dev)
    rec_y = out[1:] if plan.default else torch.full((n_steps,) + tuple(x0.shape), 7.0, device=dev)
    nbytes = int(lib.ndcn_explicit_adams_train_workspace_bytes(x0.shape[0], H))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args = lambda nb: (csr.view_ref(), _lib.ptr(W), _lib.ptr(b), H, _lib.F_RELU, _lib.ptr(out[0]), dts, n_steps, steps, same, offs, n_emit,
                       max_order, _lib.ptr(out[1:]), _lib.ptr(rec_f), _lib.ptr(rec_y), _lib.ptr(ws), nb, _lib.stream_ptr())
    with torch.cuda.device(dev):
        assert lib.ndcn_explicit_adams_train_f32(*args(nbytes - 1)) == _lib.EINVAL        # the same argument checks as the solve
        torch.cuda.synchronize()
        assert bool((rec_f == 7.0).all())
        _lib.check(lib.ndcn_explicit_adams_train_f32(*args(nbytes)))
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    for i in range(n_steps):
        y = x0 if i == 0 else rec_y[i - 1]
        assert torch.equal(rec_f[i], hip.rhs(csr, y, W, b)), i
    for j in range(1, n_emit + 1):                                   # every tick is the state after the step that reports it
        y = rec_y[plan.tick_step[j]]
        assert torch.equal(out[j], y if plan.tick_coincident[j] else y + 0.0)


# --------------------------------------------------------------------------------------------------------------------------- gradients

def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def fp64_solve(A, W, b, y0, dts, max_order=12):
    """explicit_adams in float64 torch on the CPU with the exact rational weights: the function whose autograd is the truth.
    -> the states after every grid step, y0 first"""
    f = lambda x: torch.relu((A @ x) @ W.t() + b)
    hist, y, sol = [], y0, [y0]
    for dt in dts:
        hist.insert(0, f(y))
        del hist[max_order - 1:]
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


_DENSE = {}


def dense_operator(side):
    from ndcn_amd import graphs
    if side not in _DENSE:
        _DENSE[side] = torch.from_numpy(np.asarray(graphs.normalized_laplacian(graphs.grid_8_neighbor(side)).todense())).double()
    return _DENSE[side]


def check_gradients(dev, side, H, t, step_size=None, max_order=12, C=None, seed=3):
    """one loss.backward() through odeint with the switch on (set by the caller) against autograd through fp64_solve; -> the node's name"""
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.torchdiffeq._impl import core
    f, x0 = lattice_func(side, H, dev, seed=seed)
    x = x0.clone().requires_grad_(True)
    gen = torch.Generator().manual_seed(9)
    plan = core.fixed_plan(t.numpy(), step_size)
    n, n_ticks = side * side, len(t)
    Wd = bd = None
    if C is not None:
        Wd = (torch.randn(C, H, generator=gen) / 4).to(dev).requires_grad_(True)
        bd = torch.randn(C, generator=gen).to(dev).requires_grad_(True)
    target = torch.rand(n_ticks, n, C if C is not None else H, generator=gen)
    y = ode.odeint(f, x, t.to(dev), method='explicit_adams', options=options_of(step_size, max_order),
                   readout=None if C is None else (Wd, bd))
    name = type(y.grad_fn).__name__
    loss = torch.nn.functional.l1_loss(y, target.to(dev))
    loss.backward()
    W = f.wt.weight.detach().cpu().double().requires_grad_(True)
    b = f.wt.bias.detach().cpu().double().requires_grad_(True)
    xc = x0.detach().cpu().double().requires_grad_(True)
    states = fp64_solve(dense_operator(side), W, b, xc, [float(d) for d in plan.dts], max_order)
    yo = states[[0] + [int(s) + 1 for s in plan.tick_step[1:]]]               # a tick is the state after the step that reports it
    got, leaves = [x.grad, f.wt.weight.grad, f.wt.bias.grad], [xc, W, b]
    if C is not None:
        Wdc, bdc = (v.detach().cpu().double().requires_grad_(True) for v in (Wd, bd))
        yo = yo @ Wdc.t() + bdc
        got, leaves = got + [Wd.grad, bd.grad], leaves + [Wdc, bdc]
    lo = torch.nn.functional.l1_loss(yo, target.double())
    assert float((y.detach().cpu().double() - yo.detach()).abs().max()) < 1e-5
    assert abs(float(loss.detach()) - float(lo.detach())) < 1e-5
    lo.backward()
    worst = [rel(g.cpu().double(), leaf.grad) for g, leaf in zip(got, leaves)]
    print('explicit_adams training, %d x %d, H = %d, max_order %d, step_size %s, C %s: gradient errors of (y0, W, b%s) / max = %s'
          % (side, side, H, max_order, step_size, C, ', Wd, bd' if C is not None else '', ' '.join('%.2e' % w for w in worst)))
    assert all(w < TOL for w in worst), worst
    return name


NODE = '_ExplicitAdamsSolveBackward'
T13 = torch.arange(13) / 128.0


@pytest.mark.parametrize('max_order', [12, 5, 4, 3])
def test_gradients_small_lattice(dev, monkeypatch, max_order):
    """6 x 6, H = 8, 12 steps: order 11 reached / orders up to 4 / order 3 only / RK4 throughout"""
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '1')
    assert check_gradients(dev, 6, 8, T13, max_order=max_order) == NODE


@pytest.mark.parametrize('grid', ['step_size', 'step_size_loose'])
def test_gradients_on_a_step_size_plan(dev, monkeypatch, grid):
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '1')
    t, step_size, max_order = PLANS[grid]
    assert check_gradients(dev, 6, 8, t, step_size=step_size, max_order=max_order) == NODE


@pytest.mark.parametrize('grid', ['default', 'step_size'])
@pytest.mark.parametrize('C', [1, 3])
def test_gradients_with_the_decoder_inside_the_node(dev, monkeypatch, C, grid):
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '1')
    t, step_size, max_order = (T13, None, 12) if grid == 'default' else PLANS['step_size']
    assert check_gradients(dev, 6, 8, t, step_size=step_size, max_order=max_order, C=C) == NODE


@pytest.mark.parametrize('mid_bwd', [0, 2], ids=['composed', 'rhs_mid_bwd'])
def test_gradients_larger_lattice(dev, monkeypatch, mid_bwd):
    """40 x 40 - beyond the one-launch solves -, H = 20, 15 steps, the reverse evaluation composed and in one launch"""
    from ndcn_amd import _lib, hip
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '1')
    prev = hip.set_rhs_mid_bwd(mid_bwd)
    try:
        assert check_gradients(dev, 40, 20, torch.arange(16) / 128.0) == NODE
        torch.cuda.synchronize()
        path = int(_lib.load().ndcn_debug_last_rhs_vjp_path())
    finally:
        hip.set_rhs_mid_bwd(prev)
    assert path == (_lib.VJP_MID if mid_bwd == 2 else _lib.VJP_COMPOSED)


def test_ndcn_training_step(dev, monkeypatch):
    """NDCN(method='explicit_adams') in training mode, one loss.backward(): every parameter's gradient against the float64 model"""
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import NDCN
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '1')
    S, H = 6, 8
    torch.manual_seed(1)
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(S)), dev)
    m = NDCN(input_size=1, hidden_size=H, A=A, num_classes=1, method='explicit_adams').to(dev).train()
    x0 = torch.from_numpy(graphs.x0_blocks(S)[:S * S])
    target = torch.rand(13, S * S, 1, generator=torch.Generator().manual_seed(2))
    out = m(T13.to(dev), x0.to(dev))
    assert type(out.grad_fn).__name__ == NODE
    loss = torch.nn.functional.l1_loss(out, target.to(dev))
    loss.backward()
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    h = torch.tanh(x0.double() @ sd['input_layer.0.weight'].t() + sd['input_layer.0.bias']) @ sd['input_layer.2.weight'].t() + sd['input_layer.2.bias']
    states = fp64_solve(dense_operator(S), sd['neural_dynamic_layer.odefunc.wt.weight'], sd['neural_dynamic_layer.odefunc.wt.bias'], h,
                        [1.0 / 128] * 12)
    lo = torch.nn.functional.l1_loss(states @ sd['output_layer.weight'].t() + sd['output_layer.bias'], target.double())
    lo.backward()
    assert abs(float(loss.detach()) - float(lo.detach())) < 1e-5
    for name, p in m.named_parameters():
        assert rel(p.grad.cpu().double(), sd[name].grad) < TOL, name


# ------------------------------------------------------------------------------------------------------------------------------ routes

def test_the_node_takes_the_solve_and_its_forward_is_the_plain_solve(dev, monkeypatch):
    from ndcn_amd import torchdiffeq as ode
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '1')
    f, x0 = lattice_func(6, 8, dev, seed=3)
    t = T13.to(dev)
    for opts in (None, {'max_order': 5}, {'step_size': 1.0 / 256, 'max_order': 6}):
        with torch.no_grad():
            want = ode.odeint(f, x0, t, method='explicit_adams', options=opts)
        y = ode.odeint(f, x0.clone().requires_grad_(True), t, method='explicit_adams', options=opts)
        assert type(y.grad_fn).__name__ == NODE
        assert torch.equal(y.detach(), want)


def test_everything_else_keeps_its_route_and_its_gradients(dev, monkeypatch):
    """the switch off, a lambda, no_control, an active dropout: not the node - and a gradient all the same"""
    from ndcn_amd import graphs
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.neural_dynamics import ODEFunc
    f, x0 = lattice_func(6, 8, dev, seed=3)
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(6)), dev)
    torch.manual_seed(5)
    f_nc = ODEFunc(8, A, no_control=True).to(dev).eval()
    f_drop = ODEFunc(8, A, dropout=0.5).to(dev).train()
    t = T13.to(dev)

    def run(func):
        x = x0.clone().requires_grad_(True)
        y = ode.odeint(func, x, t, method='explicit_adams')
        y.sum().backward()
        assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
        return type(y.grad_fn).__name__
    monkeypatch.delenv('NDCN_ADAMS_TRAIN', raising=False)
    assert run(f) != NODE
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '0')
    assert run(f) != NODE
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '1')
    assert run(f) == NODE
    assert run(lambda tt, y: f(tt, y)) != NODE
    assert run(f_nc) != NODE
    assert run(f_drop) != NODE
    f_drop.eval()                                                    # dropout that is not active does not keep the node away
    assert run(f_drop) == NODE
