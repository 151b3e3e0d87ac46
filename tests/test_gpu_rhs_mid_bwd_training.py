"""Whole training steps with the one-launch reverse of the right-hand side (csrc/rhs_mid_bwd.hip) switched on - mode 2 of
ndcn_set_rhs_mid_bwd - against the same steps with it off: the route writes the composed launches' bits, so every parameter gradient
and the input gradient are EQUAL, not close.  72 x 72 lattice (5 184 rows: 81 weight-gradient chunks of 64 rows), H = 20 and 64 - too
large for the one-launch small solve (asserted), so the fixed grids train on the native sweep and dopri5 on the native tape, whose
reverse passes call the same rhs_vjp_f32 as ndcn_rhs_vjp_f32.  Each case asserts through ndcn_debug_last_rhs_vjp_path that the fused
reverse ran with the switch on and did not with it off, and counts the calls of hip.rhs_vjp: none on the native tapes (the library
ran the reverse itself), one on the per-operation path."""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
SIDE = 72
WIDTHS = (20, 64)
SWITCHES = ('NDCN_TAPE_DROPOUT', 'NDCN_TAPE_BUDGET_MB', 'NDCN_GRAD_TAPE')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need a ROCm device'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lattice(dev):
    from ndcn_amd import graphs
    return graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(SIDE)), dev)


@pytest.fixture
def calls(monkeypatch):
    """counts hip.rhs_vjp calls (the per-operation path's entry; the native tapes do not pass through it)"""
    from ndcn_amd import hip
    inner = hip.rhs_vjp
    seen = []

    def counted(*a, **k):
        seen.append(1)
        return inner(*a, **k)
    monkeypatch.setattr(type(hip), 'rhs_vjp', staticmethod(counted))
    return seen


@contextlib.contextmanager
def switch(mode):
    from ndcn_amd import hip
    prev = hip.set_rhs_mid_bwd(mode)
    try:
        yield
    finally:
        hip.set_rhs_mid_bwd(prev)


@contextlib.contextmanager
def environment(**env):
    assert not any(k in os.environ for k in SWITCHES)
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            del os.environ[k]


def route():
    from ndcn_amd import _lib
    return int(_lib.load().ndcn_debug_last_rhs_vjp_path())


def bits(t):
    return t.contiguous().view(torch.int32)


def func(lattice, dev, H, dropout=0.0):
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(0)
    return ODEFunc(H, lattice, dropout=dropout).to(dev)


def step(dev, lattice, H, method, dropout=0.0):
    """one training step's gradients: (loss, [g_x0, g_W, g_b], trajectory, autograd node name, route of the last reverse evaluation)"""
    from ndcn_amd import torchdiffeq as ode
    f = func(lattice, dev, H, dropout)
    f.train(True)
    x0 = torch.rand(SIDE * SIDE, H, generator=torch.Generator().manual_seed(2)).to(dev).requires_grad_(True)
    w = torch.randn(4, SIDE * SIDE, H, generator=torch.Generator().manual_seed(1)).to(dev)
    t = torch.linspace(0., 0.6, 4).to(dev)
    kw = dict(rtol=0.01, atol=0.001) if method == 'dopri5' else {}
    torch.manual_seed(5)
    y = ode.odeint(f, x0, t, method=method, **kw)
    loss = (y * w).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = [x0.grad] + [p.grad for p in f.parameters()]
    assert len(grads) == 3 and all(g is not None for g in grads)
    return loss.detach(), grads, y.detach(), type(y.grad_fn).__name__, route()


def compare(dev, lattice, H, method, calls, node, dropout=0.0):
    from ndcn_amd import _lib
    res = {}
    for mode in (0, 2):
        with switch(mode):
            res[mode] = step(dev, lattice, H, method, dropout)
    assert res[0][3].startswith(node) and res[2][3].startswith(node), (res[0][3], res[2][3])
    assert not calls, 'the native reverse pass went through hip.rhs_vjp'
    assert res[0][4] == _lib.VJP_COMPOSED and res[2][4] == _lib.VJP_MID, (res[0][4], res[2][4])
    assert torch.equal(bits(res[0][2]), bits(res[2][2]))
    assert torch.equal(bits(res[0][0]), bits(res[2][0]))
    for name, a, b in zip(('x0', 'W', 'b'), res[0][1], res[2][1]):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name
        assert torch.equal(bits(a), bits(b)), 'gradient of %s differs' % name


@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('method', ['rk4', 'euler'])
def test_fixed_grid_step(dev, lattice, calls, method, H):
    from ndcn_amd import _lib
    for m in (method,):
        assert _lib.load().ndcn_solve_small_supported(lattice.view_ref(), H, _lib.F_RELU, _lib.METHODS[m], 1) == 0      # not the one-launch solve
    compare(dev, lattice, H, method, calls, '_NativeFixedGrid')


@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('budget', [None, 0])
def test_dopri5_tape_step(dev, lattice, calls, budget, H):
    """the native tape, whole and with NDCN_TAPE_BUDGET_MB=0 (every attempt past the budget is re-formed in the reverse pass)"""
    from ndcn_amd.torchdiffeq._impl import tape
    env = {} if budget is None else {'NDCN_TAPE_BUDGET_MB': str(budget)}
    with environment(**env):
        compare(dev, lattice, H, 'dopri5', calls, '_TapeDopri5')
        if budget == 0:
            assert tape.last_record['thin_attempts'] > 0, tape.last_record


@pytest.mark.parametrize('H', WIDTHS)
def test_dopri5_tape_step_with_dropout(dev, lattice, calls, H):
    """dropout 0.5 under NDCN_TAPE_DROPOUT=1: the stored K' is the mask, s = 2 rides in acc_scale and the transposed SpMM's alpha"""
    with environment(NDCN_TAPE_DROPOUT='1'):
        compare(dev, lattice, H, 'dopri5', calls, '_TapeDopri5', dropout=0.5)


@pytest.mark.parametrize('dropout', [None, (0.5, 7, 3)])
@pytest.mark.parametrize('H', WIDTHS)
def test_per_operation_evaluation(dev, lattice, calls, H, dropout):
    """autograd_ops.rhs, one evaluation: its backward is ONE hip.rhs_vjp call with the switch on, the composed wrappers with it off"""
    from ndcn_amd import _lib, autograd_ops
    n = SIDE * SIDE
    res = {}
    for mode in (0, 2):
        del calls[:]
        with switch(mode):
            gen = torch.Generator(device=dev).manual_seed(4)
            x = (torch.rand(n, H, generator=gen, device=dev) - 0.3).requires_grad_(True)
            W = ((torch.rand(H, H, generator=gen, device=dev) - 0.5) / 4).requires_grad_(True)
            b = ((torch.rand(H, generator=gen, device=dev) - 0.5) / 4).requires_grad_(True)
            w = torch.randn(n, H, generator=gen, device=dev)
            y = autograd_ops.rhs(lattice, x, W, b, False, False, dropout)
            (y * w).sum().backward()
            torch.cuda.synchronize()
            res[mode] = (y.detach(), [x.grad, W.grad, b.grad], len(calls), route())
    assert res[0][2] == 0 and res[2][2] == 1, (res[0][2], res[2][2])
    assert res[2][3] == _lib.VJP_MID
    assert torch.equal(bits(res[0][0]), bits(res[2][0]))
    for name, a, c in zip(('x', 'W', 'b'), res[0][1], res[2][1]):
        assert a is not None and float(a.abs().max()) > 0, name
        assert torch.equal(bits(a), bits(c)), 'gradient of %s differs' % name
