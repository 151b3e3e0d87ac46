"""Whole solves with the one-launch right-hand side for hidden widths 16..128 (csrc/rhs_mid.hip) switched on - mode 1 of
ndcn_set_rhs_mid - against the same solves with it off: the route writes the composed path's bits, so trajectories, step logs, losses
and gradients are EQUAL, not close.  70 x 70 lattice, H = 64: 313 600 elements - above 2^18, where the narrow-panel kernel stops and
mode 1 applies, and below 2^23, so the device solver replays a captured graph of the step (the launch sits inside a hipGraph)."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
SIDE, H = 70, 64


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need a ROCm device'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lattice(dev):
    from ndcn_amd import graphs
    return graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(SIDE)), dev)


@contextlib.contextmanager
def mid(mode):
    from ndcn_amd import hip
    prev = hip.set_rhs_mid(mode)
    try:
        yield
    finally:
        hip.set_rhs_mid(prev)


def rhs_path():
    from ndcn_amd import _lib
    return int(_lib.load().ndcn_debug_last_rhs_path())


def func(lattice, dev):
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(0)
    return ODEFunc(H, lattice).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('method', ['dopri5', 'rk4', 'euler'])
def test_inference(dev, lattice, method):
    from ndcn_amd import _lib
    from ndcn_amd import torchdiffeq as ode
    assert SIDE * SIDE * H > 1 << 18
    x0 = torch.rand(SIDE * SIDE, H, generator=torch.Generator().manual_seed(2)).to(dev)
    t = torch.linspace(0., 1., 5).to(dev)
    res = {}
    for mode in (0, 1):
        with mid(mode), torch.no_grad():
            f = func(lattice, dev)
            log = []
            kw = dict(rtol=0.01, atol=0.001, step_log=log) if method == 'dopri5' else {}
            y = ode.odeint(f, x0, t, method=method, **kw)
            torch.cuda.synchronize()
            res[mode] = (y, log, rhs_path())
    assert res[0][2] & _lib.PATH_MID == 0, hex(res[0][2])
    assert res[1][2] & _lib.PATH_MID, hex(res[1][2])
    assert res[0][1] == res[1][1]
    if method == 'dopri5':
        assert len(res[0][1]) > 0
    assert torch.equal(bits(res[0][0]), bits(res[1][0]))
    assert bool(torch.isfinite(res[1][0]).all())


@pytest.mark.parametrize('method', ['rk4', 'dopri5'])
def test_training(dev, lattice, method):
    """rk4: the fixed-grid training path, whose stages ride in the right-hand-side launches; dopri5: the native tape"""
    from ndcn_amd import _lib
    from ndcn_amd import torchdiffeq as ode
    x0h = torch.rand(SIDE * SIDE, H, generator=torch.Generator().manual_seed(2))
    w = torch.randn(5, SIDE * SIDE, H, generator=torch.Generator().manual_seed(1)).to(dev)
    t = torch.linspace(0., 1., 5).to(dev)
    res = {}
    for mode in (0, 1):
        with mid(mode):
            f = func(lattice, dev)
            x0 = x0h.clone().to(dev).requires_grad_(True)
            log = []
            kw = dict(rtol=0.01, atol=0.001, step_log=log) if method == 'dopri5' else {}
            y = ode.odeint(f, x0, t, method=method, **kw)
            path = rhs_path()                                  # (of the forward solve: the reverse pass has launches of its own)
            loss = (y * w).sum()
            loss.backward()
            torch.cuda.synchronize()
            grads = [x0.grad] + [p.grad for p in f.parameters()]
            assert len(grads) == 3 and all(g is not None for g in grads)
            res[mode] = (loss.detach(), grads, log, path, y.detach())
    if method == 'dopri5':
        # (rk4: the step's last launch asks for no K - RkOpt::no_k, a field the route declines - so the path left behind is the composed
        # one; the three launches before it took the route)
        assert res[1][3] & _lib.PATH_MID, hex(res[1][3])
    assert res[0][2] == res[1][2]
    assert torch.equal(bits(res[0][4]), bits(res[1][4]))
    assert torch.equal(bits(res[0][0]), bits(res[1][0]))
    for name, a, b in zip(('y0', 'W', 'b'), res[0][1], res[1][1]):
        assert torch.equal(bits(a), bits(b)), 'gradient of %s differs' % name
