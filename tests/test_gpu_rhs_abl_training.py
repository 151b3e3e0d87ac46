"""Whole training steps of the ablation models through the one-launch right-hand side (csrc/rhs_abl.hip, ndcn_set_rhs_abl) against the
same steps with the switch off.  NDCN(1, 20, ..., no_control=True) and NDCN(1, 20, ..., no_graph=True) on a 12 x 12 eight-neighbour
lattice, 5 ticks: method='dopri5' trains on the native tape, method='rk4' with dropout=0.5 on the fixed-grid sweep whose evaluations
carry a mask.  The route writes the composed launches' bits, so the decoded output, dopri5's step log and every parameter gradient of one
forward + backward are the SAME raw words; after the switched-on forward pass the last right-hand side of the thread reports
NDCN_PATH_ABL (with NDCN_PATH_DROP_EPI under dropout), after the switched-off one it does not."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
SIDE, H, TICKS = 12, 20, 5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need a ROCm device'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lattice(dev):
    from ndcn_amd import graphs
    return graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(SIDE)), dev)


@contextlib.contextmanager
def abl(on):
    from ndcn_amd import hip
    prev = hip.set_rhs_abl(on)
    try:
        yield
    finally:
        hip.set_rhs_abl(prev)


def rhs_path():
    from ndcn_amd import _lib
    return int(_lib.load().ndcn_debug_last_rhs_path())


def bits(t):
    return t.contiguous().view(torch.int32)


def step(dev, lattice, form, method, dropout):
    """one forward + backward of NDCN.forward's own sequence - encoder, the solve with the decoder as its readout - with the step log:
    (output, step log, {parameter: gradient}, path after the forward pass)"""
    from ndcn_amd import graphs
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.neural_dynamics import NDCN
    torch.manual_seed(0)
    model = NDCN(1, H, lattice, 1, dropout=dropout, rtol=.01, atol=.001, method=method, **{form: True}).to(dev)
    model.train(True)
    x0 = torch.from_numpy(graphs.x0_blocks(SIDE)[:SIDE * SIDE]).to(dev)
    t = torch.linspace(0., 1., TICKS).to(dev)
    w = torch.randn(TICKS, SIDE * SIDE, 1, generator=torch.Generator().manual_seed(1)).to(dev)
    log = []
    torch.manual_seed(5)                                       # the solve's dropout stream draws its seed from here
    block, dec = model.neural_dynamic_layer, model.output_layer
    y = ode.odeint(block.odefunc, model.input_layer(x0), t, rtol=block.rtol, atol=block.atol, method=block.method, step_log=log,
                   readout=(dec.weight, dec.bias))
    path = rhs_path()
    assert tuple(y.shape) == (TICKS, SIDE * SIDE, 1)
    (y * w).sum().backward()
    torch.cuda.synchronize()
    grads = {name: p.grad for name, p in model.named_parameters()}
    return y.detach(), log, grads, path


@pytest.mark.parametrize('method,dropout', [('dopri5', 0.0), ('rk4', 0.5)])
@pytest.mark.parametrize('form', ['no_control', 'no_graph'])
def test_training_step(dev, lattice, form, method, dropout):
    from ndcn_amd import _lib
    res = {}
    for on in (0, 1):
        with abl(on):
            res[on] = step(dev, lattice, form, method, dropout)
    want = _lib.PATH_ABL | (_lib.PATH_DROP_EPI if dropout else 0)
    assert res[1][3] & (_lib.PATH_ABL | _lib.PATH_DROP_EPI) == want, hex(res[1][3])
    assert res[0][3] & _lib.PATH_ABL == 0, hex(res[0][3])
    assert torch.equal(bits(res[0][0]), bits(res[1][0])), 'output differs'
    assert bool(torch.isfinite(res[1][0]).all())
    assert res[0][1] == res[1][1], 'step log differs'
    if method == 'dopri5':
        assert len(res[1][1]) > 1
    assert set(res[0][2]) == set(res[1][2]) and len(res[1][2]) >= 6
    for name, a in res[0][2].items():
        b = res[1][2][name]
        if 'odefunc.wt' in name and form == 'no_control':      # relu(A x) has no weight: no gradient reaches it
            assert a is None or float(a.abs().max()) == 0
            assert (a is None) == (b is None)
            if a is None:
                continue
        assert a is not None and b is not None and bool(torch.isfinite(a).all()), name
        assert torch.equal(bits(a), bits(b)), 'gradient of %s differs' % name
    assert any(g is not None and float(g.abs().max()) > 0 for g in res[1][2].values())
