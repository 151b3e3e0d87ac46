"""The fixed-grid training nodes of ndcn_amd/torchdiffeq/_impl/fixed_train.py with the decoder as an optional input: the gradients they
return for subsets of their inputs, and the saved-tensor contract.  20 x 20 eight-neighbour lattice (400 rows), H = 64 - wide enough
that the one-launch pair declines -, C = 3, rk4.

odeint comes to these nodes only when the state or ODEFunc's parameters need a gradient (a decoder alone that does is decoded in a step
of its own), so the cases are put to the module's own routing function, which odeint calls with the same arguments.

Pinned elsewhere, not repeated here: an in-place edit of the returned trajectory of the plain _NativeFixedGrid and an in-place weight
change under _SmallEulerSolve and the dopri5 tape (test_gpu_tape.py); two runs of every decoder route giving the same bits
(test_gpu_readout_bwd.py::test_odeint_readout_under_a_gradient)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SIDE, H, C = 20, 64, 3
NODES = ('native', 'python', 'step_size')
SUBSETS = {'only_y0': ('y0',), 'only_Wd': ('Wd',), 'all_but_bd': ('y0', 'W', 'b', 'Wd')}
NAMES = ('y0', 'W', 'b', 'Wd', 'bd')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need a ROCm device'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def case(dev):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(SIDE)), dev)
    torch.manual_seed(4)
    f = ODEFunc(H, A).to(dev).train()
    g = torch.Generator().manual_seed(5)
    x0 = torch.rand(SIDE * SIDE, H, generator=g).to(dev)
    Wd = ((torch.rand(C, H, generator=g) - 0.5) * (2.0 / H ** 0.5)).to(dev)
    bd = (torch.rand(C, generator=g) - 0.5).to(dev)
    G = torch.randn(6, SIDE * SIDE, C, generator=g).to(dev)
    return f, x0, Wd, bd, G


def solve(case, node, wanted):
    """the decoded solution from `node` with requires_grad on the inputs named in `wanted` -> (out, {name: leaf})"""
    from ndcn_amd.ops import new_solve_epoch
    from ndcn_amd.torchdiffeq._impl import core, fixed_train
    f, x0, Wd, bd, _ = case
    f.wt.weight.requires_grad_('W' in wanted)
    f.wt.bias.requires_grad_('b' in wanted)
    f.zero_grad()
    leaves = dict(y0=x0.clone().requires_grad_('y0' in wanted), W=f.wt.weight, b=f.wt.bias,
                  Wd=Wd.clone().requires_grad_('Wd' in wanted), bd=bd.clone().requires_grad_('bd' in wanted))
    t, plan = torch.tensor([0., .25, .375, .625, 1.125, 1.25]), None
    if node == 'step_size':
        t = torch.tensor([0., .13, .5, .55, .6, 1.0])                 # .13, .55: strictly inside steps of 0.1; .5, .6: step ends
        plan = core.fixed_plan(t.numpy(), 0.1)
    if node == 'python':
        os.environ['NDCN_FIXED_GRID_NATIVE'] = '0'
    try:
        new_solve_epoch()
        out = fixed_train._fixed_grid_with_grad(f, leaves['y0'], t.to(x0.device), 'rk4', plan, readout=(leaves['Wd'], leaves['bd']))
    finally:
        os.environ.pop('NDCN_FIXED_GRID_NATIVE', None)
    want = {'native': '_NativeFixedGridBackward', 'python': '_FixedGridSolveBackward', 'step_size': '_SubstepSolveBackward'}[node]
    assert type(out.grad_fn).__name__ == want and out.shape == (6, SIDE * SIDE, C), (type(out.grad_fn).__name__, out.shape)
    return out, leaves


@pytest.fixture(scope='module')
def full(case):
    """per node: the gradients with everything requiring grad, computed once"""
    made = {}

    def get(node):
        if node not in made:
            out, leaves = solve(case, node, NAMES)
            (out * case[4]).sum().backward()
            made[node] = {k: v.grad.clone() for k, v in leaves.items()}
            assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in made[node].values())
        return made[node]
    return get


@pytest.mark.parametrize('subset', sorted(SUBSETS))
@pytest.mark.parametrize('node', NODES)
def test_decoder_gradient_subsets(case, full, node, subset):
    """None exactly where no gradient was asked for; where one was, the bits of the run that asked for all five"""
    ref = full(node)
    out, leaves = solve(case, node, SUBSETS[subset])
    (out * case[4]).sum().backward()
    for name in NAMES:
        g = leaves[name].grad
        if name not in SUBSETS[subset]:
            assert g is None, name
        else:
            assert g is not None and torch.equal(g, ref[name]), name


@pytest.mark.parametrize('node', NODES)
def test_saved_tensor_contract(case, node):
    """W, b, Wd and the trajectory are saved through autograd: a second reverse sweep over a retained graph gives the same bits, and an
    in-place write to W between forward and backward (one that changes no value) is refused"""
    out, leaves = solve(case, node, NAMES)
    loss = (out * case[4]).sum()
    first = torch.autograd.grad(loss, list(leaves.values()), retain_graph=True)
    second = torch.autograd.grad(loss, list(leaves.values()), retain_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    with torch.no_grad():
        leaves['W'].add_(0)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        loss.backward()
