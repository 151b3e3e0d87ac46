"""The static-GCN modules under gradients: ode_gcn.ResBlock in its six configurations, models.GCN and the resGCN Sequential of
drivers/dgnn.py against the float64 restatement tests/_resgcn.py - outputs, the gradient of the input and of every parameter (through
autograd_ops.spmm / linear, ode_gcn._RowNorm and the learnable time_step) -, the no-grad route against the gradient route, the
`stochastic` branch with a known mask, and one short driver run that must reach the reverse row-norm kernel.

Bounds (tests/test_gpu_tgcn.py): outputs within 1e-5, gradients within 2e-4 of each tensor's maximum.  (The same restatement run in
float32 on the host needs 1.1e-7 for the outputs and 2.7e-6 for the gradients of the ResBlock cases against its float64 run.)

Inputs: the drivers' power-law graph (300 nodes) under dgnn's operator with one node cut off (an empty CSR row), features relu(randn) at
H = 20 (vector row-norm kernel) and H = 33 (two-pass kernel).  Conditions, asserted in every case on its float64 run: no ReLU
pre-activation other than an exact zero within 1e-6 of zero, no normalised row's L1 norm within a factor 2 of the clamp at 1e-12."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _resgcn
from conftest import load_golden

pytestmark = pytest.mark.gpu
OUT_TOL, GRAD_TOL = 1e-5, 2e-4
N = 300
CONFIGS = {'plain': {}, 'normalize': dict(normalize=True), 'time_varying': dict(time_varying=True), 'Euler': dict(Euler=True),
           'normalize_time_varying': dict(normalize=True, time_varying=True), 'normalize_Euler': dict(normalize=True, Euler=True)}
WIDTHS = (20, 33)
# feature draws chosen on the host so that every case meets the input conditions; (mask, configuration, H) -> draw, 0 where not listed
DRAWS = {(False, 'normalize_time_varying', 33): 2}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def graph(dev):
    """(the device operator, the same matrix dense in float64 on the host)"""
    from ndcn_amd import CsrOperator
    m = _resgcn.graph(N, seed=0)
    return CsrOperator.from_scipy(m, device=dev), torch.from_numpy(m.toarray().astype(np.float64))


def err(got, want):
    """max |got - want| over max |want| (0 / 0 = 0)"""
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    d = float((got - want).abs().max())
    return 0.0 if d == 0.0 else d / float(want.abs().max())


def block_seed(masked, config, H):
    return (200 if masked else 100) + H + 1000 * DRAWS.get((masked, config, H), 0)


def features(H, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(N, H, generator=g))
    assert bool((x.abs().sum(1) > 0.1).all())                      # no all-zero input row (clamped rows: tests/test_gpu_rownorm.py)
    return x, torch.randn(N, H, generator=g), ((torch.rand(N, H, generator=g) < 0.5).float() * 2.0)


class FixedMask(nn.Module):
    """stands in for nn.Dropout(0.5): a known 0 / 2 panel"""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, f):
        return f * self.mask


def make_block(H, config, A, dev, mask=None):
    from ndcn_amd.ode_gcn import ResBlock
    torch.manual_seed(11 + H)
    blk = ResBlock(H, A, dropout=0 if mask is None else 0.5, **CONFIGS[config]).to(dev).train()
    if mask is not None:
        blk.dropout_layer = FixedMask(mask.to(dev))
    return blk


def block_in_float64(blk, Ad, x, R, mask=None):
    """(output, {name: gradient}) of sum(block(x) * R) in float64, the input conditions asserted"""
    p = {k: v.detach().cpu().double().requires_grad_() for k, v in blk.named_parameters()}
    x64 = x.double().requires_grad_()
    pre, norms = [], []
    out = _resgcn.block(Ad, x64, p.get('linear.weight'), p.get('linear.bias'), p.get('time_step', 1.0), blk.normalize,
                        None if mask is None else mask.double(), pre, norms)
    assert _resgcn.clear_of_the_kink(pre) and _resgcn.clear_of_the_clamp(norms)
    (out * R.double()).sum().backward()
    grads = {k: v.grad for k, v in p.items()}
    grads['x'] = x64.grad
    return out.detach(), grads


def block_on_device(blk, x, R, dev):
    blk.zero_grad()
    xd = x.to(dev).requires_grad_()
    out = blk(xd)
    (out * R.to(dev)).sum().backward()
    grads = {k: v.grad for k, v in blk.named_parameters()}
    grads['x'] = xd.grad
    return out.detach(), grads


def assert_block(got, want, what):
    (out, grads), (wout, wgrads) = got, want
    assert err(out, wout) <= OUT_TOL, (what, 'output', err(out, wout))
    assert set(grads) == set(wgrads)
    for k in sorted(wgrads):
        assert grads[k] is not None and err(grads[k], wgrads[k]) <= GRAD_TOL, (what, k, err(grads[k], wgrads[k]))


@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_resblock_under_gradients(dev, graph, config, H):
    A, Ad = graph
    x, R, _ = features(H, block_seed(False, config, H))
    blk = make_block(H, config, A, dev)
    want_names = {'x'} | ({'linear.weight', 'linear.bias'} if 'time_varying' in config else set()) | ({'time_step'} if 'Euler' in config else set())
    got = block_on_device(blk, x, R, dev)
    assert set(got[1]) == want_names
    assert_block(got, block_in_float64(blk, Ad, x, R), (config, H))


@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_resblock_no_grad_route_has_the_gradient_route_s_words(dev, graph, config, H):
    """ode_gcn's claim: ReLU fused into the SpMM or Linear, and fixed_stage op 0 rounding the product before the sum, give the words of
    the composed route"""
    A, Ad = graph
    x, R, _ = features(H, block_seed(False, config, H))
    blk = make_block(H, config, A, dev)
    with_grad = blk(x.to(dev).requires_grad_())
    assert with_grad.requires_grad
    for mode in ('train', 'eval'):
        getattr(blk, mode)()
        with torch.no_grad():
            plain = blk(x.to(dev))
        assert not plain.requires_grad and torch.equal(plain, with_grad.detach()), (config, H, mode)
    assert err(plain, block_in_float64(blk, Ad, x, R)[0]) <= OUT_TOL


@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_resblock_with_a_known_dropout_mask(dev, graph, config, H):
    A, Ad = graph
    x, R, mask = features(H, block_seed(True, config, H))
    blk = make_block(H, config, A, dev, mask=mask)
    want = block_in_float64(blk, Ad, x, R, mask)
    got = block_on_device(blk, x, R, dev)
    assert_block(got, want, (config, H))
    with torch.no_grad():                                           # the `stochastic` branch: training mode, no gradients
        assert blk.training and blk.dropout > 0
        out = blk(x.to(dev))
    assert not out.requires_grad and err(out, want[0]) <= OUT_TOL
    assert torch.equal(out, got[0])
    blk.eval()                                                      # eval: the fused route, which applies no mask
    unmasked = block_in_float64(blk, Ad, x, R)[0]
    with torch.no_grad():
        assert err(blk(x.to(dev)), unmasked) <= OUT_TOL


def test_gcn_under_gradients(dev, graph):
    from ndcn_amd.models import GCN
    A, Ad = graph
    x, _, _ = features(33, 300)
    R = torch.randn(N, 7, generator=torch.Generator().manual_seed(5))
    torch.manual_seed(3)
    m = GCN(33, 16, 7, dropout=0, num_middle_layers=1).to(dev).train()
    xd = x.to(dev).requires_grad_()
    out = m(xd, A)
    (out * R.to(dev)).sum().backward()
    p = {k: v.detach().cpu().double().requires_grad_() for k, v in m.named_parameters()}
    assert set(p) == {a + '.fc.' + b for a in ('gc1', 'gc2', 'conv_middle.0') for b in ('weight', 'bias')}
    x64 = x.double().requires_grad_()
    pre = []
    want = _resgcn.gcn(Ad, x64, p, 1, pre)
    assert _resgcn.clear_of_the_kink(pre)
    (want * R.double()).sum().backward()
    assert err(out, want) <= OUT_TOL
    assert err(xd.grad, x64.grad) <= GRAD_TOL
    for k, v in m.named_parameters():
        assert err(v.grad, p[k].grad) <= GRAD_TOL, (k, err(v.grad, p[k].grad))
    with torch.no_grad():                                           # hip.gcn: Linear -> SpMM in one call
        fused = m(x.to(dev), A)
    assert err(fused, want) <= OUT_TOL and err(fused, out.detach().cpu()) <= OUT_TOL


def test_resgcn_sequential_takes_one_cross_entropy_step(dev, graph):
    """the model as drivers/dgnn.py builds it for --model resGCN --normalize --Euler -nhl 2 --dropout 0"""
    from ndcn_amd.ode_gcn import ResBlock
    A, Ad = graph
    feats, _, _ = features(33, 400)
    g = torch.Generator().manual_seed(6)
    labels, idx = torch.randint(0, 7, (N,), generator=g), torch.randperm(N, generator=g)[:40]
    torch.manual_seed(4)
    model = nn.Sequential(nn.Linear(33, 20, bias=True), nn.ReLU(inplace=True),
                          *[ResBlock(20, A, dropout=0, normalize=True, Euler=True) for _ in range(2)],
                          nn.Linear(20, 7, bias=True)).to(dev).train()
    loss = F.cross_entropy(model(feats.to(dev))[idx.to(dev)], labels.to(dev)[idx.to(dev)])
    loss.backward()
    p = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    assert set(p) == {'0.weight', '0.bias', '2.time_step', '3.time_step', '4.weight', '4.bias'}
    pre, norms = [], []
    want = F.cross_entropy(_resgcn.resgcn(Ad, feats.double(), p, 2, True, pre, norms)[idx], labels[idx])
    assert _resgcn.clear_of_the_kink(pre) and _resgcn.clear_of_the_clamp(norms) and len(norms) == 4
    want.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= OUT_TOL * abs(float(want.detach()))
    for k, v in model.named_parameters():
        assert err(v.grad, p[k].grad) <= GRAD_TOL, (k, err(v.grad, p[k].grad))


def cora(dev):
    from ndcn_amd import CsrOperator
    import scipy.sparse as sp
    d, g = load_golden('dataset_cora'), load_golden('operators_cora')
    n = int(g['n'])
    adj = CsrOperator.from_arrays(g['alpha00_indptr'], g['alpha00_indices'], g['alpha00_data'], (n, n), dev)
    feats = sp.csr_matrix((d['feat_data'], d['feat_indices'].astype(np.int64), d['feat_indptr']), shape=tuple(d['feat_shape']))
    ix = lambda k: torch.from_numpy(d[k].astype(np.int64)).to(dev)
    return adj, torch.from_numpy(feats.toarray()).to(dev), ix('labels'), ix('idx_train'), ix('idx_val'), ix('idx_test')


def test_driver_reaches_the_reverse_row_norm_kernel(dev, monkeypatch):
    from ndcn_amd import hip
    from ndcn_amd.drivers import dgnn
    calls, real = [], hip.row_l1_normalize_bwd

    def counted(g, X):
        calls.append(tuple(X.shape))
        return real(g, X)

    monkeypatch.setattr(hip, 'row_l1_normalize_bwd', counted)
    accs = dgnn.main(['--dataset', 'cora', '--model', 'resGCN', '-nhl', '2', '--hidden', '64', '--dropout', '0.5', '--normalize', '--Euler',
                      '--epochs', '3', '--weight_decay', '5e-4', '--alpha', '0', '--seed', '0'], data=cora(dev), quiet=True)
    assert accs.shape == (1,) and np.isfinite(accs).all() and 0.0 <= float(accs[0]) <= 1.0
    # two blocks, two normalisations each, three epochs: every one of them has an upstream that requires grad
    assert len(calls) == 12 and set(calls) == {(2708, 64)}
