"""The one-launch reverse of the no_control / no_graph ablations for hidden widths 16..128 (csrc/rhs_abl_bwd.hip, NDCN_VJP_ABL,
ndcn_set_rhs_abl_bwd) against the composed launches - no_control: relu_bwd into a scratch panel, transposed SpMM; no_graph:
ndcn_linear_bwd_f32's three launches plus the scaling pass - BIT FOR BIT: gX, gW and gb are compared as int32 (torch.equal on the raw
words: +0 / -0 and NaN positions count).  Every case calls ndcn_rhs_vjp_f32 with the switch on and off and asserts the route through
ndcn_debug_last_rhs_vjp_path.

Graphs, inputs and shapes are those of tests/test_gpu_rhs_mid_bwd.py (its docstring derives them from the chunking of the weight
gradient, which the no_graph route shares; `chunks` there): n = 37, 100, 4097, 20000 x H = 16, 20, 64, 96, 100, 128 on the 8-neighbour
lattice and on the ragged graph with empty rows, 1..3-entry rows (the gather's remainder loop) and a 300-entry hub; a NaN and a -0.0
planted in g and in K.  For the no_control kernel, whose tiles are 64 rows of the transposed operator dealt over the persistent grid,
the same sizes give one partial tile (37), two tiles (100), a last tile of ONE row (4097) and 313 tiles (20000)."""
import contextlib

import numpy as np
import pytest
import torch

from _fma_chain import chain
from test_gpu_rhs_mid_bwd import SIZES, WIDTHS, U, GRAPHS, bits, chunks, inputs, op, same

pytestmark = pytest.mark.gpu
FORMS = ('no_control', 'no_graph')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from ndcn_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _L():
    from ndcn_amd import _lib
    return _lib


def route():
    return int(_L().load().ndcn_debug_last_rhs_vjp_path())


@contextlib.contextmanager
def switch(on):
    from ndcn_amd import hip
    prev = hip.set_rhs_abl_bwd(on)
    try:
        yield
    finally:
        hip.set_rhs_abl_bwd(prev)


def call(A, X, W, K, g, on, want_route=None, **kw):
    """(gX, gW, gb) of hip.rhs_vjp with the switch at `on`; the route is asserted (default: NDCN_VJP_ABL when on, composed when off)"""
    from ndcn_amd import hip
    with switch(on):
        out = hip.rhs_vjp(A, X, W, K, g, **kw)
        torch.cuda.synchronize()
        got = route()
    if want_route is None:
        want_route = _L().VJP_ABL if on else _L().VJP_COMPOSED
    assert got == want_route, (on, got, want_route, kw)
    return out


def both(A, X, W, K, g, what, want_route=None, **kw):
    """the call with the switch on and off: equal words in (gX, gW, gb); accumulating calls start from the same totals"""
    acc = kw.pop('acc', None)
    outs = []
    for on in (1, 0):
        k2 = dict(kw)
        if acc is not None:
            k2['gW'], k2['gb'] = acc[0].clone(), (acc[1].clone() if kw.get('need_b', True) else None)
        outs.append(call(A, X, W, K, g, on, want_route=(want_route if on else None), **k2))
    for name, a, b in zip(('gX', 'gW', 'gb'), outs[0], outs[1]):
        same(a, b, '%s %s' % (what, name))
    return outs[0]


@pytest.mark.parametrize('kind', sorted(GRAPHS))
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('form', FORMS)
def test_equal_words(dev, form, H, n, kind):
    A, _ = op(kind, n, dev)
    X, K, g, W = inputs(n, H, 100 * H + n % 97, dev)
    gX, gW, gb = both(A, X, W, K, g, form, **{form: True})
    assert gX is not None and bool(torch.isnan(gX).any())        # the planted NaNs arrive
    if form == 'no_graph':
        assert gW is not None and gb is not None and bool(torch.isnan(gW).any())
    else:
        assert gW is None and gb is None
    both(A, X, W, K, g, form + ', scale 2', acc_scale=2.0, **{form: True})


@pytest.mark.parametrize('form', FORMS)
def test_equal_words_variants(dev, form):
    """one size, the lattice: gX not wanted, gb not wanted, acc_scale = 2, accumulating into given gW / gb"""
    n, H = 4097, 20
    A, _ = op('lattice', n, dev)
    X, K, g, W = inputs(n, H, 11, dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    acc = (torch.randn(H, H, generator=gen, device=dev), torch.randn(H, generator=gen, device=dev))
    graph = form == 'no_graph'
    # no_control without gX has nothing to do: the route declines
    out = both(A, X, W, K, g, 'gX null', need_x=False, want_route=None if graph else _L().VJP_COMPOSED, **{form: True})
    assert out[0] is None and (out[1] is not None) == graph
    out = both(A, X, W, K, g, 'gb null', need_b=False, **{form: True})
    assert out[2] is None
    for scale in (1.0, 2.0):
        out = both(A, X, W, K, g, 'accumulate, scale %g' % scale, acc=acc, acc_scale=scale, **{form: True})
        if graph:
            assert not torch.equal(bits(out[1]), bits(acc[0]))
    both(A, X, W, K, g, 'accumulate, gb null', acc=acc, acc_scale=2.0, need_b=False, **{form: True})
    both(A, X, W, K, g, 'gX null, accumulate', acc=acc, acc_scale=2.0, need_x=False,
         want_route=None if graph else _L().VJP_COMPOSED, **{form: True})
    if graph:                                                  # the forms of gZ the composed call knows, through the same launch
        both(A, X, W, K, g, 'no ReLU', relu=False, acc_scale=2.0, no_graph=True)
        gz = torch.where((K.cpu() <= 0).to(dev), torch.zeros_like(g), g)
        pre = both(A, X, W, K, gz, 'premasked', premasked=True, no_graph=True)
        ref = call(A, X, W, K, g, 1, no_graph=True)
        for name, a, b in zip(('gX', 'gW', 'gb'), pre, ref):
            same(a, b, 'premasked against masked %s' % name)


@pytest.mark.parametrize('alpha', (1.0, 2.0))
@pytest.mark.parametrize('H', (20, 64))
@pytest.mark.parametrize('kind', sorted(GRAPHS))
def test_no_control_against_the_host_chain(dev, kind, H, alpha):
    """gX = the sequential fma chain of tests/_fma_chain.py over At, applied to g masked by K, then times alpha - bit for bit"""
    n = 4097
    A, _ = op(kind, n, dev)
    X, K, g, W = inputs(n, H, 21, dev)
    gX, _, _ = call(A, X, W, K, g, 1, no_control=True, acc_scale=alpha)
    mt = A.transpose().to_scipy().tocsr()
    Kc, gc = K.cpu().numpy(), g.cpu().numpy()
    gz = np.where(Kc <= 0, np.float32(0.0), gc).astype(np.float32)      # a NaN K passes
    want = torch.from_numpy(chain(mt.indptr, mt.indices, mt.data, gz, alpha=alpha)).to(dev)
    same(gX, want, 'gX against the fma chain of A^T over the masked g')


def test_no_graph_against_fp64(dev):
    """n = 20000, H = 64: gX = 2 gZ W, gW = 2 gZ^T X, gb = 2 colsum gZ against fp64 products of the same fp32 inputs, to the bounds
    test_against_fp64_and_the_fma_chain of tests/test_gpu_rhs_mid_bwd.py uses for gS / gW / gb - per element (Ho + 2) u sum |gZ W|,
    1.01 u (rows_per_chunk + chunks) sum |gZ X|, 1.01 u (rows_per_chunk + chunks + 1) sum |gZ|, u = 2^-24; acc_scale = 2 is exact in
    fp32, so the bounds scale with it.  No NaN is planted here (as there): every element is compared."""
    n, H = 20000, 64
    gen = torch.Generator(device=dev).manual_seed(9)
    X = torch.randn(n, H, generator=gen, device=dev)
    g = torch.randn(n, H, generator=gen, device=dev)
    K = torch.relu(torch.randn(n, H, generator=gen, device=dev))
    K[::5, 3] = -0.0
    W = (torch.rand(H, H, generator=gen, device=dev) - 0.5) / 4
    gX, gW, gb = call(None, X, W, K, g, 1, no_graph=True, acc_scale=2.0)
    gz = torch.where((K.cpu() <= 0).to(dev), torch.zeros_like(g), g).double()
    Wd, Xd = W.double(), X.double()

    def within(got, ref, bound, what):
        err = (got.double() - ref).abs()
        bad = ~(err <= bound)
        print('%s: largest error / bound = %.3f' % (what, float((err / bound.clamp_min(1e-300)).max())))
        assert not bool(bad.any()), '%s: %d elements out of bound' % (what, int(bad.sum()))

    rpc, used, _ = chunks(n)
    within(gX, 2.0 * (gz @ Wd), 2.0 * (H + 2) * U * (gz.abs() @ Wd.abs()), 'gX')
    within(gW, 2.0 * (gz.t() @ Xd), 2.0 * 1.01 * U * (rpc + used) * (gz.abs().t() @ Xd.abs()), 'gW')
    within(gb, 2.0 * gz.sum(0), 2.0 * 1.01 * U * (rpc + used + 1) * gz.abs().sum(0), 'gb')


@pytest.mark.parametrize('form', FORMS)
def test_two_calls_give_the_same_words(dev, form):
    n, H = 4097, 96
    A, _ = op('ragged', n, dev)
    X, K, g, W = inputs(n, H, 3, dev)
    a = call(A, X, W, K, g, 1, acc_scale=2.0, **{form: True})
    b = call(A, X, W, K, g, 1, acc_scale=2.0, **{form: True})
    for name, u, v in zip(('gX', 'gW', 'gb'), a, b):
        same(u, v, name)


def test_declined_calls_run_composed(dev):
    """switch on: other widths, both flags, no_control without a mask to fuse and a misaligned g take the composed launches and give
    their words; with neither flag the route is what NDCN_RHS_MID_BWD says"""
    from ndcn_amd import hip
    comp = _L().VJP_COMPOSED
    n = 100
    A, _ = op('lattice', n, dev)
    for H in (256, 12):
        X, K, g, W = inputs(n, H, 1, dev)
        for form in FORMS:
            both(A, X, W, K, g, 'H = %d %s' % (H, form), want_route=comp, **{form: True})
    X, K, g, W = inputs(n, 64, 2, dev)
    both(A, X, W, K, g, 'both flags', want_route=comp, no_graph=True, no_control=True)
    gz = torch.where((K.cpu() <= 0).to(dev), torch.zeros_like(g), g)
    pre = both(A, X, W, K, gz, 'no_control premasked', want_route=comp, no_control=True, premasked=True)
    same(pre[0], call(A, X, W, K, g, 1, no_control=True)[0], 'premasked against masked gX')
    both(A, X, W, K, g, 'no_control without the ReLU', want_route=comp, no_control=True, relu=False)
    buf = torch.empty(n * 64 + 1, device=dev)
    g1 = buf[1:].view(n, 64)
    g1.copy_(g)
    assert g1.data_ptr() % 16 == 4 and g1.is_contiguous()
    for form in FORMS:
        a = call(A, X, W, K, g1, 1, want_route=comp, **{form: True})
        b = call(A, X, W, K, g, 0, **{form: True})
        c = call(A, X, W, K, g, 1, **{form: True})
        for name, u, v, w in zip(('gX', 'gW', 'gb'), a, b, c):
            same(u, v, '%s, misaligned g %s' % (form, name))
            same(w, v, '%s, aligned g %s' % (form, name))
    # neither flag: this switch does not touch the full model's reverse
    for mode, want in ((0, comp), (2, _L().VJP_MID)):
        prev = hip.set_rhs_mid_bwd(mode)
        try:
            a = call(A, X, W, K, g, 1, want_route=want)
            b = call(A, X, W, K, g, 0, want_route=want)
        finally:
            hip.set_rhs_mid_bwd(prev)
        for name, u, v in zip(('gX', 'gW', 'gb'), a, b):
            same(u, v, 'neither flag, NDCN_RHS_MID_BWD %d %s' % (mode, name))
