"""The one-launch reverse of the right-hand side for hidden widths 16..128 (csrc/rhs_mid_bwd.hip, NDCN_VJP_MID, ndcn_set_rhs_mid_bwd)
against the composed launches - SpMM into S, linear_gs_kernel, linear_wgrad_kernel, chunk sum, transposed SpMM - BIT FOR BIT: gS, gX, gW
and gb are compared as int32 (torch.equal on the raw words: +0 / -0 and NaN positions count).  Every case calls ndcn_rhs_vjp_f32 with the
switch at 2 and at 0 and asserts the route through ndcn_debug_last_rhs_vjp_path.

Shapes, from the kernel's constants.  A workgroup is one row chunk of the weight gradient (linear_bwd.hip wgrad_chunks) walked in 64-row
tiles from the chunk's first row:
  n = 37      chunks of 16 rows, one partial tile each, the last chunk 5 rows
  n = 100     chunks of 16 rows, the last of 4 rows (half a round of 8)
  n = 4097    65 chunks of 64 rows, the last of ONE row
  n = 20000   250 chunks of 80 rows: a full tile plus a 16-row tile, tiles unaligned to 64 globally
Widths 16 (minimum), 20 (not a multiple of 32: ragged MFMA tiles), 64 (P = 64 exactly, four accumulator pairs), 96 (nine pairs on eight
waves), 100 (P = 128 with padding) and 128 (sixteen pairs, two per wave).  Graphs: an 8-neighbour lattice, and a random graph with empty
rows, rows of 1..3 entries (the gather's remainder loop) and one hub row of up to 300 entries.  A NaN and a -0.0 are planted in g and in K
(a NaN K passes the mask, -0.0 blocks it)."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from _fma_chain import chain

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
WIDTHS = (16, 20, 64, 96, 100, 128)
SIZES = (37, 100, 4097, 20000)


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
def switch(mode):
    from ndcn_amd import hip
    prev = hip.set_rhs_mid_bwd(mode)
    try:
        yield
    finally:
        hip.set_rhs_mid_bwd(prev)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(got, want, what):
    if got is None or want is None:
        assert got is None and want is None, what
        return
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(bits(got), bits(want)):
        bad = (bits(got) != bits(want)).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError('%s: %d of %d words differ; first at %s: got %r (%#010x) want %r (%#010x)' % (
            what, bad.shape[0], got.numel(), i, float(got[i]), int(bits(got)[i]) & 0xffffffff, float(want[i]), int(bits(want)[i]) & 0xffffffff))


def chunks(n):
    """linear_bwd.hip wgrad_chunks + the launcher's rounding: (rows per chunk, chunks used, rows of the last chunk)"""
    c = (n + 15) // 16 if n <= 4096 else (n + 63) // 64
    c = max(1, min(c, 256))
    rpc = -(-(-(-n // c)) // 8) * 8
    used = -(-n // rpc)
    return rpc, used, n - (used - 1) * rpc


def test_the_sizes_reach_the_edges():
    assert chunks(37) == (16, 3, 5)
    assert chunks(100) == (16, 7, 4)
    assert chunks(4097) == (64, 65, 1)
    assert chunks(20000) == (80, 250, 80)


def lattice(n):
    """an 8-neighbour lattice of n nodes, w = ceil(sqrt(n)) per line (the last line may be short), random weights, no self loops"""
    w = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    r, c = i // w, i % w
    rows, cols = [], []
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr == 0 and dc == 0:
                continue
            rr, cc = r + dr, c + dc
            j = rr * w + cc
            ok = (rr >= 0) & (cc >= 0) & (cc < w) & (j < n)
            rows.append(i[ok])
            cols.append(j[ok])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    val = (np.random.RandomState(n).randn(rows.size) / 4).astype(np.float32)
    m = sp.csr_matrix((val, (rows, cols)), shape=(n, n))
    m.sort_indices()
    return m


def ragged(n):
    """row r has (0, 1, 2, 3, 1)[r % 5] entries at distinct columns; row 3 is a hub of min(n, 300) entries"""
    deg = np.array((0, 1, 2, 3, 1))[np.arange(n) % 5]
    deg[3] = min(n, 300)
    rows = np.repeat(np.arange(n), deg)
    j = np.arange(rows.size) - np.repeat(np.cumsum(deg) - deg, deg)
    step = 7 if n % 7 else 11
    assert n % step
    cols = (rows * 3 + j * step) % n                         # step and n coprime: distinct within a row
    val = (np.random.RandomState(n + 1).randn(rows.size) / 4).astype(np.float32)
    m = sp.csr_matrix((val, (rows, cols)), shape=(n, n))
    m.sort_indices()
    assert m.nnz == rows.size
    return m


GRAPHS = {'lattice': lattice, 'ragged': ragged}
_ops = {}


def op(kind, n, dev):
    """(operator, its scipy form), built once per (kind, n)"""
    from ndcn_amd import CsrOperator
    if (kind, n) not in _ops:
        m = GRAPHS[kind](n)
        A = CsrOperator.from_arrays(m.indptr, m.indices, m.data, m.shape, dev)
        A._plans_tried = True
        _ops[(kind, n)] = (A, m)
    return _ops[(kind, n)]


def inputs(n, H, seed, dev):
    gen = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn(n, H, generator=gen, device=dev) * torch.exp2(torch.randint(-6, 7, (n, 1), generator=gen, device=dev).float())
    g = torch.randn(n, H, generator=gen, device=dev) * torch.exp2(torch.randint(-6, 7, (n, 1), generator=gen, device=dev).float())
    g[torch.rand(n, H, generator=gen, device=dev) < 0.1] = 0.0
    K = torch.relu(torch.randn(n, H, generator=gen, device=dev))
    W = (torch.rand(H, H, generator=gen, device=dev) - 0.5) / 4
    r = torch.arange(n, device=dev)
    g[r[0::7], (5 * r[0::7]) % H] = float('nan')
    g[r[1::7], (5 * r[1::7] + 1) % H] = -0.0
    K[r[2::7], (5 * r[2::7] + 2) % H] = float('nan')         # passes the mask
    K[r[3::7], (5 * r[3::7] + 3) % H] = -0.0                 # blocks it
    K[r[0::14], (5 * r[0::14]) % H] = 1.0                    # half of g's NaNs are let through, half are masked (K random there)
    return X, K, g, W


def call(A, X, W, K, g, mode, want_route=None, **kw):
    from ndcn_amd import hip
    with switch(mode):
        out = hip.rhs_vjp(A, X, W, K, g, return_gs=True, **kw)
        torch.cuda.synchronize()
        got = route()
    if want_route is None:
        want_route = _L().VJP_MID if mode else _L().VJP_COMPOSED
    assert got == want_route, (mode, got, want_route)
    return out


def both(A, X, W, K, g, what, **kw):
    """the call with the switch at 2 and at 0: equal words in (gX, gW, gb, gS); accumulating calls start from the same totals"""
    acc = kw.pop('acc', None)
    outs = []
    for mode in (2, 0):
        k2 = dict(kw)
        if acc is not None:
            k2['gW'], k2['gb'] = acc[0].clone(), (acc[1].clone() if kw.get('need_b', True) else None)
        outs.append(call(A, X, W, K, g, mode, **k2))
    for name, a, b in zip(('gX', 'gW', 'gb', 'gS'), outs[0], outs[1]):
        same(a, b, '%s %s' % (what, name))
    return outs[0]


@pytest.mark.parametrize('kind', sorted(GRAPHS))
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('H', WIDTHS)
def test_equal_words(dev, H, n, kind):
    from ndcn_amd import hip
    A, _ = op(kind, n, dev)
    X, K, g, W = inputs(n, H, 100 * H + n % 97, dev)
    S = hip.spmm(A, X)
    gen = torch.Generator(device=dev).manual_seed(5)
    acc = (torch.randn(H, H, generator=gen, device=dev), torch.randn(H, generator=gen, device=dev))
    gX, gW, gb, gS = both(A, X, W, K, g, 'mask, S gathered')
    assert gX is not None and gW is not None and gb is not None and gS is not None
    assert bool(torch.isnan(gS).any()) and bool(torch.isnan(gW).any())      # the planted NaNs arrive
    both(A, X, W, K, g, 'mask, S supplied', S=S)
    gz = torch.where((K.cpu() <= 0).to(dev), torch.zeros_like(g), g)
    pre = both(A, X, W, K, gz, 'premasked', premasked=True)
    for name, a, b in zip(('gX', 'gW', 'gb', 'gS'), pre, (gX, gW, gb, gS)):
        same(a, b, 'premasked against masked %s' % name)     # g (.) [K > 0] formed here or by the caller: the same gZ
    both(A, X, W, K, g, 'no ReLU', relu=False, S=S)
    both(A, X, W, K, g, 'gb null', need_b=False)
    out = both(A, X, W, K, g, 'gX null', need_x=False, S=S)
    assert out[0] is None and out[3] is None
    for scale in (1.0, 2.0):
        both(A, X, W, K, g, 'accumulate, scale %g' % scale, acc=acc, acc_scale=scale)
        both(A, X, W, K, g, 'overwrite, scale %g' % scale, acc_scale=scale, S=S)
    both(A, X, W, K, g, 'accumulate, gb null', acc=acc, acc_scale=2.0, need_b=False, premasked=True)


def test_against_fp64_and_the_fma_chain(dev):
    """n = 20000, H = 64 on the lattice: gS and gW / gb against fp64 products of the same fp32 inputs, to the fp32-route bounds of
    tests/test_gpu_linear_routes.py - per element (Ho + 2) u sum |gZ W| for gS, 1.01 u (rows_per_chunk + chunks) sum |gZ S| for gW,
    1.01 u (rows_per_chunk + chunks + 1) sum |gZ| for gb, u = 2^-24; S and gX against the sequential fma chain, bit for bit."""
    n, H = 20000, 64
    A, m = op('lattice', n, dev)
    gen = torch.Generator(device=dev).manual_seed(9)
    X = torch.randn(n, H, generator=gen, device=dev)
    g = torch.randn(n, H, generator=gen, device=dev)
    K = torch.relu(torch.randn(n, H, generator=gen, device=dev))
    K[::5, 3] = -0.0
    W = (torch.rand(H, H, generator=gen, device=dev) - 0.5) / 4
    gX, gW, gb, gS = call(A, X, W, K, g, 2, acc_scale=2.0)
    gz = torch.where((K.cpu() <= 0).to(dev), torch.zeros_like(g), g).double()
    Wd = W.double()

    def within(got, ref, bound, what):
        err = (got.double() - ref).abs()
        bad = ~(err <= bound)
        print('%s: largest error / bound = %.3f' % (what, float((err / bound.clamp_min(1e-300)).max())))
        assert not bool(bad.any()), '%s: %d elements out of bound' % (what, int(bad.sum()))

    within(gS, gz @ Wd, (H + 2) * U * (gz.abs() @ Wd.abs()), 'gS')
    S = torch.from_numpy(chain(m.indptr, m.indices, m.data, X.cpu().numpy())).to(dev)
    rpc, used, _ = chunks(n)
    Sd = S.double()
    # (acc_scale = 2 is exact in fp32: the bounds scale with it)
    within(gW, 2.0 * (gz.t() @ Sd), 2.0 * 1.01 * U * (rpc + used) * (gz.abs().t() @ Sd.abs()), 'gW')
    within(gb, 2.0 * gz.sum(0), 2.0 * 1.01 * U * (rpc + used + 1) * gz.abs().sum(0), 'gb')
    mt = A.transpose().to_scipy().tocsr()
    want = torch.from_numpy(chain(mt.indptr, mt.indices, mt.data, gS.cpu().numpy(), alpha=2.0)).to(dev)
    same(gX, want, 'gX against the fma chain of A^T over gS')
    # the gathered S is the chain too: the weight gradient from the chain's S, supplied, has the same words
    out = call(A, X, W, K, g, 2, acc_scale=2.0, S=S)
    same(out[1], gW, 'gW, S gathered against the chain supplied')


def test_two_calls_give_the_same_words(dev):
    n, H = 4097, 96
    A, _ = op('ragged', n, dev)
    X, K, g, W = inputs(n, H, 3, dev)
    a = call(A, X, W, K, g, 2)
    b = call(A, X, W, K, g, 2)
    for name, u, v in zip(('gX', 'gW', 'gb', 'gS'), a, b):
        same(u, v, name)


def test_declined_shapes_run_composed(dev):
    """switch at 2: H = 256, NO_CONTROL and a g that is 4 bytes off 16-byte alignment take the composed launches and give their words"""
    from ndcn_amd import hip
    comp = _L().VJP_COMPOSED
    n = 100
    A, _ = op('lattice', n, dev)
    X, K, g, W = inputs(n, 256, 1, dev)
    a = call(A, X, W, K, g, 2, want_route=comp)
    b = call(A, X, W, K, g, 0)
    for name, u, v in zip(('gX', 'gW', 'gb'), a, b):
        same(u, v, 'H = 256 %s' % name)
    X, K, g, W = inputs(n, 64, 2, dev)
    a = call(A, X, W, K, g, 2, want_route=comp, no_control=True)
    b = call(A, X, W, K, g, 0, no_control=True)
    assert a[1] is None and a[2] is None
    same(a[0], b[0], 'NO_CONTROL gX')
    same(a[0], hip.spmm(A.transpose(), hip.relu_bwd(g, K)), 'NO_CONTROL gX against its two launches')
    buf = torch.empty(n * 64 + 1, device=dev)
    g1 = buf[1:].view(n, 64)
    g1.copy_(g)
    assert g1.data_ptr() % 16 == 4 and g1.is_contiguous()
    a = call(A, X, W, K, g1, 2, want_route=comp)
    b = call(A, X, W, K, g, 0)
    c = call(A, X, W, K, g, 2)
    for name, u, v, w in zip(('gX', 'gW', 'gb', 'gS'), a, b, c):
        same(u, v, 'misaligned g %s' % name)
        same(w, v, 'aligned g %s' % name)
