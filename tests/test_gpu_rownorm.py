"""The three kernels of csrc/rownorm.hip through hip.row_l1_normalize / hip.row_l1_normalize_bwd against the float64 restatement
tests/_rownorm.py, element by element inside its float32 bounds (derived there from the arithmetic, not from a run).

Which kernel a case reaches, from the dispatcher row_l1_normalize_f32: rownorm_vec_kernel needs H % 4 == 0, H <= 1024 and both panels
16-byte aligned - VEC_H on fresh allocations, one to four float4 register slots per lane in use (H <= 256, 260..512, 516..768,
772..1024); everything else takes rownorm_any_kernel: ANY_H (odd H, H % 4 != 0, H > 1024) and every VEC_H again on a contiguous view
that starts one float into its buffer (input, output or both misaligned).  rownorm_bwd_kernel has one form.  The grid is capped at
16 blocks of four rows per compute unit: row counts past 4 * 16 * CUs are reached only by the grid-stride loop.

Range: every finite row's L1 norm is at most 1e15.  Above about 1.8e19 den * den overflows in float32 in the reverse, in the
reference as well; that range is outside this test."""
import ctypes

import numpy as np
import pytest
import torch

import _rownorm

pytestmark = pytest.mark.gpu
VEC_H = (4, 32, 252, 256, 260, 512, 1020, 1024)
ANY_H = (1, 2, 3, 5, 63, 65, 66, 1023, 1025, 1028, 2050)
ROWS = (1, 3, 4, 5, 9, 29)            # 29: every special row at once, eight blocks
SENTINEL = 7.0
PAD = 64                              # floats in front of and behind a view: 256 bytes, so PAD keeps and PAD + 1 breaks the alignment


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def D(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def words(t):
    return t.contiguous().view(torch.int32)


def inputs(n_rows, H, seed=None):
    seed = (7 * n_rows + H) if seed is None else seed
    X, index = _rownorm.panel(n_rows, H, seed)
    G = np.random.RandomState(1000 + seed).normal(0, 1, X.shape).astype(np.float32)
    return X, G, index


def view_in(buf, n_rows, H, off):
    """a contiguous n_rows x H view that starts `off` floats into buf"""
    v = buf[off:off + n_rows * H].view(n_rows, H)
    assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (off % 4 == 0)
    return v


def shifted(t, off=PAD + 1):
    """t's data in a view that starts off floats into a sentinel buffer: (view, buffer)"""
    buf = torch.full((t.numel() + off + PAD,), SENTINEL, device=t.device)
    v = view_in(buf, t.shape[0], t.shape[1], off)
    v.copy_(t)
    return v, buf


def sentinels_intact(buf, n, off):
    return bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())


def assert_forward(got, X, index, what):
    got = got.cpu().numpy().astype(np.float64)
    want, bound = _rownorm.forward(X), _rownorm.forward_bound(X)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, 'NaN positions', index)
    ok = ~np.isnan(want)
    over = np.abs(got - want)[ok] > bound[ok]
    assert not over.any(), (what, float((np.abs(got - want)[ok] / bound[ok]).max()), index)
    for name in ('pos_inf', 'neg_inf'):
        if name in index:                       # the finite entries of an infinite row: exact zeros, as the reference produces
            r, j = index[name]
            assert not np.delete(got[r], j).any(), (what, name)


def assert_reverse(got, G, X, index, what):
    got = got.cpu().numpy().astype(np.float64)
    want, bound = _rownorm.vjp(G, X), _rownorm.vjp_bound(G, X)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, 'NaN positions', index)
    ok = ~np.isnan(want)
    over = np.abs(got - want)[ok] > bound[ok]
    assert not over.any(), (what, float((np.abs(got - want)[ok] / bound[ok]).max()), index)
    Gd = G.astype(np.float64)
    if 'one_zero' in index and X[index['one_zero']] == 0:            # (H = 1 has no room for the zero)
        r, j = index['one_zero']
        den = np.abs(X[r].astype(np.float64)).sum()
        assert abs(got[r, j] - Gd[r, j] / den) <= bound[r, j], (what, 'no second term at a zero entry')
    for name in ('zeros', 'signed_zeros', 'clamped', 'denormal'):
        if name in index:
            r = index[name][0]
            assert (np.abs(got[r] - Gd[r] / _rownorm.EPS) <= bound[r]).all(), (what, name, 'g / eps in a clamped row')


def cus():
    from ndcn_amd.ops import device_info
    n = device_info()['compute_units']
    assert n > 0
    return n


def row_counts(H):
    if H in (4, 5):
        return ROWS + (4 * 16 * cus() + 1, 2 * 4 * 16 * cus() + 3)
    return ROWS


@pytest.mark.parametrize('H', VEC_H + ANY_H)
def test_forward_and_reverse_against_float64(dev, H):
    from ndcn_amd import hip
    for n_rows in row_counts(H):
        X, G, index = inputs(n_rows, H)
        Xd, Gd = D(X, dev), D(G, dev)
        assert Xd.data_ptr() % 16 == 0                              # fresh allocations: VEC_H takes the vector kernel
        Y = hip.row_l1_normalize(Xd)
        assert_forward(Y, X, index, (n_rows, H))
        assert torch.equal(words(Y), words(hip.row_l1_normalize(Xd)))                       # two runs, the same words
        GX = hip.row_l1_normalize_bwd(Gd, Xd)
        assert_reverse(GX, G, X, index, (n_rows, H))
        assert torch.equal(words(GX), words(hip.row_l1_normalize_bwd(Gd, Xd)))
        assert torch.equal(words(Xd), words(D(X, dev))) and torch.equal(words(Gd), words(D(G, dev)))     # inputs untouched


@pytest.mark.parametrize('H', VEC_H)
def test_misaligned_panels_take_the_two_pass_kernel(dev, H):
    from ndcn_amd import hip
    for n_rows in row_counts(H):
        X, _, index = inputs(n_rows, H)
        Xd = D(X, dev)
        assert_forward(hip.row_l1_normalize(Xd), X, index, (n_rows, H, 'aligned'))
        for shift_in, shift_out in ((True, False), (False, True), (True, True)):
            Xv, xbuf = shifted(Xd, PAD + 1) if shift_in else (Xd, None)
            obuf = torch.full((n_rows * H + 2 * PAD + 1,), SENTINEL, device=dev)
            off = PAD + 1 if shift_out else PAD
            out = view_in(obuf, n_rows, H, off)
            got = hip.row_l1_normalize(Xv, out=out)
            assert got.data_ptr() == out.data_ptr()
            assert_forward(out, X, index, (n_rows, H, shift_in, shift_out))
            assert sentinels_intact(obuf, n_rows * H, off)
            assert xbuf is None or (sentinels_intact(xbuf, n_rows * H, PAD + 1) and torch.equal(words(Xv), words(Xd)))


@pytest.mark.parametrize('H', VEC_H + ANY_H)
def test_nothing_is_written_outside_the_panel(dev, H):
    """all three kernels write into a view inside a sentinel buffer (the vector kernel: an aligned view)"""
    from ndcn_amd import _lib, hip
    lib = _lib.load()
    for n_rows in row_counts(H):
        X, G, index = inputs(n_rows, H)
        Xd, Gd = D(X, dev), D(G, dev)
        n = n_rows * H
        obuf = torch.full((n + 2 * PAD,), SENTINEL, device=dev)
        out = view_in(obuf, n_rows, H, PAD)
        hip.row_l1_normalize(Xd, out=out)
        assert sentinels_intact(obuf, n, PAD) and torch.equal(words(out), words(hip.row_l1_normalize(Xd)))
        for off in (PAD, PAD + 1):
            gbuf = torch.full((n + 2 * PAD + 1,), SENTINEL, device=dev)
            gx = view_in(gbuf, n_rows, H, off)
            assert lib.ndcn_row_l1_normalize_bwd_f32(_lib.ptr(Gd), _lib.ptr(Xd), _lib.ptr(gx), n_rows, H, _lib.stream_ptr()) == _lib.OK
            assert sentinels_intact(gbuf, n, off) and torch.equal(words(gx), words(hip.row_l1_normalize_bwd(Gd, Xd)))


@pytest.mark.parametrize('H', (4, 5, 260, 1023, 1024, 2050))
def test_in_place_equals_out_of_place(dev, H):
    """ResBlock.forward normalises f into itself"""
    from ndcn_amd import hip
    for n_rows in row_counts(H):
        X, _, _ = inputs(n_rows, H)
        Xd = D(X, dev)
        want = hip.row_l1_normalize(Xd)
        c = Xd.clone()
        got = hip.row_l1_normalize(c, out=c)
        assert got.data_ptr() == c.data_ptr() and torch.equal(words(c), words(want)), (n_rows, H)


@pytest.mark.parametrize('H', (4, 5, 260, 1023, 1024, 2050))
def test_rows_do_not_leak(dev, H):
    """a NaN row changes no word of any other row, forward or reverse"""
    from ndcn_amd import hip
    for n_rows in row_counts(H):
        if n_rows == 1:
            continue
        X, G, _ = inputs(n_rows, H)
        Xd, Gd = D(X, dev), D(G, dev)
        Y, GX = hip.row_l1_normalize(Xd), hip.row_l1_normalize_bwd(Gd, Xd)
        for r in sorted({0, n_rows // 2, n_rows - 1}):
            X2, G2 = Xd.clone(), Gd.clone()
            X2[r] = float('nan')
            G2[r] = float('nan')
            others = torch.arange(n_rows, device=dev) != r
            Y2 = hip.row_l1_normalize(X2)
            assert bool(torch.isnan(Y2[r]).all()) and torch.equal(words(Y2[others]), words(Y[others])), (n_rows, H, r)
            for g_, x_ in ((Gd, X2), (G2, Xd), (G2, X2)):
                GX2 = hip.row_l1_normalize_bwd(g_, x_)
                assert bool(torch.isnan(GX2[r]).all()) and torch.equal(words(GX2[others]), words(GX[others])), (n_rows, H, r)


def test_c_abi_sizes(dev):
    from ndcn_amd import _lib
    lib = _lib.load()
    P, st = _lib.ptr, _lib.stream_ptr
    x, g = torch.full((12,), SENTINEL, device=dev), torch.full((12,), SENTINEL, device=dev)
    y = torch.full((12,), SENTINEL, device=dev)
    for n_rows, H in ((-1, 4), (3, -4), (-1, -1)):
        assert lib.ndcn_row_l1_normalize_f32(P(x), P(y), n_rows, H, st()) == _lib.EINVAL
        assert lib.ndcn_row_l1_normalize_bwd_f32(P(g), P(x), P(y), n_rows, H, st()) == _lib.EINVAL
    assert lib.ndcn_row_l1_normalize_f32(None, P(y), 3, 4, st()) == _lib.EINVAL
    assert lib.ndcn_row_l1_normalize_bwd_f32(P(g), P(x), None, 3, 4, st()) == _lib.EINVAL
    null = ctypes.c_void_p(0)
    for n_rows, H in ((0, 4), (3, 0), (0, 0)):
        assert lib.ndcn_row_l1_normalize_f32(null, null, n_rows, H, st()) == _lib.OK
        assert lib.ndcn_row_l1_normalize_bwd_f32(null, null, null, n_rows, H, st()) == _lib.OK
        assert lib.ndcn_row_l1_normalize_f32(P(x), P(y), n_rows, H, st()) == _lib.OK
        assert lib.ndcn_row_l1_normalize_bwd_f32(P(g), P(x), P(y), n_rows, H, st()) == _lib.OK
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (x, g, y))


@pytest.mark.parametrize('H', (32, 33))
def test_autograd_runs_the_reverse_kernel(dev, H):
    """row_normalization on a tensor that requires grad: .backward() gives the words of hip.row_l1_normalize_bwd"""
    from ndcn_amd import hip
    from ndcn_amd.ode_gcn import RowNorm, row_normalization
    X, G, index = inputs(29, H)
    Xd, Gd = D(X, dev), D(G, dev)
    for f in (row_normalization, RowNorm()):
        x = Xd.clone().requires_grad_()
        y = f(x)
        assert y.requires_grad and torch.equal(words(y.detach()), words(hip.row_l1_normalize(Xd)))
        y.backward(Gd)
        assert torch.equal(words(x.grad), words(hip.row_l1_normalize_bwd(Gd, Xd)))
        assert_reverse(x.grad, G, X, index, H)
    with torch.no_grad():
        assert not row_normalization(Xd).requires_grad
