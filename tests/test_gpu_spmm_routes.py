"""Every SpMM route (csrc/spmm.hip, spmm_rec.hip, spmm_sweep.hip and the long-row plan in front of them) against the sequential fp32
fma chain of tests/_fma_chain.py, bit for bit, each route asserted through ndcn_debug_last_spmm_path.

DESIGN.md sections 2 and 4: SpMM is one fma per stored entry, in stored order, from +0 - the bits of a sequential loop; a hub row of
the long-row plan is the chain over its <= 256-entry segment chains.  NaN results compare as NaN (IEEE 754 leaves a NaN's sign and
payload to the implementation); every other element compares by its bits.

As a check on the reference itself, every element whose fp64 value is finite also satisfies
    |Y - exact64| <= 1.01 (|alpha| ((d + 1) u sum|a x| + d 2^-150) + 2^-150),   u = 2^-24,
d = the row length (hub rows: d + their segments): each of the d fmas errs by at most u |partial sum| + 2^-150 (half a subnormal
ulp), scaled by |alpha|; the product with alpha errs by at most u |alpha acc| + 2^-150, NOT scaled by |alpha|.  For |alpha| >= 1 this
is at most 1.01 |alpha| (d + 1) (u sum|a x| + 2^-150); for |alpha| < 1 the alpha rounding's floor must stay unscaled (alpha = 2^-20
on a subnormal sum rounds alpha * acc in the subnormal range).
Large panels compare sampled rows: the first and last row of every XCD chunk and of the panel, plus 4096 seeded rows."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from _fma_chain import U, chain, chain_hub, row_terms
from _oracle_ops import OracleOps
from _rk_epilogue import error_terms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from ndcn_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _L():
    from ndcn_amd import _lib
    return _lib


def _path():
    return int(_L().load().ndcn_debug_last_spmm_path())


def _lpr(slots):
    return 64 if slots > 32 else 32 if slots > 16 else 16 if slots > 8 else 8 if slots > 4 else 4 if slots > 2 else 2 if slots > 1 else 1


def _rpb(lpr, n_rows, nnz):
    """launch_spmm's rows per workgroup"""
    groups = 256 // lpr
    rpb = min(max(groups * 8, 64), 256)
    avg = nnz / n_rows if n_rows else 0.0
    while rpb > groups and rpb > 16 and avg * rpb > 2048:
        rpb //= 2
    return rpb


def csr_bits(vw, H, n_rows, nnz, halo):
    L = _L()
    lpr = _lpr(H // vw)
    return (L.SPMM_CSR | (L.SPMM_VEC if vw == 4 else 0) | (L.SPMM_HALO if halo else 0) | (lpr << L.SPMM_LANES_SHIFT) |
            (_rpb(lpr, n_rows, nnz) << L.SPMM_RPB_SHIFT))


def wide_bits(nv, halo, mode=0):
    L = _L()
    return L.SPMM_WIDE | L.SPMM_VEC | (L.SPMM_HALO if halo else 0) | (nv << L.SPMM_LANES_SHIFT) | (mode << L.SPMM_MODE_SHIFT)


REC_CODE = {(8, 32, 1): 1, (16, 40, 2): 2, (8, 48, 2): 3}


def rec_bits(shape, halo, mode=0):
    L = _L()
    return (L.SPMM_REC | L.SPMM_VEC | (L.SPMM_HALO if halo else 0) | (REC_CODE[tuple(shape)] << L.SPMM_REC_SHIFT) |
            (mode << L.SPMM_MODE_SHIFT))


def _rand(n_rows, n_cols, avg, seed, long_rows=(), lengths=None, empty=True, scale=1.0):
    """rows of poisson(avg) (or the given, cycled) lengths; each row's columns distinct and ascending, drawn in one vectorised pass"""
    rng = np.random.RandomState(seed)
    deg = rng.poisson(avg, size=n_rows) if lengths is None else np.resize(np.asarray(lengths, np.int64), n_rows)
    if empty and lengths is None:
        deg[rng.randint(0, n_rows, size=max(1, n_rows // 40))] = 0
    for r, d in long_rows:
        deg[r] = d
    deg = np.minimum(deg, n_cols).astype(np.int64)
    indptr = np.r_[0, np.cumsum(deg)].astype(np.int64)
    nnz = int(indptr[-1])
    rowid = np.repeat(np.arange(n_rows), deg)
    G = np.maximum(1, (n_cols - 1) // np.maximum(deg, 1))                     # gaps in [1, G]: the row spans <= n_cols columns
    gaps = 1 + (rng.random_sample(nnz) * G[rowid]).astype(np.int64)
    cs = np.r_[0, np.cumsum(gaps)]
    pos = cs[1:] - cs[indptr[:-1]][rowid] - 1
    span = cs[indptr[1:]] - cs[indptr[:-1]]
    base = (rng.random_sample(n_rows) * (n_cols - span + 1)).astype(np.int64)
    indices = pos + base[rowid]
    data = (rng.randn(nnz) * scale).astype(np.float32)
    return sp.csr_matrix((data, indices, indptr), shape=(n_rows, n_cols))


def _from_rows(rows, n_cols):
    """CSR from per-row (columns, values) lists, stored zeros kept"""
    deg = [len(c) for c, _ in rows]
    indptr = np.r_[0, np.cumsum(deg)].astype(np.int64)
    ind = np.concatenate([np.asarray(c, np.int64) for c, _ in rows]) if indptr[-1] else np.zeros(0, np.int64)
    val = np.concatenate([np.asarray(v, np.float32) for _, v in rows]) if indptr[-1] else np.zeros(0, np.float32)
    return sp.csr_matrix((val, ind, indptr), shape=(len(rows), n_cols))


def _op(m, dev, plans=False):
    from ndcn_amd import CsrOperator
    m = sp.csr_matrix(m)
    m.sort_indices()
    A = CsrOperator.from_arrays(m.indptr, m.indices, m.data, m.shape, dev)
    if not plans:
        A._plans_tried = True                    # no plans: the row kernels alone
    return A


def sample_rows(n, seed=0):
    """first / last row of every XCD chunk (chunk = ceil(n / 8)) and of the panel, plus 4096 seeded rows"""
    if n <= 6000:
        return np.arange(n)
    ch = -(-n // 8)
    edge = np.r_[np.arange(0, n, ch), np.minimum(np.arange(ch - 1, n + ch - 1, ch), n - 1), 0, n - 1]
    rng = np.random.RandomState(seed)
    return np.unique(np.r_[edge, rng.randint(0, n, 4096)])


def check(A, X, Y, X_halo=None, alpha=1.0, relu=False, rows=None, hub_thr=None, what=''):
    """Y (device, the kernel's output for the operator A = CsrOperator) against the chain on the rows `rows`; bits and the fp64 bound"""
    rp = A.rowptr.cpu().numpy().astype(np.int64)
    ci = A.colidx.cpu().numpy().astype(np.int64)
    va = A.val.cpu().numpy()
    n = A.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    Yr = Y.view(n, -1)[torch.as_tensor(rows, device=Y.device)].cpu().numpy() if rows.size else np.zeros((0, Y.shape[-1]), np.float32)
    H = Yr.shape[1]
    # the rows' operator with their columns compacted; the panel rows they read fetched from the device
    deg = rp[rows + 1] - rp[rows]
    sub_ptr = np.r_[0, np.cumsum(deg)].astype(np.int64)
    take = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows]) if sub_ptr[-1] else np.zeros(0, np.int64)
    cols, inv = np.unique(ci[take], return_inverse=True)
    X2 = X.view(X.shape[0], -1)
    n_own = X2.shape[0]
    ct = torch.as_tensor(cols, device=X.device)
    own = ct < n_own
    Xs = torch.empty((cols.size, H), dtype=torch.float32, device=X.device)
    Xs[own] = X2[ct[own]]
    if X_halo is not None:
        Xs[~own] = X_halo.view(X_halo.shape[0], -1)[ct[~own] - n_own]
    Xs = Xs.cpu().numpy()
    sub_ci, sub_va = inv.astype(np.int64), va[take]
    if hub_thr is not None:
        ref = chain_hub(sub_ptr, sub_ci, sub_va, Xs, hub_thr, alpha=alpha, relu=relu)
    else:
        ref = chain(sub_ptr, sub_ci, sub_va, Xs, alpha=alpha, relu=relu)
    gb, rb = Yr.view(np.int32), ref.view(np.int32)
    nan_both = np.isnan(Yr) & np.isnan(ref)
    bad = (gb != rb) & ~nan_both
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError('%s: %d of %d elements differ from the fma chain; first at row %d col %d: got %r (0x%08x) want %r (0x%08x)'
                             % (what, int(bad.sum()), bad.size, rows[i], j, float(Yr[i, j]), int(gb[i, j]) & 0xffffffff, float(ref[i, j]),
                                int(rb[i, j]) & 0xffffffff))
    # the reference against fp64
    S = sp.csr_matrix((sub_va.astype(np.float64), sub_ci, sub_ptr), shape=(rows.size, max(cols.size, 1)))
    Xd = Xs.astype(np.float64) if cols.size else np.zeros((1, H))
    with np.errstate(invalid='ignore', over='ignore'):
        e64 = float(alpha) * (S @ Xd)
        if relu:
            e64 = np.where(e64 < 0, 0.0, e64)
        mag = abs(S) @ np.abs(Xd)
        d = row_terms(sub_ptr, hub_thr)[:, None]
        bound = 1.01 * (abs(float(alpha)) * ((d + 1) * U * mag + d * 2.0 ** -150) + 2.0 ** -150)
        fin = np.isfinite(e64)
        err = np.abs(Yr.astype(np.float64) - e64)
    over = fin & ~(err <= bound)
    assert not over.any(), '%s: %d elements outside the fp64 bound (worst err %r)' % (what, int(over.sum()), float(err[over].max()))


def run(A, X, want_path, X_halo=None, alpha=1.0, relu=False, rows=None, hub_thr=None, what=''):
    from ndcn_amd import hip
    Y = hip.spmm(A, X, X_halo=X_halo, alpha=alpha, relu=relu)
    torch.cuda.synchronize()
    p = _path()
    assert p == want_path, '%s: path %#x, want %#x' % (what, p, want_path)
    check(A, X, Y, X_halo, alpha, relu, rows, hub_thr, what)
    return Y


def _X(n, H, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(n, H, generator=g, device=dev)


def _misaligned(n, H, dev, seed):
    buf = _X(n * H + 1, 1, dev, seed).view(-1)
    X = buf[1:].view(n, H)
    assert X.is_contiguous() and X.data_ptr() % 16 == 4
    return X


# ------------------------------------------------------------------------------------------------------------------- CSR
@pytest.mark.parametrize('halo', [False, True])
@pytest.mark.parametrize('H', [4, 8, 12, 20, 36, 68, 132, 260, 516, 1028, 1280])
def test_csr_vw4(dev, H, halo):
    n = 2000 if H < 256 else 500
    m = _rand(n, 1500, 9, seed=H)
    A = _op(m, dev)
    X = _X(1500, H, dev, H)
    Xo, Xh = (X[:1100].contiguous(), X[1100:].contiguous()) if halo else (X, None)
    run(A, Xo, csr_bits(4, H, n, m.nnz, halo), X_halo=Xh, what='VW4 H=%d halo=%s' % (H, halo))
    run(A, Xo, csr_bits(4, H, n, m.nnz, halo), X_halo=Xh, alpha=-2.5, relu=True, what='VW4 H=%d halo=%s alpha relu' % (H, halo))


@pytest.mark.parametrize('halo', [False, True])
@pytest.mark.parametrize('H', [1, 2, 3, 5, 9, 17, 33, 65, 129, 257])
def test_csr_vw1(dev, H, halo):
    n = 2000 if H < 256 else 500
    m = _rand(n, 1500, 9, seed=100 + H)
    A = _op(m, dev)
    X = _X(1500, H, dev, H)
    Xo, Xh = (X[:1100].contiguous(), X[1100:].contiguous()) if halo else (X, None)
    run(A, Xo, csr_bits(1, H, n, m.nnz, halo), X_halo=Xh, what='VW1 H=%d halo=%s' % (H, halo))
    run(A, Xo, csr_bits(1, H, n, m.nnz, halo), X_halo=Xh, alpha=2.0 ** -20, relu=True, what='VW1 H=%d halo=%s alpha' % (H, halo))


@pytest.mark.parametrize('halo', [False, True])
@pytest.mark.parametrize('H', [4, 64, 256, 512, 1024])
def test_csr_misaligned_views(dev, H, halo):
    """a panel view offset by one float (contiguous, not 16-byte aligned) leaves every vector route - sweep, hub, rec, wide - for
    the scalar kernel; the operator has its plans (ensure_plans) at H = 256"""
    n = 1200 if H <= 256 else 400
    m = _rand(n, 1500, 9, seed=200 + H)
    A = _op(m, dev, plans=True)
    X = _misaligned(1500, H, dev, H)
    Xo, Xh = (X[:1100], _misaligned(400, H, dev, H + 1)) if halo else (X, None)
    run(A, Xo, csr_bits(1, H, n, m.nnz, halo), X_halo=Xh, what='misaligned H=%d halo=%s' % (H, halo))


# ------------------------------------------------------------------------------------------------------------------- staging
@pytest.mark.parametrize('H,avg,want', [(64, 5, 128), (64, 20, 64), (64, 40, 32), (260, 5, 64), (260, 60, 32), (260, 200, 16)])
def test_csr_rows_per_block_halving(dev, H, avg, want):
    n = 1500
    m = _rand(n, 4000, avg, seed=avg, empty=False)
    assert _rpb(_lpr(H // 4), n, m.nnz) == want
    Y = run(_op(m, dev), _X(4000, H, dev, 3), csr_bits(4, H, n, m.nnz, False), what='rpb H=%d avg=%d' % (H, avg))
    assert (_path() >> _L().SPMM_RPB_SHIFT) == want and Y.shape == (n, H)


@pytest.mark.parametrize('H', [20, 3])
def test_csr_rows_past_the_lds_stage(dev, H):
    """blocks whose late rows fall past the 2048-entry stage (long rows early in a block) and rows longer than the stage"""
    n = 3000
    long_rows = [(r, 700) for r in range(3, n, 517)] + [(1000, 2500), (2999, 4000), (0, 2049)]
    m = _rand(n, 5000, 3, seed=7, long_rows=long_rows)
    vw = 4 if H % 4 == 0 else 1
    want = csr_bits(vw, H, n, m.nnz, False)
    rpb = _rpb(_lpr(H // vw), n, m.nnz)
    rp = m.indptr
    late = [b for b in range(0, n, rpb) if rp[min(b + rpb, n)] - rp[b] > 2048]
    assert late, 'no block overflows the stage'
    run(_op(m, dev), _X(5000, H, dev, 9), want, what='stage H=%d' % H)


@pytest.mark.parametrize('k', range(8))
def test_csr_xcd_remap_every_block_count(dev, k):
    """nblk % 8 = 0..7 with a ragged last block"""
    H = 20
    rpb = _rpb(_lpr(5), 10 ** 6, 3 * 10 ** 6)
    n = rpb * (8 + (k if k else 8)) - 37
    m = _rand(n, 700, 3, seed=50 + k)
    assert _rpb(_lpr(5), n, m.nnz) == rpb
    nblk = -(-n // rpb)
    assert nblk % 8 == k and n % rpb
    run(_op(m, dev), _X(700, H, dev, k), csr_bits(4, H, n, m.nnz, False), what='nblk=%d' % nblk)


# ------------------------------------------------------------------------------------------------------------------- WIDE
WIDE_LENGTHS = list(range(18)) + [63, 64, 65, 127, 128, 129, 300]


@pytest.mark.parametrize('halo', [False, True])
@pytest.mark.parametrize('nv', [1, 2, 3, 4])
def test_wide(dev, nv, halo):
    """row lengths 0..17 (every 8 / 4 / 2 / 1 batch tail), 63..65, 127..129, 300; n_rows % 8 != 0; fewer rows than waves"""
    H = 256 * nv
    for n, seed in ((1001, 1), (37, 2)):
        m = _rand(n, 1200, 0, seed=seed + 10 * nv, lengths=WIDE_LENGTHS)
        A = _op(m, dev)
        X = _X(1200, H, dev, seed)
        Xo, Xh = (X[:900].contiguous(), X[900:].contiguous()) if halo else (X, None)
        run(A, Xo, wide_bits(nv, halo), X_halo=Xh, what='wide NV=%d n=%d' % (nv, n))
        run(A, Xo, wide_bits(nv, halo), X_halo=Xh, alpha=-2.5, relu=True, what='wide NV=%d n=%d alpha relu' % (nv, n))


def test_wide_row_order(dev):
    """a random set_row_order permutation: the walk order changes, the bits do not"""
    from ndcn_amd import hip
    m = _rand(2001, 2001, 0, seed=5, lengths=WIDE_LENGTHS)
    X = _X(2001, 256, dev, 5)
    A = _op(m, dev)
    natural = run(A, X, wide_bits(1, False), what='natural order')
    B = _op(m, dev)
    B.set_row_order(np.random.RandomState(0).permutation(2001))
    B._plans_tried = True
    Y = hip.spmm(B, X)
    assert _path() == wide_bits(1, False)
    assert torch.equal(Y.view(torch.int32), natural.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------- REC
def _lattice(side):
    from ndcn_amd import graphs
    m = graphs.normalized_laplacian(graphs.grid_8_neighbor(side)).tocsr()
    m.sort_indices()
    return m


def _rec_op(m, dev, shape, hinted):
    from ndcn_amd import CsrOperator
    A = _op(m, dev)
    if hinted:
        A.group_order = torch.as_tensor(A.detect_stencil_order(), dtype=torch.int32).to(dev)
    A.build_rec_plan(*shape)
    assert A.view().rec_groups > 0
    return A


@pytest.mark.parametrize('shape', [(8, 32, 1), (16, 40, 2), (8, 48, 2)])
def test_rec(dev, shape):
    """lattice (hinted and row order) and a mixed operator whose flagged groups are gathered inside the kernel; 45 x 45 leaves a
    ragged last group; a halo panel; alpha / relu"""
    side = 45
    n = side * side
    grid = _lattice(side)
    rnd = _rand(n, n, 9, seed=5, long_rows=[(1500, 300)])
    mixed = sp.vstack([grid[:1000], rnd[1000:]]).tocsr()
    X = _X(n, 256, dev, 1)
    for m, hinted in ((grid, True), (grid, False), (mixed, False)):
        A = _rec_op(m, dev, shape, hinted)
        what = 'rec %s hinted=%s mixed=%s' % (shape, hinted, m is mixed)
        run(A, X, rec_bits(shape, False), what=what)
        run(A, X, rec_bits(shape, False), alpha=-2.5, relu=True, what=what + ' alpha relu')
        run(A, X[:1200].contiguous(), rec_bits(shape, True), X_halo=X[1200:].contiguous(), what=what + ' halo')


# ------------------------------------------------------------------------------------------------------------------- SWEEP
@pytest.mark.parametrize('name', ['one_pass', 'two_passes'])
def test_sweep(dev, name):
    from ndcn_amd import CsrOperator
    m = _rand(3000, 3000, 40, seed=1) if name == 'one_pass' else _rand(100352 + 777, 2100, 3, seed=4)
    A = CsrOperator.from_arrays(m.indptr, m.indices, m.data, m.shape, dev)
    A.build_plans(256, flags=_L().PLAN_FORCE_SWEEP | _L().PLAN_NO_REC | _L().PLAN_NO_HUB)
    A._plans_tried = True
    assert A.sweep is not None and A.sweep['passes'] == (1 if name == 'one_pass' else 2)
    run(A, _X(m.shape[1], 256, dev, 2), _L().SPMM_SWEEP | _L().SPMM_VEC, rows=sample_rows(m.shape[0]), what='sweep ' + name)


# ------------------------------------------------------------------------------------------------------------------- HUB
def test_hub(dev):
    """a power-law operator with the long-row plan (ensure_plans(256)): segments -> combine -> the light operator with alpha / relu;
    with a halo panel the plan is bypassed and the plain chain holds"""
    from ndcn_amd import graphs
    n = 4000
    m = graphs.normalized_laplacian(graphs.make_graph('power_law', n, seed=0)).tocsr()
    m.sort_indices()
    A = _op(m, dev, plans=True)
    A.ensure_plans(256)
    assert A.hub is not None and A.hub['n'] > 0 and A.sweep is None
    thr = A.hub['threshold']
    X = _X(n, 256, dev, 4)
    L = _L()
    want = L.SPMM_HUB | wide_bits(1, True)
    run(A, X, want, hub_thr=thr, what='hub')
    run(A, X, want, hub_thr=thr, alpha=-2.5, relu=True, what='hub alpha relu')
    from ndcn_amd import hip
    Y = hip.spmm(A, X[:3000].contiguous(), X_halo=X[3000:].contiguous())
    p = _path()
    assert p in (wide_bits(1, True), rec_bits((8, 32, 1), True), rec_bits((16, 40, 2), True), rec_bits((8, 48, 2), True)), hex(p)
    check(A, X[:3000], Y, X[3000:], what='hub operator with a halo panel')


def test_long_hub_rows_many_segments(dev):
    """hub rows of 257..3000 entries (1..12 segments) in a random operator, threshold from the plan"""
    n = 3000
    m = _rand(n, 4000, 6, seed=8, long_rows=[(5, 257), (77, 512), (78, 513), (1500, 3000), (2999, 1000)])
    A = _op(m, dev, plans=True)
    A.ensure_plans(256)
    assert A.hub is not None
    run(A, _X(4000, 256, dev, 8), _L().SPMM_HUB | wide_bits(1, True), hub_thr=A.hub['threshold'], alpha=-2.5, relu=True,
        what='hub segments')


# ------------------------------------------------------------------------------------------------------------------- specials
def _special_X(n, H, dev, seed, subnormals=True):
    X = _X(n, H, dev, seed)
    r = torch.arange(0, n, 37, device=dev)
    sv = [float('nan'), float('inf'), -float('inf'), -0.0] + ([1e-40, -3e-39, 1e-45] if subnormals else [])
    vals = torch.tensor(sv, device=dev)
    X[r, (7 * r) % H] = vals[torch.arange(r.numel(), device=dev) % vals.numel()]
    return X


def _special_op(n, n_cols, seed):
    """random rows; every 41st row is {(0, 0.0), (1, 1.0)}: a stored zero facing column 0 (Inf in X)"""
    m = _rand(n, n_cols, 6, seed=seed)
    rows = [([0, 1], [0.0, 1.0]) if r % 41 == 0 else (m.indices[m.indptr[r]:m.indptr[r + 1]], m.data[m.indptr[r]:m.indptr[r + 1]])
            for r in range(n)]
    return _from_rows(rows, n_cols)


@pytest.mark.parametrize('H', [20, 3, 256, 512])
@pytest.mark.parametrize('alpha', [1.0, -2.5, 2.0 ** -20])
def test_specials(dev, H, alpha):
    """NaN, +-Inf, -0 and subnormals in X; stored zeros facing an Inf (0 * Inf = NaN); relu passes a NaN"""
    n = 1000
    m = _special_op(n, 1200, seed=H)
    A = _op(m, dev)
    X = _special_X(1200, H, dev, H)
    X[0, :] = float('inf')
    vw = 4 if H % 4 == 0 else 1
    want = wide_bits(H // 256, False) if H % 256 == 0 else csr_bits(vw, H, n, m.nnz, False)
    for relu in (False, True):
        Y = run(A, X, want, alpha=alpha, relu=relu, what='specials H=%d alpha=%g relu=%s' % (H, alpha, relu))
        assert torch.isnan(Y[::41]).all()                 # 0 * Inf


@pytest.mark.parametrize('H', [20, 256])
def test_subnormal_sums(dev, H):
    """rows whose exact sums lie in the subnormal range (products 2^-140)"""
    n = 500
    m = _rand(n, 600, 5, seed=3, scale=2.0 ** -70)
    X = _X(600, H, dev, 3) * 2.0 ** -70
    vw = 4
    want = wide_bits(1, False) if H == 256 else csr_bits(vw, H, n, m.nnz, False)
    Y = run(_op(m, dev), X, want, what='subnormal sums H=%d' % H)
    y = Y.abs()
    assert bool(((y > 0) & (y < 2.0 ** -126)).any())
    run(_op(m, dev), X, want, alpha=2.0 ** -20, relu=True, what='subnormal sums H=%d alpha 2^-20' % H)


# ------------------------------------------------------------------------------------------------------------------- empties
@pytest.mark.parametrize('H', [20, 256, 1024])
def test_empties(dev, H):
    from ndcn_amd import hip, CsrOperator
    Z = CsrOperator.from_arrays(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), (0, 64), dev)
    Z._plans_tried = True
    X = _X(64, H, dev, 1)
    assert hip.spmm(Z, X).shape == (0, H) and _path() == 0
    E = CsrOperator.from_arrays(np.zeros(65, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), (64, 64), dev)
    E._plans_tried = True
    Y = hip.spmm(E, X)
    p = _path()
    assert p != 0 and (p & (_L().SPMM_CSR | _L().SPMM_WIDE | _L().SPMM_REC | _L().SPMM_SWEEP))
    assert torch.equal(Y.view(torch.int32), torch.zeros_like(Y, dtype=torch.int32))
    check(E, X, Y, what='nnz = 0')
    # all-empty rows inside a non-empty operator
    m = _rand(300, 64, 4, seed=2)
    m = _from_rows([(([], []) if r % 3 == 0 else (m.indices[m.indptr[r]:m.indptr[r + 1]], m.data[m.indptr[r]:m.indptr[r + 1]]))
                    for r in range(300)], 64)
    want = wide_bits(H // 256, False) if H % 256 == 0 else csr_bits(4, H, 300, m.nnz, False)
    run(_op(m, dev), X, want, what='empty rows H=%d' % H)


@pytest.mark.parametrize('H', [20, 256])
def test_transposed_rectangular(dev, H):
    """A^T of a rectangular operator (the backward's g_X = A^T g)"""
    m = _rand(517, 1200, 5, seed=3)
    A = _op(m, dev)
    At = A.transpose()
    At._plans_tried = True
    X = _X(517, H, dev, 7)
    want = wide_bits(1, False) if H == 256 else csr_bits(4, H, 1200, m.nnz, False)
    run(At, X, want, what='A^T H=%d' % H)


# ------------------------------------------------------------------------------------------------------------------- size edges
def test_lattice_rec_guard_at_two_to_the_22_rows(dev):
    """the record route holds n_rows * 1024 < 2^32: a 2047 x 2047 lattice takes REC, a 2048 x 2048 lattice (2^22 rows) WIDE"""
    for side, rec in ((2047, True), (2048, False)):
        m = _lattice(side)
        n = side * side
        A = _op(m, dev, plans=True)
        A.ensure_plans(256)
        assert A.rec is not None
        X = torch.rand(n, 256, device=dev)
        want = rec_bits((A.rec['rows'], A.rec['cap'], A.rec['kib']), False) if rec else wide_bits(1, False)
        run(A, X, want, rows=sample_rows(n), what='lattice %d' % side)
        del A, X
        torch.cuda.empty_cache()


def test_panels_past_two_to_the_31_elements(dev):
    """wide H = 1024 and scalar H = 257 panels of more than 2^31 elements"""
    for H, n, vw in ((1024, (1 << 21) + 3, 4), (257, (1 << 31) // 257 + 5, 1)):
        m = _rand(n, n, 0, seed=H, lengths=[3, 1, 0, 5, 2, 9])
        A = _op(m, dev)
        X = torch.rand(n, H, device=dev)
        assert X.numel() > (1 << 31)
        want = wide_bits(4, False) if vw == 4 else csr_bits(1, H, n, m.nnz, False)
        run(A, X, want, rows=sample_rows(n), what='H=%d n=%d' % (H, n))
        del A, X, m
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------- no_control
def _np(t):
    return t.cpu()


def _finish_depth(slots):
    """fused2_finish_kernel (rhs_fused2.hip): 256 threads each add ceil(slots / 256) partials from 0, then an 8-level tree"""
    return -(-slots // 256) + 8


def wide_err_depth(n_rows):
    """fp64 additions one z * z term passes through in spmm_wide_kernel's ERROR record: 4 per row a lane walks (launch_wide: 128
    workgroups of 4 waves per XCD at most, no more waves than rows), the 6-step shuffle, then the finish over grid * 4 slots"""
    chunk = -(-n_rows // 8)
    per_xcd = min(128, max((chunk + 3) // 4, 1))
    return 4 * -(-chunk // (per_xcd * 4)) + 6 + _finish_depth(per_xcd * 8 * 4)


def rec_err_depth(n_groups, rows_per_group):
    """the same for spmm_rec_kernel: a compute wave sums rows_per_group / 8 rows per group over ceil(chunk / workgroups) groups
    (launch_rec: 32 workgroups per XCD at most), the 6-step shuffle, the finish over grid * 8 slots"""
    chunk = -(-n_groups // 8)
    wpx = min(32, chunk)
    return 4 * (rows_per_group // 8) * -(-chunk // wpx) + 6 + _finish_depth(wpx * 8 * 8)


def check_err_sum(got, zz, depth, what=''):
    """|got - sum| for non-negative terms summed through `depth` fp64 additions each: <= 1.01 depth 2^-53 sum; the reference is
    math.fsum (correctly rounded: one more half ulp)"""
    s = math.fsum(zz.ravel().tolist())
    print('%s: error sum %r, reference %r, |diff| / sum %.3g, bound %.3g (depth %d)'
          % (what, got, s, abs(got - s) / s, (1.01 * depth + 1) * 2.0 ** -53, depth))
    assert abs(got - s) <= (1.01 * depth + 1) * 2.0 ** -53 * s, (what, got, s, depth)


@pytest.mark.parametrize('route', ['rec8', 'rec16', 'rec48', 'wide', 'wide_order'])
@pytest.mark.parametrize('halo', [False, True])
def test_no_control_epilogues(dev, route, halo):
    """relu(A X) + the stage algebra in the SpMM's epilogue (ndcn_rhs_rk_f32, no_control, H = 256): K against the chain's bits,
    y_next / y_aux against OracleOps over the reference K, the error record's non-finite count exactly and its sum against an fp64
    sum of the same fp32 z * z values, within the depth of the kernel's fp64 summation order (wide_err_depth / rec_err_depth)"""
    from ndcn_amd import hip
    L = _L()
    side, H = 41, 256
    n = side * side
    grid = _lattice(side)
    rnd = _rand(n, n, 7, seed=9)
    m = sp.vstack([grid[:800], rnd[800:]]).tocsr() if route.startswith('wide') else grid
    n_own = 1200 if halo else n
    shape = {'rec8': (8, 32, 1), 'rec16': (16, 40, 2), 'rec48': (8, 48, 2)}.get(route)
    sub = m[:n_own] if halo else m
    sub = sp.csr_matrix(sub)
    if shape:
        A = _op(sub, dev)
        if halo:
            A.lattice_hint = (0, n_own)
        A.group_order = torch.as_tensor(A.detect_stencil_order(), dtype=torch.int32).to(dev)
        A.build_rec_plan(*shape)
    else:
        A = _op(sub, dev)
        if route == 'wide_order':
            A.set_row_order(np.random.RandomState(1).permutation(n_own))
            A._plans_tried = True
    g = torch.Generator(device=dev).manual_seed(2)
    X = torch.rand(n, H, generator=g, device=dev) - 0.3
    y0 = torch.rand(n_own, H, generator=g, device=dev)
    ks = [torch.randn(n_own, H, generator=g, device=dev) for _ in range(5)]
    Xo, Xh = (X[:n_own].contiguous(), X[n_own:].contiguous()) if halo else (X, None)
    cs = [np.float32(c) for c in (0.11, -0.07, 0.23, 0.05, -0.31, 0.19)]
    aux = [np.float32(c) for c in (0.013, -0.02, 0.031, 0.007, -0.011, 0.017)]
    fam = (lambda mode: rec_bits(shape, halo, mode)) if shape else (lambda mode: wide_bits(1, halo, mode))
    rhs_bit = (L.PATH_REC if shape else L.PATH_WIDE) | (L.PATH_HALO if halo else 0)

    def K_checked(K, mode, what):
        assert int(L.load().ndcn_debug_last_rhs_path()) == rhs_bit, what
        assert _path() == fam(mode), '%s: %#x' % (what, _path())
        check(A, Xo, K, Xh, relu=True, what=what)

    K, yn = hip.rhs_rk(A, Xo, None, None, 'combine', y0, [], [cs[5]], no_control=True, X_halo=Xh)
    K_checked(K, L.RK_COMBINE, route + ' combine 0')
    Kc = _np(K)
    for npv in range(6):
        for with_aux in (False, True):
            out = hip.rhs_rk(A, Xo, None, None, 'combine', y0, ks[:npv], cs[:npv] + [cs[5]], no_control=True, X_halo=Xh,
                             aux_cs=(aux[:npv] + [aux[5]]) if with_aux else None)
            assert _path() == fam(L.RK_COMBINE)
            assert torch.equal(out[0].view(torch.int32), K.view(torch.int32))
            kk = [_np(k) for k in ks[:npv]] + [Kc]
            want = OracleOps.combine(_np(y0), kk, cs[:npv] + [cs[5]])
            assert torch.equal(_np(out[1]).view(torch.int32), want.view(torch.int32)), (route, npv, with_aux)
            if with_aux:
                from _oracle_ops import _wsum
                assert torch.equal(_np(out[2]).view(torch.int32), _wsum(kk, aux[:npv] + [aux[5]]).view(torch.int32))
    dt = np.float32(0.37)
    for st in range(4):
        K4, yn = hip.rhs_rk(A, Xo, None, None, 'rk4', y0, ks[:st], [dt], no_control=True, X_halo=Xh)
        assert _path() == fam(L.RK_RK4) and torch.equal(K4.view(torch.int32), K.view(torch.int32))
        want = OracleOps.fixed_stage(2 + st, _np(y0), *([_np(k) for k in ks[:st]] + [Kc]), dt=dt)
        assert torch.equal(_np(yn).view(torch.int32), want.view(torch.int32)), (route, st)
    rtol, atol = np.float32(1e-2), np.float32(1e-3)
    depth = rec_err_depth(A.rec['groups'], shape[0]) if shape else wide_err_depth(n_own)

    def err_ref(npv, y1, rows=slice(None)):
        """the fp32 z * z terms (z = the stage sum / (atol + rtol max_nan(|y0|, |y1|))) and the count of non-finite y1"""
        kk = [_np(k)[rows].numpy() for k in ks[:npv]] + [Kc[rows].numpy()]
        zz, bad = error_terms(_np(y0)[rows].numpy(), _np(y1)[rows].numpy(), kk, cs[:npv] + [cs[5]], rtol, atol)
        return zz, float(bad)

    for npv in range(6):
        Ke, (s1, b1) = hip.rhs_rk(A, Xo, None, None, 'error', y0, ks[:npv], cs[:npv] + [cs[5]], rtol=rtol, atol=atol,
                                  no_control=True, X_halo=Xh)
        assert _path() == fam(L.RK_ERROR) and torch.equal(Ke.view(torch.int32), K.view(torch.int32))
        zz, bad = err_ref(npv, Xo[:n_own])
        assert b1 == bad == 0.0, (route, npv, b1)
        check_err_sum(s1, zz, depth, '%s n_prev %d' % (route, npv))
    # a state with non-finite elements: the record counts them exactly; +-Inf leaves z = 0 there, a NaN makes the sum NaN
    y1 = Xo[:n_own].clone()
    y1[3, 5], y1[n_own - 1, 255], y1[700, 0] = float('inf'), -float('inf'), float('inf')
    for nan in (False, True):
        if nan:
            y1[9, 9] = float('nan')
        Ke, (s1, b1) = hip.rhs_rk(A, Xo, None, None, 'error', y0, ks[:3], cs[:3] + [cs[5]], rtol=rtol, atol=atol,
                                  no_control=True, X_halo=Xh, y1=y1)
        assert _path() == fam(L.RK_ERROR) and torch.equal(Ke.view(torch.int32), K.view(torch.int32))
        zz, bad = err_ref(3, y1)
        assert b1 == bad == (4.0 if nan else 3.0), (b1, bad)
        if nan:
            assert math.isnan(s1), s1
        else:
            check_err_sum(s1, zz, depth, route + ' non-finite y1')


def test_no_control_error_split_over_row_blocks(dev):
    """ERROR over two row blocks of one state (y1 rows per launch, accum on the second): one record, the sum of both"""
    from ndcn_amd import hip
    L = _L()
    m = _rand(3001, 3001, 7, seed=4)
    H = 256
    g = torch.Generator(device=dev).manual_seed(3)
    X = torch.rand(3001, H, generator=g, device=dev)
    y0 = torch.rand(3001, H, generator=g, device=dev)
    k1 = torch.randn(3001, H, generator=g, device=dev)
    cs = [np.float32(0.2), np.float32(-0.3)]
    rec = hip.new_error_record(dev)
    terms, depth = [], 0
    for lo, hi, acc in ((0, 1400, False), (1400, 3001, True)):
        part = sp.csr_matrix(m[lo:hi])
        A = _op(part, dev)
        K, r = hip.rhs_rk(A, X, None, None, 'error', y0[lo:hi].contiguous(), [k1[lo:hi].contiguous()], cs, rtol=1e-2, atol=1e-3,
                          no_control=True, y1=X[lo:hi].contiguous(), accum=acc, record=rec, fetch=acc)
        assert _path() == wide_bits(1, False, L.RK_ERROR)
        check(A, X, K, relu=True, what='error block %d' % lo)
        kk = [k1[lo:hi].cpu().numpy(), K.cpu().numpy()]
        s = (kk[0] * cs[0] + kk[1] * cs[1]).astype(np.float32)
        a0, a1 = np.abs(y0[lo:hi].cpu().numpy()), np.abs(X[lo:hi].cpu().numpy())
        tol = (np.float32(1e-3) + np.float32(1e-2) * np.maximum(a0, a1)).astype(np.float32)
        z = (s / tol).astype(np.float32)
        terms.append((z * z).astype(np.float32).astype(np.float64))
        depth = max(depth, wide_err_depth(hi - lo))
    s1, b1 = r
    assert b1 == 0.0
    check_err_sum(s1, np.concatenate([t.ravel() for t in terms]), depth + 1, 'split')      # + 1: the accumulating add


# ------------------------------------------------------------------------------------------------------------------- gather_rows
@pytest.mark.parametrize('H', [20, 256, 3, 1])
def test_gather_rows(dev, H):
    """gather_rows4_kernel (H % 4 == 0, aligned) and gather_rows_kernel (odd H, a misaligned view); n_idx 0 and 1, repeated and
    unsorted indices"""
    from ndcn_amd import hip
    X = _X(1000, H, dev, H)
    Xm = _misaligned(1000, H, dev, H)
    for idx in ([], [999], [5, 5, 3, 999, 0, 5, 17, 3], list(np.random.RandomState(H).randint(0, 1000, 3333))):
        it = torch.as_tensor(np.asarray(idx, np.int32), device=dev)
        for src in (X, Xm):
            got = hip.gather_rows(src, it)
            assert got.shape == (len(idx), H) and torch.equal(got.view(torch.int32), src[it.long()].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------- truth dynamics
_DYN = {}


def _dyn_case(n):
    """rows of 0..70 entries (cycled) plus one hub row of 5000 entries; a ~ N(0, 1), x in [0.05, 1.05)"""
    if n not in _DYN:
        m = _rand(n, n, 0, seed=n % 1000, lengths=list(range(71)), long_rows=[(7, 5000)])
        x = (0.05 + np.random.RandomState(n % 997).rand(n)).astype(np.float32)
        _DYN.clear()
        _DYN[n] = (m, x)
    return _DYN[n]


def _dyn_check(m, x, got, edge, self_term, self_err, edge_roundings, what):
    """fp64 evaluation of the same fp32 inputs; per row the bound of edge_dynamics_kernel's order: each edge term carries
    `edge_roundings` roundings (counted as separate operations: a contracted form only drops some), then passes ceil(d / 8) lane
    additions, the 3-step shuffle and the final self + acc; the self term carries self_err (a running first-order bound) and the
    final addition.  u = 2^-24, 1.01 for the second-order terms."""
    rp = m.indptr.astype(np.int64)
    d = np.diff(rp)
    rowid = np.repeat(np.arange(m.shape[0]), d)
    x64 = x.astype(np.float64)
    t = edge(m.data.astype(np.float64), x64[rowid], x64[m.indices])
    s = np.bincount(rowid, weights=t, minlength=m.shape[0])
    sa = np.bincount(rowid, weights=np.abs(t), minlength=m.shape[0])
    st = self_term(x64)
    want = st + s
    K = -(-d // 8) + 3 + 1
    bound = 1.01 * ((edge_roundings + K) * U * sa + self_err(x64) + U * np.abs(st))
    err = np.abs(got.astype(np.float64) - want)
    bad = ~(err <= bound)
    print('%s: n %d, worst err / bound %.3g' % (what, m.shape[0], float((err / np.maximum(bound, 1e-300)).max())))
    assert not bad.any(), '%s: %d rows outside the bound; first row %d: got %r want %r bound %r' % (
        what, int(bad.sum()), int(np.argmax(bad)), float(got[np.argmax(bad)]), float(want[np.argmax(bad)]), float(bound[np.argmax(bad)]))


@pytest.mark.parametrize('n', [131071, 131072, 131073, 3 * 131072])
def test_truth_dynamics_against_fp64(dev, n):
    """gene_rhs / mutual_rhs (dynamics.hip edge_dynamics_kernel) at the grid cap of 4096 x 32 rows and around it.  gene: h, f in
    {1, 2} only - the exact ipow paths (x, x * x); non-integer h goes through powf, whose error this test cannot derive, and is out
    of scope here."""
    from ndcn_amd import hip
    m, x = _dyn_case(n)
    A = _op(m, dev)
    xd = torch.from_numpy(x).to(dev)
    for h in (1.0, 2.0):
        for f in (1.0, 2.0):
            b = 1.0
            got = hip.gene_rhs(A, xd, b=b, f=f, h=h).cpu().numpy()
            # p = x^h (h = 2: one rounding), p / (p + 1): two, a * q: one
            edge = lambda a, xi, xj, h=h: a * (xj ** h / (xj ** h + 1.0))
            self_term = lambda xi, f=f: -b * xi ** f
            self_err = lambda xi, f=f: (f - 1.0) * U * np.abs(xi ** f) * abs(b) + U * np.abs(b * xi ** f)
            _dyn_check(m, x, got, edge, self_term, self_err, 3 + (h == 2.0), 'gene h=%g f=%g' % (h, f))
    b, k, c, d, e, hh = 0.1, 5.0, 1.0, 5.0, 0.9, 0.1
    got = hip.mutual_rhs(A, xd, b=b, k=k, c=c, d=d, e=e, h=hh).cpu().numpy()
    # xj xi: one; d + e xj + h xi (positive terms): three as one relative bound; division: one; a *: one

    def mutual_self_err(xi):
        a1 = xi / k
        e_a1 = U * np.abs(a1)
        b1 = 1.0 - a1
        e_b1 = e_a1 + U * np.abs(b1)
        c1 = xi / c
        e_c1 = U * np.abs(c1)
        d1 = c1 - 1.0
        e_d1 = e_c1 + U * np.abs(d1)
        ee = xi * b1
        e_ee = np.abs(xi) * e_b1 + U * np.abs(ee)
        ff = ee * d1
        e_ff = np.abs(ee) * e_d1 + np.abs(d1) * e_ee + U * np.abs(ff)
        return e_ff + U * np.abs(b + ff)

    _dyn_check(m, x, got, lambda a, xi, xj: a * (xj * xi / (d + e * xj + hh * xi)),
               lambda xi: b + xi * (1.0 - xi / k) * (xi / c - 1.0), mutual_self_err, 6, 'mutual')
