"""Dropout on the fused right-hand side on a real MI355X: the kernels against the numpy reference of the mask contract
(tests/_philox.py; ndcn_amd/csrc/dropout.h), bit for bit unless said otherwise - the streaming pass, every route of ops.rhs, the stage
epilogues of ops.rhs_rk, the gradients of autograd_ops.rhs, the fixed-grid training path against the per-operation path, and the
repeatability of a seeded dgnn training step."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _philox
from conftest import load_golden
from oracle import ndcn_oracle as orc

pytestmark = pytest.mark.gpu

SEED = 0x9e3779b97f4a7c15          # both key words in use
P = 0.5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def rand_csr(n_rows, n_cols, per_row, seed):
    rs = np.random.RandomState(seed)
    m = sp.random(n_rows, n_cols, density=min(1.0, per_row / n_cols), random_state=rs, format='csr', dtype=np.float32)
    m.data = (m.data - 0.5).astype(np.float32)
    m.sort_indices()
    return m


def same_bits(got, want):
    """equal as float32 bit patterns, any NaN standing for any NaN"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(nan_g, nan_w) and np.array_equal(got.view(np.uint32)[~nan_g], want.view(np.uint32)[~nan_w]))


def masked(K, p, seed, evaluation):
    """K * mask in numpy: one rounded float32 product per element, NaN and Inf times 0 are NaN"""
    K = K.detach().cpu().numpy()
    with np.errstate(invalid='ignore', over='ignore'):
        return K * _philox.mask(p, seed, evaluation, K.shape[0], K.shape[1])


# --------------------------------------------------------------------------------------------------- the streaming pass

@pytest.mark.parametrize('H', [1, 16, 20, 100, 256])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 2 ** 20 + 1])
def test_dropout_apply_on_ones_is_the_mask(dev, n, H):
    from ndcn_amd import hip
    for p, ev in ((0.5, 0), (0.1, 2 ** 33 + 7)):
        K = torch.ones(n, H, device=dev)
        out = hip.dropout_apply(K, (p, SEED, ev))
        assert out is K
        got = K.cpu().numpy().reshape(-1)
        for first in range(0, n * H, 1 << 24):                  # (the numpy mask in chunks: bounded memory at 2^28 elements)
            cnt = min(1 << 24, n * H - first)
            want = np.where(_philox.kept(p, SEED, ev, cnt, first=first), _philox.scale(p), np.float32(0))
            assert same_bits(got[first:first + cnt], want), (n, H, p, first)


def test_dropout_apply_on_a_misaligned_view_and_specials(dev):
    from ndcn_amd import hip
    n, H = 777, 20
    buf = torch.ones(n * H + 3, device=dev)
    view = buf[1:1 + n * H]
    assert view.data_ptr() % 16 != 0
    hip.dropout_apply(view, (P, SEED, 5))
    got = buf.cpu().numpy()
    assert got[0] == 1.0 and got[-2] == 1.0 and got[-1] == 1.0                        # nothing outside the view is touched
    assert same_bits(got[1:1 + n * H].reshape(n, H), _philox.mask(P, SEED, 5, n, H))   # the index is the position in the VIEW
    # NaN and Inf times a dropped factor stay NaN (x * mask * scale in torch); kept values are one rounded product
    vals = torch.tensor([float('nan'), float('inf'), -0.0, 0.0, 1e-45, 3.4e38, 0.3], device=dev).repeat(64)
    K = vals.clone().view(-1, 7)
    hip.dropout_apply(K, (0.1, SEED, 1))
    assert same_bits(K.cpu().numpy(), masked(vals.view(-1, 7), 0.1, SEED, 1))
    with pytest.raises(Exception) as e:
        hip.dropout_apply(torch.ones(4, 4, device=dev), (1.0, SEED, 0))
    assert getattr(e.value, 'code', None) == -1


def test_dropout_apply_on_a_panel_over_2_31_elements(dev):
    from ndcn_amd import hip
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip('needs ~8 GiB of device memory, %.1f GiB free' % (free / 2 ** 30))
    n = 2 ** 31 + 5
    K = torch.ones(n, device=dev)
    hip.dropout_apply(K, (P, SEED, 3))
    s = float(_philox.scale(P))
    for first, cnt in ((0, 4096), (2 ** 31 - 2048, 2053), (2 ** 30 + 1, 1000)):
        want = np.where(_philox.kept(P, SEED, 3, cnt, first=first), np.float32(s), np.float32(0))
        assert same_bits(K[first:first + cnt].cpu().numpy(), want), first
    kept = int(torch.count_nonzero(K)) / n
    assert abs(kept - 0.5) <= 5 * np.sqrt(0.25 / n)
    del K


# --------------------------------------------------------------------------------------------------- every route of ops.rhs

def _lattice(dev, S=32):
    from ndcn_amd import graphs
    return graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(S)), dev), S * S


def _gnp(dev, n=9000):
    from ndcn_amd import graphs
    op = graphs.normalized_laplacian(graphs.make_graph('random', n, seed=0)).tocsr()
    op.sort_indices()
    return graphs.to_device(op, dev), n


def _random(dev, n, seed=1):
    from ndcn_amd import CsrOperator
    return CsrOperator.from_scipy(rand_csr(n, n, 6, seed), dev), n


ROUTES = {
    # name: (operator factory, H, kwargs, small route?)
    'small_H16': (lambda d: _random(d, 1500), 16, {}, True),
    'small_H20': (lambda d: _random(d, 1500), 20, {}, True),
    'small_H100': (lambda d: _random(d, 1500), 100, {}, True),
    'fused_H256_lattice': (_lattice, 256, {}, False),
    'fused_H256_random': (lambda d: _random(d, 3000), 256, {}, False),
    'composed_H48': (lambda d: _random(d, 6000), 48, {}, False),
    'no_control_row_H20': (lambda d: _random(d, 1500), 20, {'no_control': True}, False),
    'no_control_rec_H256': (_lattice, 256, {'no_control': True}, False),
    'no_control_sweep_H256': (_gnp, 256, {'no_control': True}, False),
    'no_graph_H20': (lambda d: _random(d, 1500), 20, {'no_graph': True}, False),
    'no_graph_H256': (lambda d: _random(d, 1500), 256, {'no_graph': True}, False),
    'neither_H33': (lambda d: _random(d, 1500), 33, {'no_graph': True, 'no_control': True}, False),
}


def _operands(dev, n, H, seed=0, specials=True):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, H, generator=g)
    if specials:
        X[3, :] = float('nan')
        X[n // 2, H // 2] = float('inf')
        X[n - 1, 0] = float('-inf')
    W = (torch.rand(H, H, generator=g) - 0.5) / max(1.0, H ** 0.5) * 4
    b = torch.rand(H, generator=g) - 0.5
    return X.to(dev), W.to(dev), b.to(dev)


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_rhs_with_dropout_is_rhs_times_mask_on_every_route(dev, route):
    from ndcn_amd import hip, _lib
    make, H, kw, small = ROUTES[route]
    A, n = make(dev)
    if small:
        assert int(_lib.load().ndcn_rhs_work_bytes(n, H, _lib.F_RELU)) == 16            # the one-launch route is the one taken
    if route == 'composed_H48':
        assert int(_lib.load().ndcn_rhs_work_bytes(n, H, _lib.F_RELU)) == n * H * 4
    X, W, b = _operands(dev, n, H)
    lib = _lib.load()
    K0 = hip.rhs(A, X, W, b, **kw)
    if route == 'no_control_sweep_H256':
        assert A.sweep is not None                          # (the plans are built by the first call at this width)
    # the route the name promises is the one the p = 0 call took: a dispatch change must not turn two cases into one
    rhs_path, spmm_path = int(lib.ndcn_debug_last_rhs_path()), int(lib.ndcn_debug_last_spmm_path())
    if route == 'fused_H256_lattice':
        assert rhs_path & _lib.PATH_FUSED3, rhs_path
    elif route == 'fused_H256_random':
        assert rhs_path & (_lib.PATH_FUSED2 | _lib.PATH_FUSED3 | _lib.PATH_EXACT32), rhs_path
    elif route == 'no_control_rec_H256':
        assert spmm_path & _lib.SPMM_REC, spmm_path
    elif route == 'no_control_sweep_H256':
        assert spmm_path & _lib.SPMM_SWEEP, spmm_path
    elif route in ('no_control_row_H20', 'composed_H48'):
        assert spmm_path & (_lib.SPMM_CSR | _lib.SPMM_WIDE) and not spmm_path & (_lib.SPMM_REC | _lib.SPMM_SWEEP), spmm_path
    assert bool(torch.isnan(K0).any())
    for p, ev in ((0.5, 0), (0.9, 11)):
        K = hip.rhs(A, X, W, b, dropout=(p, SEED, ev), **kw)
        path = int(_lib.load().ndcn_debug_last_rhs_path())
        assert bool(path & _lib.PATH_DROP_EPI) == small, (route, path)
        if small:
            assert path & _lib.PATH_SMALL
        want = masked(K0, p, SEED, ev)
        assert same_bits(K.cpu().numpy(), want), route
        dropped = _philox.mask(p, SEED, ev, n, H) == 0
        assert bool((np.isnan(want) & dropped).any())                                   # NaN stays NaN where dropped too
    # eval mode / p = 0 callers: the argument left out and None are the parent's launch - the same bits
    assert same_bits(hip.rhs(A, X, W, b, dropout=None, **kw).cpu().numpy(), K0.cpu().numpy())


def test_unsupported_combinations_raise_einval(dev):
    from ndcn_amd import hip, _lib
    A, n = _random(dev, 1500)
    X, W, b = _operands(dev, n, 20, specials=False)
    with pytest.raises(_lib.NdcnHipError) as e:
        hip.rhs(A, X[:900].contiguous(), W, b, X_halo=X[900:].contiguous(), dropout=(P, SEED, 0))
    assert e.value.code == _lib.EINVAL and 'halo' in str(e.value)
    with pytest.raises(_lib.NdcnHipError) as e:
        hip.rhs(A, X, W, b, relu=False, dropout=(P, SEED, 0))
    assert e.value.code == _lib.EINVAL
    for bad in (0.0, 1.0, -0.1, float('nan')):
        with pytest.raises(_lib.NdcnHipError) as e:
            hip.rhs(A, X, W, b, dropout=(bad, SEED, 0))
        assert e.value.code == _lib.EINVAL
    y0 = torch.rand_like(X)
    with pytest.raises(_lib.NdcnHipError) as e:
        hip.rhs_rk(A, X[:900].contiguous(), W, b, 'combine', y0, [], [0.1], X_halo=X[900:].contiguous(), dropout=(P, SEED, 0))
    assert e.value.code == _lib.EINVAL


# --------------------------------------------------------------------------------------------------- the stage epilogues

RK_ROUTES = {
    'small_H20': (lambda d: _random(d, 1500), 20, {}, True),
    'small_H100': (lambda d: _random(d, 1500), 100, {}, True),
    'composed_H48': (lambda d: _random(d, 6000), 48, {}, False),
    'fused_H256_lattice': (_lattice, 256, {}, False),
    'no_control_row_H20': (lambda d: _random(d, 1500), 20, {'no_control': True}, False),
    'no_control_rec_H256': (_lattice, 256, {'no_control': True}, False),
    'no_graph_H20': (lambda d: _random(d, 1500), 20, {'no_graph': True}, False),
}


@pytest.mark.parametrize('route', sorted(RK_ROUTES))
def test_rhs_rk_with_dropout_consumes_the_masked_K(dev, route):
    """K is the masked K; y_next, the second combination and the rk4 stage inputs are what the un-fused kernels (hip.combine,
    hip.fixed_stage) give on that masked K, bit for bit on the one-launch route and on the composed ones.  The error record: the
    composed routes run hip.error's own kernel (equal); the one-launch epilogue sums in fp64 where the stand-alone kernel sums a
    panel of this size in ATen's float32 order - the p = 0 launch agrees with it to 1e-5 of the sum (tests/test_gpu_kernels.py:
    test_narrow_panel_rhs_is_one_launch_and_equals_the_composed_kernels), and that is what the masked launch is held to."""
    from ndcn_amd import hip, _lib
    make, H, kw, small = RK_ROUTES[route]
    A, n = make(dev)
    X, W, b = _operands(dev, n, H, seed=3, specials=False)
    g = torch.Generator().manual_seed(9)
    y0 = torch.rand(n, H, generator=g).to(dev)
    ks = [torch.randn(n, H, generator=g).to(dev) for _ in range(5)]
    cs = [np.float32(c) for c in (0.11, -0.07, 0.23, 0.05, -0.31, 0.19)]
    ce = [np.float32(c) for c in (0.013, 0.021, -0.017, 0.009, -0.004, 0.025)]
    K0 = hip.rhs(A, X, W, b, **kw)
    lib = _lib.load()
    ev = 0
    for npv in range(6):
        ev += 1
        drop = (P, SEED, ev)
        Km = torch.from_numpy(masked(K0, *drop)).to(dev)
        c = cs[:npv] + [cs[5]]
        K1, yn, E = hip.rhs_rk(A, X, W, b, 'combine', y0, ks[:npv], c, aux_cs=ce[:npv] + [ce[5]], dropout=drop, **kw)
        assert bool(int(lib.ndcn_debug_last_rhs_path()) & _lib.PATH_DROP_EPI) == small
        assert torch.equal(K1, Km), (route, npv)
        assert torch.equal(yn, hip.combine(y0, ks[:npv] + [Km], c)), (route, npv)
        assert torch.equal(E, hip.combine(torch.zeros_like(y0), ks[:npv] + [Km], ce[:npv] + [ce[5]])), (route, npv)
        K2, (s1, b1) = hip.rhs_rk(A, X, W, b, 'error', y0, ks[:npv], c, rtol=1e-2, atol=1e-3, dropout=drop, **kw)
        s2, b2 = hip.error(y0, X, ks[:npv] + [Km], c, 1e-2, 1e-3)
        print('%s n_prev=%d: error sum %r (launch) %r (hip.error), relative difference %.3e' % (route, npv, s1, s2, abs(s1 - s2) / abs(s2)))
        assert torch.equal(K2, Km) and b1 == b2 == 0.0
        if small:
            assert abs(s1 - s2) <= 1e-5 * abs(s2)
        else:
            assert s1 == s2
    dt = np.float32(0.37)
    for st in range(4):
        drop = (0.1, SEED + 1, st)
        Km = torch.from_numpy(masked(K0, *drop)).to(dev)
        K3, yn = hip.rhs_rk(A, X, W, b, 'rk4', y0, ks[:st], [dt], dropout=drop, **kw)
        assert torch.equal(K3, Km) and torch.equal(yn, hip.fixed_stage(2 + st, y0, *(ks[:st] + [Km]), dt=dt)), (route, st)


# --------------------------------------------------------------------------------------------------- gradients

@pytest.mark.parametrize('name', ['rhs_grid400_H20_default_coo', 'rhs_grid400_H20_no_control_coo',
                                  'rhs_grid400_H20_no_graph_coo', 'rhs_grid400_H256_default_coo'])
def test_rhs_gradients_with_dropout(dev, name):
    """autograd_ops.rhs(dropout=t) against fp64 torch autograd of relu(z) * mask with the numpy mask, at the shapes of
    tests/test_gpu_autograd.py::test_rhs_gradients under its tolerance times s (every gradient term is linear in s)."""
    from ndcn_amd import CsrOperator
    from ndcn_amd.autograd_ops import rhs as ag_rhs
    d = load_golden(name)
    H = d['W'].shape[0]
    kw = dict(no_graph='no_graph' in name, no_control='no_control' in name)
    A = CsrOperator.from_arrays(d['indptr'], d['indices'], d['data'], d['shape'], dev)
    g = torch.randn(400, H, generator=torch.Generator().manual_seed(0))
    for p, ev in ((0.5, 4), (0.1, 0)):
        s = float(_philox.scale(p))
        m = T(_philox.mask(p, SEED, ev, 400, H)).double()
        x = T(d['x']).to(dev).requires_grad_(True)
        W, b = T(d['W']).to(dev).requires_grad_(True), T(d['b']).to(dev).requires_grad_(True)
        y = ag_rhs(A, x, W, b, kw['no_graph'], kw['no_control'], dropout=(p, SEED, ev))
        (y * g.to(dev)).sum().backward()
        Ao = orc.coo_from_csr(d['indptr'], d['indices'], d['data'], d['shape']).double()
        Wo, bo, xo = (T(d[k]).double().requires_grad_(True) for k in ('W', 'b', 'x'))
        yo = orc.odefunc_rhs(Ao, xo, Wo, bo, **kw) * m
        (yo * g.double()).sum().backward()
        assert float((y.detach().cpu().double() - yo.detach()).abs().max()) < 2e-5 * s
        tol = 1e-4 * s
        print('%s p=%.1f: g_x %.3e' % (name, p, rel(x.grad.cpu().double(), xo.grad)))
        assert rel(x.grad.cpu().double(), xo.grad) < tol
        if not kw['no_control']:
            print('   g_W %.3e g_b %.3e' % (rel(W.grad.cpu().double(), Wo.grad), rel(b.grad.cpu().double(), bo.grad)))
            assert rel(W.grad.cpu().double(), Wo.grad) < tol and rel(b.grad.cpu().double(), bo.grad) < tol
        else:
            assert W.grad is None or float(W.grad.abs().max()) == 0.0


@pytest.mark.parametrize('variant', ['no_graph', 'neither'])
def test_gradient_sign_cases(dev, variant):
    """z = x (identity weight, no bias, no graph): kept with z < 0, kept with z > 0, dropped with z > 0, dropped with z < 0 all occur;
    the gradient wrt x is exactly s * g where the element is kept AND z > 0, exactly 0 elsewhere."""
    from ndcn_amd.autograd_ops import rhs as ag_rhs
    n, H = 64, 8
    gen = torch.Generator().manual_seed(1)
    xh = torch.randn(n, H, generator=gen)
    gh = torch.randn(n, H, generator=gen)
    m = T(_philox.mask(P, SEED, 2, n, H))
    kept, pos = m > 0, xh > 0
    for a in (kept & pos, kept & ~pos, ~kept & pos, ~kept & ~pos):
        assert bool(a.any())
    x = xh.to(dev).requires_grad_(True)
    W = torch.eye(H, device=dev).requires_grad_(True)
    b = torch.zeros(H, device=dev).requires_grad_(True)
    y = ag_rhs(None, x, W, b, True, variant == 'neither', dropout=(P, SEED, 2))
    assert torch.equal(y.detach().cpu(), torch.relu(xh) * m)
    (y * gh.to(dev)).sum().backward()
    want = torch.where(kept & pos, gh * 2.0, torch.zeros_like(gh))
    assert torch.equal(x.grad.cpu(), want)
    if variant == 'no_graph':
        assert torch.equal(b.grad.cpu(), want.sum(0)) or rel(b.grad.cpu(), want.sum(0)) < 1e-6


# --------------------------------------------------------------------------------------------------- fixed-grid training

def _case(dev, S, H, no_control=False, no_graph=False, seed=0, dropout=0.5):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    L = graphs.normalized_laplacian(graphs.grid_8_neighbor(S))
    torch.manual_seed(seed)
    f = ODEFunc(H, graphs.to_device(L, dev), dropout=dropout, no_control=no_control, no_graph=no_graph).to(dev)
    x0 = torch.rand(L.shape[0], H, generator=torch.Generator().manual_seed(seed + 1))
    return f, L, x0


def _fixed_grid_pair(dev, method, variant, shape, options=None):
    from ndcn_amd import torchdiffeq as ode
    S, H = shape
    f, L, x0 = _case(dev, S, H, no_control=variant == 'no_control', no_graph=variant == 'no_graph', seed=11)
    f.train()
    t = torch.sort(torch.rand(9, generator=torch.Generator().manual_seed(6)) * 1.5).values
    t[0] = 0.0
    wts = torch.randn(9, x0.shape[0], H, generator=torch.Generator().manual_seed(7))
    kw = {} if options is None else {'options': options}

    def run(flags, seed=5):
        os.environ.update(flags)
        try:
            f.zero_grad()
            torch.manual_seed(seed)
            y0 = x0.to(dev).requires_grad_(True)
            y = ode.odeint(f, y0, t.to(dev), method=method, **kw)
            node = type(y.grad_fn).__name__
            # the fused-launch path is one node for the whole solve; the per-operation path ends in a stack of per-tick results
            assert (node in ('_FixedGridSolveBackward', '_SubstepSolveBackward')) == ('NDCN_FIXED_GRID_GRAD' not in flags), (node, flags)
            if 'NDCN_FIXED_GRID_GRAD' not in flags:
                assert node == ('_SubstepSolveBackward' if options else '_FixedGridSolveBackward'), node
            (y * wts.to(dev)).sum().backward()
            return (y.detach().cpu(), y0.grad.cpu(), None if f.wt.weight.grad is None else f.wt.weight.grad.cpu().clone(),
                    None if f.wt.bias.grad is None else f.wt.bias.grad.cpu().clone())
        finally:
            for k in flags:
                del os.environ[k]
    ya, gya, gWa, gba = run({'NDCN_SOLVE_SMALL_GRAD': '0'})
    yb, gyb, gWb, gbb = run({'NDCN_SOLVE_SMALL_GRAD': '0', 'NDCN_FIXED_GRID_GRAD': '0'})
    assert torch.equal(ya, yb)
    assert bool(torch.isfinite(ya).all())

    def close(a, b, what):
        scale = max(1.0, float(b.abs().max()))
        print('%s: max difference %.3e, scale %.3e' % (what, float((a - b).abs().max()), scale))
        assert float((a - b).abs().max()) <= 1e-4 * scale, (what, float((a - b).abs().max()), scale)
    close(gya, gyb, 'g_y0')
    if variant != 'no_control':
        close(gWa, gWb, 'g_W')
        close(gba, gbb, 'g_b')
    else:
        assert gWa is None or float(gWa.abs().max()) == 0.0
    # the masks are live: another seed moves the trajectory, and so does eval mode
    yc = run({'NDCN_SOLVE_SMALL_GRAD': '0'}, seed=6)[0]
    assert not torch.equal(ya, yc)
    f.eval()
    with torch.no_grad():
        ye = ode.odeint(f, x0.to(dev), t.to(dev), method=method, **kw).cpu()
    f.train()
    assert not torch.equal(ya, ye)
    # and the default dispatch (no switch set) is the fused-launch path: the same bits again
    yd = run({})[0]
    assert torch.equal(ya, yd)


@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('variant', ['default', 'no_control', 'no_graph'])
@pytest.mark.parametrize('shape', [(45, 20), (30, 256), (12, 33)])
def test_fixed_grid_training_with_dropout_fused_launches_equal_the_per_op_path(dev, method, variant, shape):
    """The cases of test_gpu_small_solve.py::test_fixed_grid_training_through_fused_launches_equals_the_per_op_autograd_path with
    ODEFunc(dropout=0.5).train(): under the same torch.manual_seed the fused-launch path (_FixedGridSolve: masks re-created in the reverse
    sweep from the evaluation numbers) and the per-operation path (NDCN_FIXED_GRID_GRAD=0: ODEFunc.forward numbers its evaluations one
    by one) give the same trajectory bit for bit and gradients within that test's bound."""
    _fixed_grid_pair(dev, method, variant, shape)


@pytest.mark.parametrize('variant', ['default', 'no_control'])
@pytest.mark.parametrize('shape', [(45, 20), (30, 256)])
def test_rk4_with_step_size_and_dropout(dev, variant, shape):
    """_SubstepSolve: the interval re-run of the reverse pass gives grid step i the evaluation numbers it had in the forward pass"""
    _fixed_grid_pair(dev, 'rk4', variant, shape, options={'step_size': 0.07})


# --------------------------------------------------------------------------------------------------- the dgnn default

def _cora(dev):
    from ndcn_amd import CsrOperator
    d = load_golden('dataset_cora')
    g = load_golden('operators_cora')
    n = int(g['n'])
    adj = CsrOperator.from_arrays(g['alpha00_indptr'], g['alpha00_indices'], g['alpha00_data'], (n, n), dev)
    feats = sp.csr_matrix((d['feat_data'], d['feat_indices'].astype(np.int64), d['feat_indptr']), shape=tuple(d['feat_shape']))
    return (adj, torch.from_numpy(feats.toarray()).to(dev), torch.from_numpy(d['labels'].astype(np.int64)).to(dev),
            torch.from_numpy(d['idx_train'].astype(np.int64)).to(dev))


def test_seeded_dgnn_training_steps_repeat(dev):
    """Two Adam steps of the dgnn model at its defaults (Cora, hidden 16, dropout 0.5, dopri5 rtol = atol = 0.1) after the same
    torch.manual_seed: equal losses and gradients; another seed: another loss.  Every evaluation is ONE autograd node."""
    import torch.nn as nn
    import torch.nn.functional as F
    from ndcn_amd.neural_dynamics import ODEBlock2, ODEFunc
    adj, feats, labels, idx = _cora(dev)
    t = torch.linspace(0, 2., 5).float().to(dev)

    def run(seed):
        torch.manual_seed(0)
        model = nn.Sequential(nn.Linear(feats.shape[1], 16), nn.Tanh(),
                              ODEBlock2(ODEFunc(16, adj, dropout=0.5), t, rtol=0.1, atol=0.1, method='dopri5', terminal=True),
                              nn.Linear(16, int(labels.max()) + 1)).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)
        torch.manual_seed(seed)
        model.train()
        losses = []
        for _ in range(2):
            opt.zero_grad()
            out = model(feats)
            loss = F.cross_entropy(out[idx], labels[idx])
            loss.backward()
            opt.step()
            losses.append(loss.detach().cpu())
        return losses, [p.grad.detach().cpu().clone() for p in model.parameters()], out

    la, ga, out = run(17)
    lb, gb, _ = run(17)
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    assert all(torch.equal(a, b) for a, b in zip(ga, gb))
    assert all(bool(torch.isfinite(g).all()) for g in ga) and float(ga[2].abs().max()) > 0      # (ga[2]: the ODEFunc weight)
    lc, _, _ = run(18)
    assert not torch.equal(la[0], lc[0])
    # one autograd node per evaluation: the graph behind the output holds the fused node and none of the per-operation ones
    names, stack, seen = set(), [out.grad_fn], set()
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        stack.extend(nf for nf, _ in fn.next_functions)
    assert '_RhsBackward' in names, sorted(names)
    assert not any(nm.startswith(('_Spmm', '_Linear', 'Relu', 'NativeDropout')) for nm in names), sorted(names)


def test_eval_mode_and_p0_are_the_parent_launch(dev):
    from ndcn_amd import hip
    from ndcn_amd import torchdiffeq as ode
    for S, H in ((20, 20), (12, 256)):
        f, L, x0 = _case(dev, S, H, seed=2, dropout=0.5)
        x = x0.to(dev)
        want = hip.rhs(f.A, x, f.wt.weight, f.wt.bias)
        f.eval()
        with torch.no_grad():
            assert torch.equal(f(torch.tensor(0.0), x), want)
        assert torch.equal(f(torch.tensor(0.0), x).detach(), want)
        f0, _, _ = _case(dev, S, H, seed=2, dropout=0.0)
        f0.train()
        assert torch.equal(f0(torch.tensor(0.0), x).detach(), want)
        # training mode with 0 < p < 1: the fused launch with a mask - and the generator is read once per call
        f.train()
        torch.manual_seed(1)
        a = f(torch.tensor(0.0), x).detach()
        torch.manual_seed(1)
        b = f(torch.tensor(0.0), x).detach()
        assert torch.equal(a, b) and not torch.equal(a, want)
        dropped = float(((a == 0) & (want > 0)).sum()) / float((want > 0).sum())
        assert 0.4 < dropped < 0.6                                # about half of the positive outputs are dropped
        # a solve in eval mode draws nothing from the generator
        f.eval()
        torch.manual_seed(3)
        r = torch.rand(2)
        torch.manual_seed(3)
        with torch.no_grad():
            ode.odeint(f, x, torch.tensor([0., .1, .2]).to(dev), method='euler')
        assert torch.equal(torch.rand(2), r)
