"""csrc/solve_small.hip - the whole fixed-grid solve and its reverse sweep in one launch each - on every operator shape the drivers feed
it, not only the 8-neighbour grid: rows of 0 .. 73 entries, CSR arrays that do not fit LDS, operators that are not their own transpose,
and the sizes at which the host picks another template instantiation.

  forward   every tick bit for bit against tests/_small_solve.py - a numpy restatement of the arithmetic the file's header documents,
            pinned on the CPU by tests/test_small_solve_host.py - and against the per-step path (DeviceSolver.advance)
  reverse   gradients of sum_i <w_i, y(t_i)> against float64 autograd through the oracle's restated solver, the project's bound
            2e-4 * max(1, max |ref|)
  routes    every case asserts the exact word of ndcn_debug_last_small_route() - the template arguments of the kernel that ran.  The
            expected words below are literals (no size formula of the library is restated here); for the drivers' four networks they
            are the rows of the route table in DESIGN.md, and the library agreed with every one of them.

Instantiations nothing reaches (asserted here by the gates' two sides, listed in DESIGN.md): solve_small_bwd_fast_kernel<4, 16 | 20, *>
- the fast sweep needs 289 (H = 16) / 238 (H = 20) rows for its row groups' reduction to fit, and 4 passes hold 256 / 192."""
import functools
import os

import numpy as np
import pytest
import torch

import _small_solve as ss
from oracle import ndcn_oracle as orc

pytestmark = pytest.mark.gpu

GEN, FAST, RK = 'generic', 'fast', 'rk'
EMPTY = (0, 7, 150, 299)                                    # the nodes removed from the 300-row band: the first, the last, two inside

# name -> (operator, H)
CASES = {
    # the drivers' --network choices at the README size
    'random_h20': (lambda: ss.driver_operator('random'), 20),
    'random_h16': (lambda: ss.driver_operator('random'), 16),
    'power_law_h20': (lambda: ss.driver_operator('power_law'), 20),
    'power_law_h16': (lambda: ss.driver_operator('power_law'), 16),
    'small_world_h20': (lambda: ss.driver_operator('small_world'), 20),
    'small_world_h16': (lambda: ss.driver_operator('small_world'), 16),
    'community_h20': (lambda: ss.driver_operator('community'), 20),
    'community_h16': (lambda: ss.driver_operator('community'), 16),
    # G(n, p) whose CSR arrays fit LDS in neither direction, at 4 passes (192 rows, mean degree 120) and at 10 (450 rows)
    'random192_dense': (lambda: ss.driver_operator('random', 192, mean_degree=120), 20),
    'random450': (lambda: ss.driver_operator('random', 450), 20),
    # the ELL width gate: ceil3(longest row) <= 18
    'band16': (lambda: ss.band(300, 16), 16),
    'band17': (lambda: ss.band(300, 17), 16),
    'band18': (lambda: ss.band(300, 18), 16),
    'band19': (lambda: ss.band(300, 19), 16),
    'diagonal': (lambda: ss.band(300, 1), 16),
    # rows without entries, node 0 and node n - 1 among them
    'band17_empty_rows': (lambda: ss.without_nodes(ss.band(300, 17), EMPTY), 16),
    'band19_empty_rows': (lambda: ss.without_nodes(ss.band(300, 19), EMPTY), 16),
    'power_law_empty_rows': (lambda: ss.without_nodes(ss.driver_operator('power_law'), (0, 1, 57, 399)), 20),
    # operators that are not their own transpose at a shape the fast sweep would take
    'band_values': (lambda: ss.band(300, 9, 'values'), 16),
    'band_upper': (lambda: ss.band(300, 9, 'upper'), 16),
    # a ring (3 entries per row) where the number of passes changes, at 1..3 rows and at the widths' edges
    'ring192': (lambda: ss.ring(192), 20),
    'ring193': (lambda: ss.ring(193), 20),
    'ring432': (lambda: ss.ring(432), 20),
    'ring433': (lambda: ss.ring(433), 20),
    'ring576': (lambda: ss.ring(576), 20),
    'ring1': (lambda: ss.ring(1), 20),
    'ring2': (lambda: ss.ring(2), 20),
    'ring3': (lambda: ss.ring(3), 20),
    'ring200_h1': (lambda: ss.ring(200), 1),
    'ring50_h33': (lambda: ss.ring(50), 33),
    'ring40_h64': (lambda: ss.ring(40), 64),
    # the fast sweep's gates at width <= 9: the row groups' reduction fits from 238 (H = 20) / 289 (H = 16) rows, four panels and the
    # ELL image of width 9 fit LDS up to 407 rows (H = 20); 239: 30 row groups of 8 own rows, 4 own none
    'ring237': (lambda: ss.ring(237), 20),
    'ring238': (lambda: ss.ring(238), 20),
    'ring239': (lambda: ss.ring(239), 20),
    'band9_407': (lambda: ss.band(407, 9), 20),
    'band9_408': (lambda: ss.band(408, 9), 20),
    'ring288_h16': (lambda: ss.ring(288), 16),
    'ring289_h16': (lambda: ss.ring(289), 16),
}

# name -> forward (family, MAXIT, CSR_LDS), the Euler training pair keeps S / K, Euler reverse (family, MAXIT, CSR_LDS, symmetric) or None
# where the one-launch sweep declines the shape (2 (H^2 + H) threads for the parameter gradients: H <= 21)
EXPECT = {
    'random_h20':            ((GEN, 12, False), False, (GEN, 12, False, True)),
    'random_h16':            ((GEN, 12, True), False, (GEN, 12, False, True)),
    'power_law_h20':         ((GEN, 12, True), False, (GEN, 12, True, True)),
    'power_law_h16':         ((GEN, 12, True), False, (GEN, 12, True, True)),
    'small_world_h20':       ((FAST, 12, True), False, (GEN, 12, True, True)),
    'small_world_h16':       ((FAST, 12, True), True, (FAST, 9, False, True)),
    'community_h20':         ((GEN, 12, True), False, (GEN, 12, False, True)),
    'community_h16':         ((GEN, 12, True), False, (GEN, 12, False, True)),
    'random192_dense':       ((GEN, 4, False), False, (GEN, 4, False, True)),
    'random450':             ((GEN, 12, False), False, (GEN, 12, False, True)),
    'band16':                ((FAST, 12, True), True, (FAST, 9, False, True)),
    'band17':                ((FAST, 12, True), True, (FAST, 9, False, True)),
    'band18':                ((FAST, 12, True), True, (FAST, 9, False, True)),
    'band19':                ((GEN, 12, True), False, (GEN, 12, True, True)),
    'diagonal':              ((FAST, 12, True), True, (FAST, 9, False, True)),
    'band17_empty_rows':     ((FAST, 12, True), True, (FAST, 9, False, True)),
    'band19_empty_rows':     ((GEN, 12, True), False, (GEN, 12, True, True)),
    'power_law_empty_rows':  ((GEN, 12, True), False, (GEN, 12, True, True)),
    'band_values':           ((FAST, 12, True), False, (GEN, 12, True, False)),
    'band_upper':            ((FAST, 12, True), False, (GEN, 12, True, False)),
    'ring192':               ((FAST, 4, True), False, (GEN, 4, True, True)),
    'ring193':               ((FAST, 12, True), False, (GEN, 12, True, True)),
    'ring432':               ((FAST, 12, True), True, (FAST, 9, False, True)),
    'ring433':               ((FAST, 12, True), True, (FAST, 12, False, True)),
    'ring576':               ((FAST, 12, True), False, (GEN, 12, True, True)),
    'ring1':                 ((FAST, 4, True), False, (GEN, 4, True, True)),
    'ring2':                 ((FAST, 4, True), False, (GEN, 4, True, True)),
    'ring3':                 ((FAST, 4, True), False, (GEN, 4, True, True)),
    'ring200_h1':            ((GEN, 4, True), False, (GEN, 4, True, True)),
    'ring50_h33':            ((GEN, 4, True), False, None),
    'ring40_h64':            ((GEN, 4, True), False, None),
    'ring237':               ((FAST, 12, True), False, (GEN, 12, True, True)),
    'ring238':               ((FAST, 12, True), True, (FAST, 9, False, True)),
    'ring239':               ((FAST, 12, True), True, (FAST, 9, False, True)),
    'band9_407':             ((FAST, 12, True), True, (FAST, 9, False, True)),
    'band9_408':             ((FAST, 12, True), False, (GEN, 12, True, True)),
    'ring288_h16':           ((FAST, 12, True), False, (GEN, 12, True, True)),
    'ring289_h16':           ((FAST, 12, True), True, (FAST, 9, False, True)),
}

METHODS = ('euler', 'midpoint', 'rk4')
T5 = np.array([0.0, 0.13, 0.5, 0.55, 1.0], np.float32)      # an irregular grid of 5 ticks
T6 = np.array([0.0, 0.2, 0.3, 0.65, 0.7, 1.0], np.float32)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _lib():
    from ndcn_amd import _lib as L
    return L


def word(direction, family, maxit, csr_lds, H, keep=False, grid=False, symmetric=False, method='euler'):
    """the value of ndcn_debug_last_small_route() (include/ndcn_hip.h NDCN_SSR_*)"""
    L = _lib()
    fam = {GEN: L.SSR_GENERIC, FAST: L.SSR_FAST, RK: L.SSR_RK}[family]
    ht = H if family == FAST else 0
    return (direction | fam | (maxit << L.SSR_MAXIT_SHIFT) | (L.SSR_CSR_LDS if csr_lds else 0) | (ht << L.SSR_HT_SHIFT) |
            (L.SSR_KEEP if keep else 0) | (L.SSR_GRID if grid else 0) | (L.SSR_SYMMETRIC if symmetric else 0) |
            (L.METHODS[method] << L.SSR_METHOD_SHIFT))


def last_route():
    return int(_lib().load().ndcn_debug_last_small_route())


@functools.lru_cache(maxsize=None)
def operator(name):
    m = CASES[name][0]()
    assert m.nnz >= 1 and m.has_sorted_indices
    return m


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(W, b, y0) on the host: nn.Linear's default initialisation, a state in [0, 1)"""
    m, H = operator(name), CASES[name][1]
    torch.manual_seed(0)
    lin = torch.nn.Linear(H, H)
    y0 = torch.rand(m.shape[0], H, generator=torch.Generator().manual_seed(1))
    return lin.weight.detach().clone(), lin.bias.detach().clone(), y0


def odefunc(name, dev, no_graph=False, no_control=False):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    W, b, _ = inputs(name)
    f = ODEFunc(CASES[name][1], graphs.to_device(operator(name), dev), no_graph=no_graph, no_control=no_control).to(dev)
    f.load_state_dict({'wt.weight': W, 'wt.bias': b})
    return f


@functools.lru_cache(maxsize=None)
def restated(name, method, ticks=None, no_graph=False, no_control=False, step_size=None, nan_at=None):
    """the restatement's trajectory, computed once per case"""
    m = operator(name)
    W, b, y0 = (x.numpy() for x in inputs(name))
    if nan_at is not None:
        y0 = y0.copy()
        y0[nan_at] = np.nan
    t = T5 if ticks is None else np.asarray(ticks, np.float32)
    return ss.solve((m.indptr, m.indices, m.data), W, b, y0, t, method, no_graph=no_graph, no_control=no_control, step_size=step_size)


@functools.lru_cache(maxsize=None)
def float64_gradients(name, method, ticks=None, no_graph=False, no_control=False):
    """(g_y0, g_W, g_b) of sum_i <w_i, y(t_i)> by float64 autograd through the oracle's restated solver, and the weights w"""
    m = operator(name)
    W, b, y0 = inputs(name)
    t = torch.from_numpy(T6 if ticks is None else np.asarray(ticks, np.float32))
    w = torch.randn((len(t),) + tuple(y0.shape), generator=torch.Generator().manual_seed(7))
    A = orc.coo_from_csr(m.indptr, m.indices, m.data, m.shape).double()
    Wo, bo, yo = (x.double().clone().requires_grad_(True) for x in (W, b, y0))
    y = orc.odeint(orc.OracleODEFunc(A, Wo, bo, no_graph=no_graph, no_control=no_control), yo, t.double(), method=method)
    (y * w.double()).sum().backward()
    return yo.grad, (None if no_control else Wo.grad), (None if no_control else bo.grad), w


def train(name, dev, method, ticks=None, env=None, **variant):
    """one forward + backward through odeint -> (y, g_y0, g_W, g_b, route after the forward launch, route after the reverse launch,
    the name of the autograd node)"""
    from ndcn_amd import torchdiffeq as ode
    W, b, y0h = inputs(name)
    t = torch.from_numpy(T6 if ticks is None else np.asarray(ticks, np.float32))
    w = float64_gradients(name, method, ticks=ticks, **variant)[3]
    env = dict(env or {})
    if method != 'euler':
        env['NDCN_SOLVE_SMALL_RK_MAX'] = '1000000'          # (the default gate of the midpoint / RK4 sweep is 4 608 elements)
    os.environ.update(env)
    try:
        f = odefunc(name, dev, **variant)
        y0 = y0h.to(dev).requires_grad_(True)
        y = ode.odeint(f, y0, t.to(dev), method=method)
        torch.cuda.synchronize()
        r_fwd = last_route()
        (y * w.to(dev)).sum().backward()
        torch.cuda.synchronize()
        r_bwd = last_route()
    finally:
        for k in env:
            del os.environ[k]
    gW = None if f.wt.weight.grad is None else f.wt.weight.grad.cpu()
    gb = None if f.wt.bias.grad is None else f.wt.bias.grad.cpu()
    return y.detach().cpu(), y0.grad.cpu(), gW, gb, r_fwd, r_bwd, type(y.grad_fn).__name__


def worst_ratio(what, got, ref):
    """max over (g_y0, g_W, g_b) of |got - ref| / (2e-4 * max(1, max |ref|)): the project's gradient bound holds while this is <= 1"""
    worst = 0.0
    for g, r, label in zip(got, ref, ('g_y0', 'g_W', 'g_b')):
        if r is None:
            assert g is None or float(g.abs().max()) == 0.0, label
            continue
        assert torch.isfinite(g).all(), label
        ratio = float((g.double() - r).abs().max()) / (2e-4 * max(1.0, float(r.abs().max())))
        worst = max(worst, ratio)
    print('[small-solve gradients] %s: worst |err| / bound = %.3e' % (what, worst))
    return worst


def per_step(f, y0, t32, method):
    """the same solve one tick per call (ndcn_solver_advance: one right-hand-side launch + stage kernels per step)"""
    from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver
    solver = DeviceSolver(f, y0.shape[0], method)
    ys = torch.empty((len(t32),) + tuple(y0.shape), dtype=torch.float32, device=y0.device)
    ys[0] = y0
    tt = [float(v) for v in t32]
    solver.begin(ys[0], tt[0])
    for i in range(1, len(tt)):
        solver.advance(tt[i], ys[i])
    torch.cuda.synchronize()
    solver.close()
    return ys


# ------------------------------------------------------------------------------------------------------------------ forward

@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('name', sorted(CASES))
def test_forward_is_the_restated_arithmetic_bit_for_bit(dev, name, method):
    """5 irregular ticks: the kernel EXPECT names ran; every tick has the restatement's bits (NaN positions equal: none here); the
    per-step path, which ran other kernels (the route word is untouched by it), gives the same bits."""
    from ndcn_amd import torchdiffeq as ode
    H = CASES[name][1]
    f = odefunc(name, dev).eval()
    y0 = inputs(name)[2].to(dev)
    with torch.no_grad():
        y = ode.odeint(f, y0, torch.from_numpy(T5).to(dev), method=method)
        torch.cuda.synchronize()
        route = last_route()
        ys = per_step(f, y0, T5, method)
    family, maxit, csr_lds = EXPECT[name][0]
    assert route == word(_lib().SSR_FWD, family, maxit, csr_lds, H, method=method), (name, method, hex(route))
    assert last_route() == route
    assert ss.same_bits(y.cpu().numpy(), restated(name, method))
    assert torch.isfinite(y).all()
    assert torch.equal(y, ys)


def test_rows_beyond_twelve_passes_are_declined(dev):
    """577 rows at H = 20 are 13 passes of 16 waves x 3 rows: ndcn_solve_small_supported says no, in both directions (576: yes)"""
    from ndcn_amd import graphs
    L = _lib()
    lib = L.load()
    for n, want in ((576, 1), (577, 0)):
        A = graphs.to_device(ss.ring(n), dev)
        for backward in (0, 1):
            assert lib.ndcn_solve_small_supported(A.view_ref(), 20, L.F_RELU, L.M_EULER, backward) == want, (n, backward)


def test_a_nan_reaches_exactly_the_rows_that_read_it(dev):
    """power_law: nb is a neighbour of the 73-entry hub.  y0[nb, 3] = NaN: after one Euler step the NaN sits in every column
    of exactly the rows that store column nb (the Linear's chain multiplies it by every weight) - the hub's long gather among them, its
    mostly-finished neighbour lanes not - and the restatement has the same NaN positions and the same bits elsewhere at every tick."""
    from ndcn_amd import torchdiffeq as ode
    name, H = 'power_law_h20', 20
    m = operator(name)
    hub = int(np.diff(m.indptr).argmax())
    nb = int([c for c in m[hub].indices if c != hub][0])
    assert int(np.diff(m.indptr).max()) == 73
    f = odefunc(name, dev).eval()
    y0 = inputs(name)[2].clone()
    y0[nb, 3] = float('nan')
    t = T5[:3]
    with torch.no_grad():
        y = ode.odeint(f, y0.to(dev), torch.from_numpy(t).to(dev), method='euler')
        torch.cuda.synchronize()
    family, maxit, csr_lds = EXPECT[name][0]
    assert last_route() == word(_lib().SSR_FWD, family, maxit, csr_lds, H)
    y = y.cpu().numpy()
    readers = np.unique(m.tocsc()[:, nb].indices)
    nan_rows = np.nonzero(np.isnan(y[1]).any(axis=1))[0]
    assert hub in readers and 1 < len(readers) < m.shape[0] and np.array_equal(nan_rows, readers)
    assert np.isnan(y[1][readers]).all()
    assert ss.same_bits(y, restated(name, 'euler', ticks=tuple(t), nan_at=(nb, 3)))


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('name', ['small_world_h16', 'power_law_h20', 'random_h20'])
def test_sub_stepped_solve_per_storage_form(dev, name, method):
    """options={'step_size': 0.1} (the GRID kernels) on the ELL image, on CSR in LDS and on CSR read from global memory: ticks inside
    a step (0.13, 0.55), coincident ticks (0.5, 1.0)"""
    from ndcn_amd import torchdiffeq as ode
    H = CASES[name][1]
    f = odefunc(name, dev).eval()
    with torch.no_grad():
        y = ode.odeint(f, inputs(name)[2].to(dev), torch.from_numpy(T5).to(dev), method=method, options={'step_size': 0.1})
        torch.cuda.synchronize()
    family, maxit, csr_lds = EXPECT[name][0]
    assert last_route() == word(_lib().SSR_FWD, family, maxit, csr_lds, H, grid=True, method=method), hex(last_route())
    assert ss.same_bits(y.cpu().numpy(), restated(name, method, step_size=0.1))


# ------------------------------------------------------------------------------------------------------------------ reverse

EULER_VARIANTS = [(name, 'default') for name in sorted(CASES)] + [('random_h20', 'no_graph'), ('random_h20', 'no_control')]


@pytest.mark.parametrize('name,variant', EULER_VARIANTS)
def test_euler_reverse_against_float64_autograd(dev, name, variant):
    """6 ticks: the forward launch (with S / K kept where EXPECT says so) and the reverse launch EXPECT names ran; the trajectory has
    the restatement's bits; g_y0, g_W, g_b within 2e-4 * max(1, max |ref|) of float64 autograd.  Where S / K are kept, the re-forming
    pair (NDCN_SOLVE_SMALL_KEEP=0) gives equal bits.  The view's `symmetric` field reads 2 for the two operators that are not their
    own transpose, and they run the generic sweep with a separate A^T.  H = 33 / 64: the one-launch sweep declines (it forms the
    parameter gradients with 2 (H^2 + H) threads), the solve trains through the library's per-step loops and is held to the same
    bound.  Measured on an MI355X: worst |err| / bound per case between 3.5e-4 (ring1) and 2.1e-3 (random450)."""
    from ndcn_amd import graphs
    L = _lib()
    H = CASES[name][1]
    kw = dict(no_graph=variant == 'no_graph', no_control=variant == 'no_control')
    fwd, keep, bwd = EXPECT[name]
    if variant != 'default':                                # the plain generic kernels: nothing is packed or kept for the variants
        fwd, keep, bwd = (GEN, fwd[1], fwd[2] and not kw['no_graph']), False, (GEN, bwd[1], bwd[2] and not kw['no_graph'], not kw['no_graph'])
    A = graphs.to_device(operator(name), dev)
    view = A.view(need_symmetric=True)
    flags = L.F_RELU | (L.F_NO_GRAPH if kw['no_graph'] else 0) | (L.F_NO_CONTROL if kw['no_control'] else 0)
    assert view.symmetric == (2 if name in ('band_values', 'band_upper') else 1)
    assert L.load().ndcn_solve_small_supported(A.view_ref(), H, flags, L.M_EULER, 1) == (0 if bwd is None else 1)
    assert L.load().ndcn_solve_small_keep_supported(A.view_ref(need_symmetric=True), H, flags) == int(keep)
    y, gy, gW, gb, r_fwd, r_bwd, node = train(name, dev, 'euler', **kw)
    ref = float64_gradients(name, 'euler', ticks=None, **kw)
    assert ss.same_bits(y.numpy(), restated(name, 'euler', ticks=tuple(T6), **kw))
    if bwd is None:
        assert node == '_NativeFixedGridBackward', node
    else:
        assert node == '_SmallEulerSolveBackward', node
        assert r_fwd == word(L.SSR_FWD, fwd[0], fwd[1], fwd[2], H, keep=keep), (name, hex(r_fwd))
        assert r_bwd == word(L.SSR_BWD, bwd[0], bwd[1], bwd[2], H, keep=keep, symmetric=bwd[3]), (name, hex(r_bwd))
    assert worst_ratio('%s %s euler' % (name, variant), (gy, gW, gb), ref[:3]) <= 1.0
    if keep:
        y2, gy2, gW2, gb2, r_fwd2, r_bwd2, _ = train(name, dev, 'euler', env={'NDCN_SOLVE_SMALL_KEEP': '0'})
        assert r_fwd2 == word(L.SSR_FWD, fwd[0], fwd[1], fwd[2], H) and r_bwd2 == word(L.SSR_BWD, bwd[0], bwd[1], bwd[2], H, symmetric=True)
        for a, b2 in ((y, y2), (gy, gy2), (gW, gW2), (gb, gb2)):
            assert torch.equal(a, b2)


# name -> (MAXIT, CSR_LDS, symmetric) of solve_small_bwd_rk_kernel
RK_EXPECT = {
    'random192_dense': (4, False, True),
    'random_h20': (9, False, True),
    'random450': (12, False, True),
    'ring576': (12, True, True),
    'band_values': (9, True, False),
}


@pytest.mark.parametrize('method', ['midpoint', 'rk4'])
@pytest.mark.parametrize('name', sorted(RK_EXPECT))
def test_midpoint_and_rk4_reverse_against_float64_autograd(dev, name, method):
    """the one-launch midpoint / RK4 reverse sweep (NDCN_SOLVE_SMALL_RK_MAX raised over its default size gate) at 4, 9 and 12 passes
    with the CSR arrays read from global memory, at 12 passes with them in LDS, and with a separate A^T"""
    L = _lib()
    H = CASES[name][1]
    y, gy, gW, gb, r_fwd, r_bwd, node = train(name, dev, method)
    assert node == '_SmallEulerSolveBackward', node
    fwd = EXPECT[name][0]
    maxit, csr_lds, symmetric = RK_EXPECT[name]
    assert r_fwd == word(L.SSR_FWD, fwd[0], fwd[1], fwd[2], H, method=method), hex(r_fwd)
    assert r_bwd == word(L.SSR_BWD, RK, maxit, csr_lds, H, symmetric=symmetric, method=method), hex(r_bwd)
    assert ss.same_bits(y.numpy(), restated(name, method, ticks=tuple(T6)))
    assert worst_ratio('%s %s' % (name, method), (gy, gW, gb), float64_gradients(name, method, ticks=None)[:3]) <= 1.0


def test_129_ticks_hand_the_state_and_the_adjoint_between_two_launches(dev):
    """random operator, 129 Euler ticks: a launch covers 128, so each direction runs two - the second forward launch starts from the
    first's last tick, the second reverse launch from the adjoint the first left in g_y0.  Forward: the restatement's bits and the
    per-step path's; gradients within the float64 bound."""
    L = _lib()
    name, H = 'random_h20', 20
    t = tuple(np.linspace(0.0, 1.0, 130, dtype=np.float32))
    y, gy, gW, gb, r_fwd, r_bwd, node = train(name, dev, 'euler', ticks=t)
    fwd, keep, bwd = EXPECT[name]
    assert node == '_SmallEulerSolveBackward' and not keep
    assert r_fwd == word(L.SSR_FWD, fwd[0], fwd[1], fwd[2], H) and r_bwd == word(L.SSR_BWD, bwd[0], bwd[1], bwd[2], H, symmetric=bwd[3])
    assert ss.same_bits(y.numpy(), restated(name, 'euler', ticks=t))
    with torch.no_grad():
        ys = per_step(odefunc(name, dev).eval(), inputs(name)[2].to(dev), np.asarray(t, np.float32), 'euler')
    assert torch.equal(y, ys.cpu())
    assert worst_ratio('random_h20 euler, 129 ticks', (gy, gW, gb), float64_gradients(name, 'euler', ticks=t)[:3]) <= 1.0
