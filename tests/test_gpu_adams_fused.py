"""The three-pass step of method 'adams' (csrc/adams_vc.hip: ndcn_adams_predict_f32 / ndcn_adams_correct_f32 / ndcn_adams_update_f32)
on a real MI355X: each kernel against the ndcn_scale_f32 / ndcn_rk_combine_f32 / ndcn_rk_error_f32 calls core.Adams.step composes the
step from - bit for bit, panels and sums -, its argument errors, and whole solves with hip.set_adams_fused(1) against (0) in one process.

ndcn_rk_combine_f32 takes at most 8 terms, so the composed predictor exists up to order 9 only; the order-12 predictor is compared with
the numpy restatement (tests/_adams_vc.py, which tests/test_adams_fused_host.py holds to core.Adams.step) instead, bit for bit."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import _adams_vc as vc

pytestmark = pytest.mark.gpu
f32 = np.float32
BIG = (1 << 18) + 4            # above the ATen-order bound (2^18), a multiple of 4: the 16-byte path


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def bits(x):
    return struct.pack('d', float(x))


def same_panel(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


class Case:
    """random panels and coefficients of one step at `order`; off: the panel named there starts one float past a 16-byte boundary"""

    def __init__(self, dev, order, max_order, n, off=None, seed=0):
        g = torch.Generator().manual_seed(1000 * order + 10 * max_order + seed)
        self.order, self.max_order, self.n = order, max_order, n

        def panel(name):
            x = torch.randn(n + 1, generator=g)
            return x.to(dev)[1:] if off == name else x[:n].to(dev)
        self.y0 = panel('y0')
        self.phis = [panel('phi%d' % j) for j in range(order)]
        self.nf, self.nf2 = panel('nf'), panel('nf2')
        r = lambda k: [float(v) for v in (torch.rand(k, generator=g) + 0.5)]
        self.betas = [None] + [f32(v) for v in r(order)][1:]
        self.m = max(1, order - 1)
        self.cs = [f32(0.01 * v) for v in r(self.m)]
        self.c_corr = f32(0.013)
        c = [f32(0.02 * v) for v in r(4)]
        # every sum the order has a link for; the fourth is what the solver leaves out at order == max_order
        self.coefs = [c[0], c[1], c[2] if order >= 2 else None, c[3] if order < max_order else None]
        self.rtol, self.atol = 1e-3, 1e-4
        self.n_out = min(order + 1, max_order)

    def composed(self, hip, p_next):
        """what core.Adams.step launches: the explicit phi, the chain of single-term combines, y_next, one error call per sum, the new phi"""
        o = self.order
        ephi = [self.phis[0]] + [hip.scale(self.phis[j], self.betas[j]) for j in range(1, o)]
        pred = hip.combine(self.y0, ephi[:self.m], self.cs) if self.m <= 8 else None
        ip = [self.nf]
        for j in range(1, o + 1):
            ip.append(hip.combine(ip[j - 1], [ephi[j - 1]], [f32(-1.0)]))
        y_next = hip.combine(p_next, [ip[o - 1]], [self.c_corr])
        link = [o, o - 1, o - 2, o]
        sums = [None if self.coefs[q] is None else hip.error(self.y0, y_next, [ip[link[q]]], [self.coefs[q]], self.rtol, self.atol)[0]
                for q in range(4)]
        new = [self.nf2]
        for j in range(1, self.n_out):
            new.append(hip.combine(new[j - 1], [ephi[j - 1]], [f32(-1.0)]))
        return pred, y_next, sums, new

    def restated(self):
        a = lambda t: t.cpu().numpy()
        phis = [a(p) for p in self.phis]
        p_next = vc.predict(a(self.y0), phis, self.betas, self.cs, self.order)
        y_next, r2 = vc.correct(a(self.nf), phis, self.betas, self.order, p_next, a(self.y0), self.c_corr, self.coefs, self.rtol, self.atol)
        return p_next, y_next, r2


def run_fused(hip, c):
    p_next = hip.adams_predict(c.y0, c.phis, c.betas, c.cs, c.order)
    y_next, sums = hip.adams_correct(c.nf, c.phis, c.betas, c.order, p_next, c.y0, c.c_corr, c.coefs, c.rtol, c.atol)
    new = hip.adams_update(c.nf2, c.phis, c.betas, c.order, c.n_out)
    return p_next, y_next, sums, new


SIZES = {'n1': (1, None), 'n5': (5, None), 'n7': (7, None), 'vec': (BIG, None), 'scalar': (BIG + 1, None), 'misaligned': (BIG, 'y0')}


@pytest.mark.parametrize('size', list(SIZES))
@pytest.mark.parametrize('trunc', [False, True], ids=['max12', 'max_is_order'])
@pytest.mark.parametrize('order', [1, 2, 3, 4, 9, 12])
def test_kernels_equal_the_composed_calls(dev, order, trunc, size):
    """Sizes below 8 and above 2^18 elements: ndcn_rk_error_f32 takes its parallel fp64 pair there, so every sum is compared as raw
    float64 bits.  `misaligned`: y0 (read by the predictor, the corrector and the composed error call alike) one float off a 16-byte
    boundary - both forms take the single-element path.  Order 9 is the highest whose predictor ndcn_rk_combine_f32 can form."""
    from ndcn_amd import hip
    n, off = SIZES[size]
    c = Case(dev, order, order if trunc else 12, n, off)
    p_next, y_next, sums, new = run_fused(hip, c)
    pred, y_ref, s_ref, new_ref = c.composed(hip, p_next)
    if pred is not None:
        assert same_panel(p_next, pred)
    else:
        assert p_next.cpu().numpy().tobytes() == c.restated()[0].tobytes()
    assert same_panel(y_next, y_ref)
    for q in range(4):
        assert (sums[q] is None) == (c.coefs[q] is None)
        if sums[q] is not None:
            assert bits(sums[q]) == bits(s_ref[q]), (q, sums[q], s_ref[q])
    assert len(new) == len(new_ref) == c.n_out and new[0] is c.nf2
    for a, b in zip(new[1:], new_ref[1:]):
        assert same_panel(a, b)


@pytest.mark.parametrize('order', [3, 12])
def test_sums_inside_the_aten_range_against_fp64(dev, order):
    """4096 elements: ndcn_rk_error_f32 sums in ATen's float32 order here (core.Adams keeps the composed calls at this size); the fused
    call is still callable and sums the same float32 r^2 values in fp64.  All terms are non-negative, so any fp64 summation order stays
    within n * 2^-52 relative of the fp64 sum of the restatement's r^2 values; the panels are the composed ones bit for bit."""
    from ndcn_amd import hip, _lib
    n = 4096
    assert 8 < n <= int(_lib.load().ndcn_aten_norm_max())
    c = Case(dev, order, 12, n)
    p_next, y_next, sums, new = run_fused(hip, c)
    pred, y_ref, _, new_ref = c.composed(hip, p_next)
    rp, ry, r2 = c.restated()
    assert same_panel(y_next, y_ref) and (pred is None or same_panel(p_next, pred))
    assert p_next.cpu().numpy().tobytes() == rp.tobytes() and y_next.cpu().numpy().tobytes() == ry.tobytes()
    for a, b in zip(new[1:], new_ref[1:]):
        assert same_panel(a, b)
    assert sums[3] is None if order == 12 else all(s is not None for s in sums)
    for q in range(4):
        if sums[q] is None:
            continue
        want = float(r2[q].sum(dtype=np.float64))
        print('sum %d: fused %.17g  fp64 of the restatement %.17g' % (q, sums[q], want))
        assert abs(sums[q] - want) <= n * 2.0 ** -52 * want


def test_signed_zero_inf_and_nan(dev):
    """-0.0, an Inf and a NaN in known places of phi_1 (and -0.0 against +0.0 in the chain's first link): panels equal bit for bit,
    NaN included; the sums are NaN where the composed ones are."""
    from ndcn_amd import hip
    c = Case(dev, 4, 12, BIG)
    c.phis[1][3] = -0.0
    c.phis[1][10] = float('inf')
    c.phis[1][17] = float('nan')
    c.nf[5] = -0.0
    c.nf2[5] = -0.0
    c.phis[0][5] = 0.0                   # -0 - (+0): +0 as combine forms it
    p_next, y_next, sums, new = run_fused(hip, c)
    pred, y_ref, s_ref, new_ref = c.composed(hip, p_next)
    assert same_panel(p_next, pred) and same_panel(y_next, y_ref)
    for a, b in zip(new[1:], new_ref[1:]):
        assert same_panel(a, b)
    assert bool(torch.isnan(y_next[17])) and new[1][5].item() == 0.0 and not bool(torch.signbit(new[1][5]))
    for q in range(4):
        assert np.isnan(sums[q]) == np.isnan(s_ref[q]) and (np.isnan(sums[q]) or bits(sums[q]) == bits(s_ref[q]))
    assert any(np.isnan(s) for s in sums)


def test_argument_errors(dev):
    """every NDCN_EINVAL case: the code, an error text, and outputs that were pre-filled with 7.0 still 7.0"""
    from ndcn_amd import _lib
    from ndcn_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    n, o = 64, 3
    P, F = ctypes.c_void_p, ctypes.c_float
    mk = lambda: torch.randn(n, device=dev)
    y, nf, pn = mk(), mk(), mk()
    phis = [mk() for _ in range(o)]
    outs = [torch.full((n,), 7.0, device=dev) for _ in range(4)]
    out4 = torch.full((4,), 7.0, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.ndcn_adams_correct_ws_bytes()), dtype=torch.uint8, device=dev)
    beta, cs, coef = (F * 12)(*[1.0] * 12), (F * 12)(*[0.1] * 12), (F * 4)(*[0.1] * 4)
    arr = lambda ts: (P * len(ts))(*[t.data_ptr() if t is not None else 0 for t in ts])

    def predict(out=outs[0], y_=y, ph=phis, order=o, n_=n):
        return lib.ndcn_adams_predict_f32(ptr(out), ptr(y_), arr(ph), beta, cs, order, n_, stream_ptr())

    def correct(out=outs[0], ph=phis, order=o, nf_=nf, ws_bytes=None, mask=15):
        return lib.ndcn_adams_correct_f32(ptr(out), ptr(nf_), arr(ph), beta, order, ptr(pn), ptr(y), 0.1, coef, mask, 1e-3, 1e-4, n,
                                          ptr(out4), ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, stream_ptr())

    def update(os_=None, ph=phis, order=o, n_out=4, nf_=nf):
        return lib.ndcn_adams_update_f32(arr(os_ if os_ is not None else outs), ptr(nf_), arr(ph), beta, order, n_out, n, stream_ptr())

    twelve = phis * 5
    bad = [
        lambda: predict(order=0, ph=twelve), lambda: predict(order=13, ph=twelve), lambda: predict(y_=None),
        lambda: predict(ph=[phis[0], None, phis[2]]), lambda: predict(out=None), lambda: predict(n_=0),
        lambda: correct(order=0, ph=twelve), lambda: correct(order=13, ph=twelve), lambda: correct(nf_=None),
        lambda: correct(ph=[phis[0], phis[1], None]), lambda: correct(ws_bytes=ws.numel() - 8), lambda: correct(order=1, mask=4),
        lambda: update(order=0, ph=twelve), lambda: update(order=13, ph=twelve), lambda: update(nf_=None), lambda: update(n_out=5),
        lambda: update(os_=[outs[0], outs[1], None, outs[3]]), lambda: update(ph=[None, phis[1], phis[2]]),
        # an output aliasing another output
        lambda: update(os_=[outs[0], outs[1], outs[1], outs[3]]),
    ]
    for i, call in enumerate(bad):
        assert call() == _lib.EINVAL, i
        assert lib.ndcn_last_error().decode().strip(), i
    # an output aliasing an input: the shared panel holds 7.0 and keeps it
    seven = outs[0]
    for call in (lambda: predict(out=seven, y_=seven), lambda: predict(out=seven, ph=[phis[0], seven, phis[2]]),
                 lambda: correct(out=seven, nf_=seven), lambda: correct(out=seven, ph=[seven, phis[1], phis[2]]),
                 lambda: update(nf_=outs[2]), lambda: update(ph=[phis[0], outs[3], phis[2]])):
        assert call() == _lib.EINVAL and lib.ndcn_last_error().decode().strip()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs) and bool((out4 == 7.0).all())


# ------------------------------------------------------------------------------------------------ whole solves
class Counter:
    NAMES = ('adams_predict', 'adams_correct', 'adams_update', 'scale')

    def __init__(self, monkeypatch):
        from ndcn_amd.ops import HipOps
        self.n = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(HipOps, name, staticmethod(self._wrap(name, getattr(HipOps, name))))

    def _wrap(self, name, fn):
        def call(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return call

    def take(self):
        out, self.n = self.n, dict.fromkeys(self.NAMES, 0)
        return out


@pytest.fixture(scope='module')
def lattice(dev):
    from ndcn_amd import graphs
    op = graphs.normalized_laplacian(graphs.grid_8_neighbor(65))
    return op, graphs.to_device(op, dev)


def make_f(lattice, dev, H, as_module=True):
    from ndcn_amd import hip
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(0)
    f = ODEFunc(H, lattice[1]).to(dev).eval()
    if as_module:
        return f
    W, b = f.wt.weight.detach(), f.wt.bias.detach()
    return lambda t, y: hip.rhs(lattice[1], y, W, b)


def solve_both(counter, f, x0, t, **kw):
    """the same solve with the fused step and with the composed calls: (trajectory, step log incl. nfe, call counts) each"""
    from ndcn_amd import hip, torchdiffeq as ode
    out = []
    try:
        for mode in (1, 0):
            hip.set_adams_fused(mode)
            log = []
            with torch.no_grad():
                y = ode.odeint(f, x0, t, method='adams', step_log=log, **kw)
            out.append((y, [tuple(r) for r in log], counter.take()))
    finally:
        hip.set_adams_fused(-1)
    return out


def assert_same_solve(fused, composed):
    ys = fused[0] if isinstance(fused[0], tuple) else (fused[0],)
    yc = composed[0] if isinstance(composed[0], tuple) else (composed[0],)
    assert all(torch.equal(a, b) for a, b in zip(ys, yc))
    assert fused[1] == composed[1] and fused[1][-1][0] == 'nfe'
    assert all(fused[2][k] >= 1 for k in ('adams_predict', 'adams_correct', 'adams_update')) and fused[2]['scale'] == 0
    assert all(composed[2][k] == 0 for k in ('adams_predict', 'adams_correct', 'adams_update'))


@pytest.fixture
def counted(monkeypatch):
    return Counter(monkeypatch)


X0_SEED = 3


def x0_of(dev, H):
    return torch.rand(4225, H, generator=torch.Generator().manual_seed(X0_SEED)).to(dev)


@pytest.mark.parametrize('as_module', [True, False], ids=['module', 'callable'])
def test_loose_solve_fused_equals_composed(dev, lattice, counted, as_module):
    """65 x 65 lattice, H = 64 (270 400 elements, above 2^18): rtol 1e-3, atol 1e-4, 5 ticks on [0, 1]"""
    f = make_f(lattice, dev, 64, as_module)
    fused, composed = solve_both(counted, f, x0_of(dev, 64), torch.linspace(0., 1., 5).to(dev), rtol=1e-3, atol=1e-4)
    assert_same_solve(fused, composed)
    assert composed[2]['scale'] >= 1


TIGHT = dict(rtol=1e-7, atol=1e-9)
TIGHT_T = (0., 1., 5)


def test_tight_solve_fused_equals_composed(dev, lattice, counted):
    """rtol 1e-7, atol 1e-9, 5 ticks on [0, 1].  At rtol 1e-6, atol 1e-8 the composed path reaches order 5 on these inputs but rejects
    no step (66 attempts, none rejected); a decade tighter its log holds 148 attempts, 8 of them rejected, orders up to 5.  Both
    properties are asserted on the composed run's log, so that the comparison cannot pass on a log without either."""
    f = make_f(lattice, dev, 64)
    fused, composed = solve_both(counted, f, x0_of(dev, 64), torch.linspace(*TIGHT_T).to(dev), **TIGHT)
    steps = composed[1][:-1]
    assert any(r[3] == 0.0 for r in steps), 'no rejected step'
    assert max(r[2] for r in steps) >= 4, 'order stays below 4'
    assert_same_solve(fused, composed)


def test_max_order_3(dev, lattice, counted):
    f = make_f(lattice, dev, 64)
    fused, composed = solve_both(counted, f, x0_of(dev, 64), torch.linspace(0., 1., 5).to(dev), rtol=1e-5, atol=1e-6, options={'max_order': 3})
    assert max(r[2] for r in composed[1][:-1]) == 3
    assert_same_solve(fused, composed)


def test_tuple_state(dev, lattice, counted):
    """two tensors, both above the bound: one adams_correct read-back each, accept / worst / min(e1 + e2) over the lists as composed"""
    from ndcn_amd import hip
    f = make_f(lattice, dev, 64)
    W, b, A = f.wt.weight.detach(), f.wt.bias.detach(), lattice[1]
    g = lambda t, y: (hip.rhs(A, y[0], W, b), hip.rhs(A, y[1], W, b))
    x0 = (x0_of(dev, 64), 0.5 * x0_of(dev, 64) + 0.1)
    fused, composed = solve_both(counted, g, x0, torch.linspace(0., 1., 5).to(dev), rtol=1e-4, atol=1e-5)
    assert isinstance(fused[0], tuple) and len(fused[0]) == 2
    assert_same_solve(fused, composed)
    assert fused[2]['adams_correct'] == 2 * (len(fused[1]) - 1)


def test_below_the_bound_the_fused_kernels_are_not_called(dev, lattice, counted):
    """4225 x 20 = 84 500 elements, NDCN_ATEN_NORM_MAX left alone: the error sums keep ATen's order, so the step keeps today's launches"""
    f = make_f(lattice, dev, 20)
    fused, composed = solve_both(counted, f, x0_of(dev, 20), torch.linspace(0., 1., 5).to(dev), rtol=1e-3, atol=1e-4)
    assert torch.equal(fused[0], composed[0]) and fused[1] == composed[1]
    assert all(fused[2][k] == 0 for k in ('adams_predict', 'adams_correct', 'adams_update')) and fused[2]['scale'] >= 1


def test_loose_solve_against_the_reference_algorithm(dev, lattice):
    """the fused solve against the CPU oracle's method='adams' on the same inputs; trajectory only (above the bound neither path sums in
    ATen's order, so orders and accept flags are not compared); the tolerance is test_adams_golden's"""
    from ndcn_amd import torchdiffeq as ode, hip
    from oracle import ndcn_oracle as orc
    op = lattice[0]
    f = make_f(lattice, dev, 64)
    x0, t = x0_of(dev, 64), torch.linspace(0., 1., 5)
    assert hip.adams_fused_on() == 1
    with torch.no_grad():
        y = ode.odeint(f, x0, t.to(dev), rtol=1e-3, atol=1e-4, method='adams')
    fo = orc.OracleODEFunc(orc.coo_from_csr(op.indptr, op.indices, op.data, op.shape), f.wt.weight.detach().cpu(), f.wt.bias.detach().cpu())
    ref = orc.odeint(fo, x0.cpu(), t, rtol=1e-3, atol=1e-4, method='adams')
    err = np.abs(y.cpu().numpy() - ref.numpy())
    scale = max(1.0, float(ref.abs().max()))
    print('L1 %.3e  max %.3e' % (err.mean(), err.max()))
    assert err.mean() < 1e-5 * scale, 'L1 %.3e' % err.mean()
    assert err.max() < 2e-4 * scale, 'max %.3e' % err.max()


def test_with_a_gradient_the_graph_stays_per_operation(dev, lattice, counted):
    from ndcn_amd import hip, torchdiffeq as ode
    f = make_f(lattice, dev, 64)
    t = torch.linspace(0., .5, 3).to(dev)
    res = []
    try:
        for mode in (1, 0):
            hip.set_adams_fused(mode)
            x0 = x0_of(dev, 64).requires_grad_()
            y = ode.odeint(f, x0, t, rtol=1e-3, atol=1e-4, method='adams')
            y[-1].sum().backward()
            res.append((y.detach(), x0.grad.clone(), counted.take()))
    finally:
        hip.set_adams_fused(-1)
    assert all(r[2][k] == 0 for r in res for k in ('adams_predict', 'adams_correct', 'adams_update'))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
