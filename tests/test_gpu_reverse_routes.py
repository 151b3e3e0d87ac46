"""Every solver-VJP kernel of rk_bwd.hip (combine_bwd, error_bwd, rms_bwd, dense_bwd, dense_bwd_multi, dot_diff, pull) on fp32 inputs
against an fp64 evaluation of the reference's expression of the same op - misc.py:71-76 (rms norm), misc.py:146-157 (error ratio with
tol = atol + rtol max(|y0|, |y1|)), interp.py:21-65 + dopri5.py:39-45 (dense output), misc.py:22-25 (linear combination) - at the sizes
where a grid-stride loop runs once or twice, on both element paths, each case asserting its kernel, element path and grid through
ndcn_debug_last_rk_bwd_path.

Bounds are per element, in terms of the same expression evaluated in fp64 on absolute values (u = 2^-24; every bound allows hipcc's
default contraction of a * b + c into one FMA; scalars are fp32 values, so the reference sees the kernel's own coefficients):
  combine   gk_j = acc_j + c_j g                2.01 u (|acc_j| + |c_j g|)       (u: c_j g alone, a single rounding)
            gy0 = acc_y0 + g                    u (|acc_y0| + |g|)
  dots      fp32 products summed in fp64        1.01 (u + n 2^-53) sum |products|   (any summation tree of n terms: n - 1 roundings)
            (pull / dot_diff: e = ua - ub rounded first: 2 u in place of u)
  pull      out = [mask <= 0 ? 0 :] base + ((c_0 p_0 + c_1 p_1) + ...), each product and sum rounded on its own (rk_combine's order and
            rounding): BIT-EQUAL to the same fp32 torch ops on the device and to ndcn_rk_combine_f32 on the same panels, masked; both
            within (n_p + 1) u (|base| + sum |c_j p_j|) of fp64
  error     E = sum |c_j k_j|, T = atol + rtol max(|y0|, |y1|), S = 2 E inv_n / T^2 (the magnitude of s = d r / d e):
            e takes n_k roundings of E, tol 2 of T, s = 2 q inv_n / tol 5 more (inv_n is rounded to fp32: one of them)
            gk_j   (n_k + 12) u (|g_r c_j| S + |acc_j|)
            gy0/1  (2 n_k + 16) u (|g_r| rtol (E / T) S + |acc|)        (q s: both factors' errors, then g_r, rtol, + acc)
            d_j    1.01 ((n_k + 9) u + n 2^-53) sum S |k_j|
  rms       V = (|a| + |b|) / scale, scale = atol + |y| rtol:  ga, gb  8 u |coef| V / scale ;  gy  16 u |coef| V^2 rtol / scale
  dense     per weight w(x) (a polynomial in x of <= 5 terms, times dt, times c_mid): <= 15 roundings of W(|x|) = the same polynomial on
            |x|, |dt|, |c_mid| with every coefficient's magnitude:  gy0 / gy1 / gk_j   16 u (W |g| + |acc|);  ticks of one launch add
            three roundings each: (16 + 3 nt) u (sum_t W(x_t) |g_t| + |acc|)
            <g, d o / d x>, <g, d o / d dt>: <= 23 fp32 roundings per element of the magnitude expression, then fp64:
            1.01 (32 u + n nt 2^-53) sum |g| |d o / d .|(abs)
torch.max splits its gradient in half on ties |y0| == |y1| and abs has gradient 0 at 0: the fp64 reference is torch autograd through
torch.max(a0.abs(), a1.abs()), so the halves and signs are torch's own.  A NaN input: NaN at the same positions, finite elements in bound.
The ReLU mask of pull is torch's threshold_backward: 0 where mask <= 0, the gradient elsewhere, a NaN mask included."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
E53 = 2.0 ** -53
CAP = 1024                        # rk_bwd.hip bwd_grid: the streaming VJPs' grid cap; the dense VJPs and rms run on 2048
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
SPECIALS = (0.0, -0.0, 1e-40, 1e-37, float('nan'))      # +0, -0, subnormal, tiny positive, NaN


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def _L():
    from ndcn_amd import _lib
    return _lib


class _Ws:
    ws = dots = None


def _scratch(dev):
    if _Ws.ws is None:
        _Ws.ws = torch.empty(int(_L().load().ndcn_rk_bwd_ws_bytes()), dtype=torch.uint8, device=dev)
        _Ws.dots = torch.zeros(8, dtype=torch.float64, device=dev)
    _Ws.dots.fill_(-7.0)
    return _Ws.ws, _Ws.dots


class _Empty:
    buf = None


def _addr(t):
    """the device address of t; an empty panel (torch reports 0) gets one inside a spare allocation at the same 16-byte phase, so
    n = 0 reaches the kernels with the pointers a caller would pass and the element path its offset selects"""
    if t.numel():
        return t.data_ptr()
    if _Empty.buf is None:
        _Empty.buf = torch.zeros(64, device=t.device)
    return _Empty.buf.data_ptr() + 4 * (t.storage_offset() % 4)


def _p(t):
    return None if t is None else ctypes.c_void_p(_addr(t))


def _pa(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else _addr(t) for t in ts])


def _fa(cs):
    return (ctypes.c_float * len(cs))(*[float(c) for c in cs])


def _ok(rc):
    L = _L()
    assert rc == 0, (rc, L.load().ndcn_last_error())


def _route():
    v = int(_L().load().ndcn_debug_last_rk_bwd_path())
    return v & 0xffff, v >> 16


def _expect(kernel, n, vec, cap=CAP):
    items = n // 4 if vec else n
    grid = max(1, min(-(-items // 256), 2048, cap))
    got = _route()
    want = (kernel | (_L().RKB_VEC if vec else 0), grid)
    assert got == want, (got, want)
    return grid


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------------------ inputs
def _panel(n, gen, dev, k=6, zero_every=13):
    """randn, each element times 2^j (j uniform in [-k, k]); every zero_every-th element +0 / -0"""
    x = torch.randn(n, generator=gen, device=dev) * torch.exp2(torch.randint(-k, k + 1, (n,), generator=gen, device=dev).float())
    if zero_every:
        x[::zero_every] = 0.0
        x[zero_every // 2::2 * zero_every] = -0.0
    return x


def _view(x):
    """the same values at a 4-byte offset from a 16-byte-aligned allocation: the scalar element path"""
    v = torch.empty(x.numel() + 1, device=x.device)[1:]
    v.copy_(x)
    assert _addr(v) % 16 == 4
    return v


def _within(got, ref, bound, what, nan_match=True):
    got = got.double()
    gn, rn = torch.isnan(got), torch.isnan(ref)
    if nan_match:
        assert torch.equal(gn, rn), '%s: NaN positions differ (%d vs %d)' % (what, int(gn.sum()), int(rn.sum()))
    err = (got - ref).abs()
    bad = ~(err <= bound) & ~rn
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        pytest.fail('%s: %d elements out of bound; first flat %d: got %r ref %r bound %r' % (
            what, int(bad.sum()), i, float(got.flatten()[i]), float(ref.flatten()[i]), float(bound.flatten()[i])))


def _within_s(got, ref, bound, what):
    import math
    if math.isnan(ref):
        assert math.isnan(got), (what, got, ref)
        return
    assert abs(got - ref) <= bound, (what, got, ref, bound)


# element-path cases: (n, mode): 'vec' (n % 4 == 0, aligned), 'view' (n % 4 == 0, one input 4 bytes off), 'scalar' (n % 4 != 0)
EDGE = CAP * 256
PATH_CASES = ([(0, 'vec'), (0, 'view'), (1, 'scalar'), (3, 'scalar'), (4, 'vec'), (4, 'view'), (5, 'scalar'), (1023, 'scalar')] +
              [(4 * (EDGE + d), m) for d in (-1, 1) for m in ('vec', 'view')] + [(EDGE + d, 'scalar') for d in (-1, 1)])
DENSE_EDGE = 2048 * 256
DENSE_CASES = [0, 1, 3, 4, 5, 1023, DENSE_EDGE - 1, DENSE_EDGE + 1]


def test_path_cases_reach_the_loop_edges():
    """the sizes above run the grid-stride loop exactly once (last item of a full grid) and twice (one item over), per element path"""
    for n, m in PATH_CASES:
        items = n // 4 if m != 'scalar' else n
        assert m == 'scalar' or n % 4 == 0
        if items > CAP * 256 - 2:
            assert -(-items // 256) in (CAP, CAP + 1)
    assert {n for n, m in PATH_CASES if m == 'vec'} >= {4 * (EDGE - 1), 4 * (EDGE + 1)}


# ------------------------------------------------------------------------------------------------------------------------ combine
def _combine(g, ks, cs, gk, accs=None, gy0=None, acc_y0=None):
    ws, dots = _scratch(g.device)
    _ok(_L().load().ndcn_rk_combine_bwd_f32(_p(g), _pa(ks), _fa(cs), len(ks), _pa(gk), _pa(accs) if accs else None, _p(gy0), _p(acc_y0),
                                            _p(dots), _p(ws), g.numel(), _stream()))
    return dots.cpu().tolist(), _route()


def _check_combine(g, ks, cs, gk, accs, gy0, acc_y0, dots, what):
    gd = g.double()
    for j, (k, c) in enumerate(zip(ks, cs)):
        cg = c * gd
        if gk[j] is not None:
            a = accs[j].double() if accs and accs[j] is not None else None
            if a is None:
                _within(gk[j], cg, U * cg.abs(), '%s gk%d' % (what, j))
            else:
                _within(gk[j], a + cg, 2.01 * U * (a.abs() + cg.abs()), '%s gk%d+acc' % (what, j))
        pr = gd * k.double()
        _within_s(dots[j], float(pr.sum()), 1.01 * (U + g.numel() * E53) * float(pr.abs().sum()), '%s dot%d' % (what, j))
    if gy0 is not None:
        a = acc_y0.double()
        _within(gy0, a + gd, U * (a.abs() + gd.abs()), what + ' gy0')


def _combine_inputs(n, nk, seed, dev, mode):
    gen = torch.Generator(device=dev).manual_seed(seed)
    g = _panel(n, gen, dev)
    ks = [_panel(n, gen, dev, zero_every=7 + j) for j in range(nk)]
    accs = [_panel(n, gen, dev) for _ in range(nk)]
    acc_y0 = _panel(n, gen, dev)
    cs = [F32(0.37 * (-1) ** j / (j + 1)) for j in range(nk)]
    if mode == 'view':
        ks[nk - 1] = _view(ks[nk - 1])
    return g, ks, cs, accs, acc_y0


@pytest.mark.parametrize('n,mode', PATH_CASES)
def test_combine_bwd_paths(dev, n, mode):
    g, ks, cs, accs, acc_y0 = _combine_inputs(n, 3, n + 1, dev, mode)
    for with_acc in (False, True):
        gk = [torch.empty_like(g) for _ in ks]
        gy0 = torch.empty_like(g) if with_acc else None
        dots, _ = _combine(g, ks, cs, gk, accs if with_acc else None, gy0, acc_y0 if with_acc else None)
        _expect(_L().RKB_COMBINE, n, mode == 'vec')
        _check_combine(g, ks, cs, gk, accs if with_acc else None, gy0, acc_y0 if with_acc else None, dots, 'combine n=%d' % n)
        gk2 = [torch.empty_like(g) for _ in ks]
        gy02 = torch.empty_like(g) if with_acc else None
        dots2, _ = _combine(g, ks, cs, gk2, accs if with_acc else None, gy02, acc_y0 if with_acc else None)
        assert dots2 == dots and all(torch.equal(a, b) for a, b in zip(gk, gk2)) and (not with_acc or torch.equal(gy0, gy02))


@pytest.mark.parametrize('nk', range(1, 9))
@pytest.mark.parametrize('n,mode', [(1021, 'scalar'), (1024, 'vec'), (1024, 'view')])
def test_combine_bwd_terms_subsets_and_aliasing(dev, n, mode, nk):
    """n_k = 1..8 (kBwdMaxK); every subset of requested gk (n_k <= 4), acc given or not per term; gk aliasing its acc gives the bits of
    the call that writes elsewhere"""
    g, ks, cs, accs, acc_y0 = _combine_inputs(n, nk, 100 * nk + n, dev, mode)
    full = [torch.empty_like(g) for _ in ks]
    dots, _ = _combine(g, ks, cs, full, accs)
    _expect(_L().RKB_COMBINE, n, mode == 'vec')
    _check_combine(g, ks, cs, full, accs, None, None, dots, 'combine nk=%d' % nk)
    subsets = range(1 << nk) if nk <= 4 else [0, (1 << nk) - 1, 0b10101010 & ((1 << nk) - 1)]
    for s in subsets:
        gk = [torch.empty_like(g) if s >> j & 1 else None for j in range(nk)]
        sub_acc = [accs[j] if j % 2 else None for j in range(nk)]
        d2, _ = _combine(g, ks, cs, gk, sub_acc)
        _expect(_L().RKB_COMBINE, n, mode == 'vec')
        assert d2 == dots, s
        _check_combine(g, ks, cs, gk, sub_acc, None, None, d2, 'combine subset %d' % s)
        for j in range(nk):
            if gk[j] is not None and sub_acc[j] is not None:
                assert torch.equal(gk[j], full[j]), (s, j)
    alias = [a.clone() for a in accs]
    d3, _ = _combine(g, ks, cs, alias, alias)
    y0a = acc_y0.clone()
    d4, _ = _combine(g, ks, cs, [None] * nk, None, y0a, y0a)
    gy0 = torch.empty_like(g)
    _combine(g, ks, cs, [None] * nk, None, gy0, acc_y0)
    assert d3 == dots and d4 == dots and all(torch.equal(a, b) for a, b in zip(alias, full)) and torch.equal(y0a, gy0)


# ------------------------------------------------------------------------------------------------------------------------ pull
def _pull(out, base, ps, cs, mask, ua, ub):
    ws, dots = _scratch(out.device)
    _ok(_L().load().ndcn_rk_pull_f32(_p(out), _p(base), _pa(ps), _fa(cs), len(ps), _p(mask), _p(ua), _p(ub), _p(dots), _p(ws), out.numel(),
                                     _stream()))
    return dots.cpu().tolist()[0], _route()


def _pull_ref32(base, ps, cs, mask):
    """the pull's documented arithmetic as fp32 torch ops on the device: ((c_0 p_0 + c_1 p_1) + ...), then base +, then threshold_backward's
    mask; the same bits as ndcn_rk_combine_f32 (y0 = base, nullable) on the same panels, and within its bound of fp64"""
    c = lambda v: torch.tensor(v, dtype=torch.float32, device=ps[0].device)
    s = ps[0] * c(cs[0])
    for p, cj in zip(ps[1:], cs[1:]):
        s = s + p * c(cj)
    if base is not None:
        s = base + s
    if s.numel():
        comb = torch.empty_like(s)
        _ok(_L().load().ndcn_rk_combine_f32(_p(comb), _p(base), _pa(ps), _fa(cs), len(ps), s.numel(), _stream()))
        assert torch.equal(comb, s)
        ref = sum(c * p.double() for c, p in zip(cs, ps)) + (base.double() if base is not None else 0.0)
        mag = sum(abs(c) * p.double().abs() for c, p in zip(cs, ps)) + (base.double().abs() if base is not None else 0.0)
        _within(s, ref, 1.01 * (len(ps) + 1) * U * mag, 'combine / pull arithmetic')
    if mask is not None:
        s = torch.where((mask.cpu() <= 0).to(s.device), torch.zeros_like(s), s)    # on the CPU: a subnormal compares as itself
    return s


def _relu_mask(n, gen, dev):
    """a ReLU output with SPECIALS[q] at every element 7 (5 r + q) + 3"""
    m = torch.relu(torch.randn(n, generator=gen, device=dev))
    for q, v in enumerate(SPECIALS):
        m[7 * q + 3::35] = v
    return m


def _pull_case(n, nk, seed, dev, mode, use):
    gen = torch.Generator(device=dev).manual_seed(seed)
    ps = [_panel(n, gen, dev, zero_every=5 + j) for j in range(nk)]
    base, ua, ub = (_panel(n, gen, dev) for _ in range(3))
    mask = _relu_mask(n, gen, dev)
    cs = [F32(0.3 + 0.1 * j) * (-1) ** j for j in range(nk)]
    if mode == 'view':
        mask = _view(mask)
    base, mask, ua, ub = (t if u else None for t, u in zip((base, mask, ua, ub), use))
    if mode == 'view' and mask is None:
        ps[0] = _view(ps[0])
    out = torch.empty_like(ps[0])
    d, route = _pull(out, base, ps, cs, mask, ua, ub)
    if n == 0:
        assert route == (0, 0)
    else:
        _expect(_L().RKB_PULL, n, mode == 'vec')
    assert torch.equal(out, _pull_ref32(base, ps, cs, mask)), 'pull bits n=%d use=%s' % (n, use)
    if ua is not None:
        e = ua.double() - (ub.double() if ub is not None else 0.0)
        mag = ps[0].double().abs() * (ua.double().abs() + (ub.double().abs() if ub is not None else 0.0))
        _within_s(d, float((ps[0].double() * e).sum()), 1.01 * (2 * U + n * E53) * float(mag.sum()), 'pull dot n=%d' % n)
    out2 = torch.empty_like(out)
    d2, _ = _pull(out2, base, ps, cs, mask, ua, ub)
    assert torch.equal(out, out2) and (ua is None or d2 == d)
    return out, d


@pytest.mark.parametrize('n,mode', PATH_CASES)
def test_pull_paths(dev, n, mode):
    """every input given; the mask threads +0, -0, a subnormal, a tiny positive value and NaN through both element paths"""
    _pull_case(n, 3, n + 3, dev, mode, (True, True, True, True))


@pytest.mark.parametrize('nk', range(1, 9))
@pytest.mark.parametrize('n,mode', [(1021, 'scalar'), (1024, 'vec'), (1024, 'view')])
def test_pull_terms_and_optional_inputs(dev, n, mode, nk):
    """n_p = 1..8; each subset of (base, mask, ua, ub) (ub only with ua); VEC and scalar paths give the same bits on the same data"""
    for use in [(b, m, a, a and bb) for b in (0, 1) for m in (0, 1) for a in (0, 1) for bb in (0, 1) if a or not bb]:
        out, _ = _pull_case(n, nk, 7 * nk + n, dev, mode, use)
        if mode == 'view':
            ref, _ = _pull_case(n, nk, 7 * nk + n, dev, 'vec', use)
            assert torch.equal(out, ref)


def test_pull_mask_is_threshold_backward(dev):
    """mask = +0, -0 stop the gradient; a subnormal, a tiny positive value and NaN pass it - VEC and scalar alike"""
    n = 4 * 65
    for mode in ('vec', 'view'):
        p = torch.ones(n, device=dev)
        mask = torch.tensor(SPECIALS * (n // 5), device=dev)
        if mode == 'view':
            mask = _view(mask)
        out = torch.empty_like(p)
        _pull(out, None, [p], [1.0], mask, None, None)
        _expect(_L().RKB_PULL, n, mode == 'vec')
        assert out.view(-1, 5)[:, :2].eq(0).all() and out.view(-1, 5)[:, 2:].eq(1).all(), mode
        from ndcn_amd import hip
        o2, d = hip.pull([p], [1.0], mask=mask, ua=p)                 # the ops wrapper: same launch, same bits
        _expect(_L().RKB_PULL, n, mode == 'vec')
        assert torch.equal(o2, out) and d == float(n)


# ------------------------------------------------------------------------------------------------------------------------ dot_diff
@pytest.mark.parametrize('n,mode', PATH_CASES)
def test_dot_diff_paths(dev, n, mode):
    gen = torch.Generator(device=dev).manual_seed(n + 11)
    g, a, b = (_panel(n, gen, dev) for _ in range(3))
    if mode == 'view':
        b = _view(b)
    ws, dots = _scratch(dev)
    for bb in (b, None):
        if mode == 'view' and bb is None:
            a = _view(a)
        res = []
        for _ in range(2):
            ws, dots = _scratch(dev)
            _ok(_L().load().ndcn_rk_dot_diff_f32(_p(g), _p(a), _p(bb), _p(dots), _p(ws), n, _stream()))
            res.append(dots.cpu().tolist()[0])
            _expect(_L().RKB_DOT_DIFF, n, mode == 'vec')
        assert res[0] == res[1]
        e = a.double() - (bb.double() if bb is not None else 0.0)
        mag = g.double().abs() * (a.double().abs() + (bb.double().abs() if bb is not None else 0.0))
        _within_s(res[0], float((g.double() * e).sum()), 1.01 * (2 * U + n * E53) * float(mag.sum()), 'dot_diff n=%d' % n)


# ------------------------------------------------------------------------------------------------------------------------ error ratio
RTOL, ATOL, G_R = F32(1e-2), F32(1e-3), F32(0.7)


def _error(y0, y1, ks, cs, gy0, gy1, gk, accs=None, acc_y0=None, acc_y1=None, inv_n=None):
    ws, dots = _scratch(y0.device)
    n = y0.numel()
    _ok(_L().load().ndcn_rk_error_bwd_f32(_p(y0), _p(y1), _pa(ks), _fa(cs), len(ks), RTOL, ATOL, G_R, 1.0 / max(n, 1) if inv_n is None else inv_n,
                                          _p(gy0), _p(gy1), _pa(gk), _p(acc_y0), _p(acc_y1), _pa(accs) if accs else None, _p(dots), _p(ws),
                                          n, _stream()))
    return dots.cpu().tolist(), _route()


def _error_ref(y0, y1, ks, cs, n_total):
    """fp64 autograd through misc.py:146-157: mean(((sum c_j k_j) / (atol + rtol max(|y0|, |y1|)))^2), upstream g_r; plus the magnitudes"""
    kd = [k.double().requires_grad_(True) for k in ks]
    cd = [torch.tensor(c, dtype=torch.float64, device=y0.device, requires_grad=True) for c in cs]
    a0, a1 = y0.double().requires_grad_(True), y1.double().requires_grad_(True)
    e = sum(c * k for c, k in zip(cd, kd))
    r = e / (ATOL + RTOL * torch.max(a0.abs(), a1.abs()))
    ((r * r).sum() / n_total).backward(torch.tensor(G_R, dtype=torch.float64, device=y0.device))
    with torch.no_grad():
        E = sum(abs(c) * k.detach().abs() for c, k in zip(cs, kd))
        T = ATOL + RTOL * torch.max(y0.double().abs(), y1.double().abs())
        S = 2 * E / n_total / T ** 2
    return [k.grad for k in kd], [float(c.grad) / G_R for c in cd], a0.grad, a1.grad, E, T, S


def _check_error(y0, y1, ks, cs, gk, gy0, gy1, dots, accs, acc_y0, acc_y1, what):
    n, nk = y0.numel(), len(ks)
    rgk, rdots, rg0, rg1, E, T, S = _error_ref(y0, y1, ks, cs, max(n, 1))
    acc = lambda a: (a.double(), a.double().abs()) if a is not None else (0.0, 0.0)
    for j in range(nk):
        if gk[j] is not None:
            a, am = acc(accs[j] if accs else None)
            _within(gk[j], a + rgk[j], (nk + 12) * U * (abs(G_R * cs[j]) * S + am), '%s gk%d' % (what, j))
        _within_s(dots[j], rdots[j], 1.01 * ((nk + 9) * U + n * E53) * float((S * ks[j].double().abs()).nansum()), '%s dot%d' % (what, j))
    for got, ref, ac, name in ((gy0, rg0, acc_y0, 'gy0'), (gy1, rg1, acc_y1, 'gy1')):
        if got is not None:
            a, am = acc(ac)
            _within(got, a + ref, (2 * nk + 16) * U * (abs(G_R) * RTOL * (E / T) * S + am), '%s %s' % (what, name))


def _error_inputs(n, nk, seed, dev, mode, special=True):
    gen = torch.Generator(device=dev).manual_seed(seed)
    y0, y1 = _panel(n, gen, dev, zero_every=11), _panel(n, gen, dev, zero_every=11)
    if special and n:
        i = torch.arange(n, device=dev)
        y1[i % 5 == 1] = y0[i % 5 == 1]                     # |y0| == |y1|, same sign
        y1[i % 5 == 2] = -y0[i % 5 == 2]                    # y0 == -y1
        y0[i % 5 == 3] = 0.0                                # both zero (with the zeros every 11th)
        y1[i % 5 == 3] = -0.0
    ks = [_panel(n, gen, dev) for _ in range(nk)]
    accs = [_panel(n, gen, dev) for _ in range(nk)]
    acc_y0, acc_y1 = _panel(n, gen, dev), _panel(n, gen, dev)
    cs = [F32(0.1 * (j + 1) * (-1) ** j) for j in range(nk)]
    if mode == 'view':
        y1 = _view(y1)
    return y0, y1, ks, cs, accs, acc_y0, acc_y1


@pytest.mark.parametrize('n,mode', PATH_CASES)
def test_error_bwd_paths(dev, n, mode):
    """7 terms (dopri5's error estimate), exact ties |y0| == |y1| (also y0 == -y1, both zero), zeros in y; with and without acc"""
    y0, y1, ks, cs, accs, acc_y0, acc_y1 = _error_inputs(n, 7, n + 5, dev, mode)
    for with_acc in (False, True):
        gk = [torch.empty_like(y0) for _ in ks]
        gy0, gy1 = torch.empty_like(y0), torch.empty_like(y0)
        A = (accs, acc_y0, acc_y1) if with_acc else (None, None, None)
        dots, _ = _error(y0, y1, ks, cs, gy0, gy1, gk, *A)
        _expect(_L().RKB_ERROR, n, mode == 'vec')
        _check_error(y0, y1, ks, cs, gk, gy0, gy1, dots, *A, 'error n=%d acc=%d' % (n, with_acc))
        gk2 = [torch.empty_like(y0) for _ in ks]
        gy02, gy12 = torch.empty_like(y0), torch.empty_like(y0)
        dots2, _ = _error(y0, y1, ks, cs, gy02, gy12, gk2, *A)
        assert dots2[:7] == dots[:7] and torch.equal(gy0, gy02) and torch.equal(gy1, gy12)
        assert all(torch.equal(a, b) for a, b in zip(gk, gk2))


@pytest.mark.parametrize('nk', range(1, 9))
@pytest.mark.parametrize('n,mode', [(1021, 'scalar'), (1024, 'vec')])
def test_error_bwd_terms_and_subsets(dev, n, mode, nk):
    """n_k = 1..8; every subset of (gy0, gy1, gk) with acc given or not; gk / gy aliasing their acc"""
    y0, y1, ks, cs, accs, acc_y0, acc_y1 = _error_inputs(n, nk, 31 * nk + n, dev, mode)
    for need in range(8):
        for with_acc in (False, True):
            gk = [torch.empty_like(y0) if need & 4 else None for _ in ks]
            gy0 = torch.empty_like(y0) if need & 1 else None
            gy1 = torch.empty_like(y0) if need & 2 else None
            A = (accs, acc_y0, acc_y1) if with_acc else (None, None, None)
            dots, _ = _error(y0, y1, ks, cs, gy0, gy1, gk, *A)
            _expect(_L().RKB_ERROR, n, mode == 'vec')
            _check_error(y0, y1, ks, cs, gk, gy0, gy1, dots, *A, 'error need=%d' % need)
    gk = [torch.empty_like(y0) for _ in ks]
    gy0, gy1 = torch.empty_like(y0), torch.empty_like(y0)
    dots, _ = _error(y0, y1, ks, cs, gy0, gy1, gk, accs, acc_y0, acc_y1)
    al = [a.clone() for a in accs]
    a0, a1 = acc_y0.clone(), acc_y1.clone()
    d2, _ = _error(y0, y1, ks, cs, a0, a1, al, al, a0, a1)
    assert d2[:nk] == dots[:nk] and torch.equal(a0, gy0) and torch.equal(a1, gy1) and all(torch.equal(a, b) for a, b in zip(al, gk))


@pytest.mark.parametrize('mode', ['scalar', 'vec'])
def test_error_bwd_nan_in_y0(dev, mode):
    """a NaN in y0: the gradients of that element and every d_j are NaN, as in the reference; the finite elements meet the bound"""
    n = 4096 if mode == 'vec' else 4095
    y0, y1, ks, cs, accs, acc_y0, acc_y1 = _error_inputs(n, 7, 77, dev, mode)
    y0[[5, 100, 2001]] = float('nan')
    gk = [torch.empty_like(y0) for _ in ks]
    gy0, gy1 = torch.empty_like(y0), torch.empty_like(y0)
    dots, _ = _error(y0, y1, ks, cs, gy0, gy1, gk, accs, acc_y0, acc_y1)
    _expect(_L().RKB_ERROR, n, mode == 'vec')
    _check_error(y0, y1, ks, cs, gk, gy0, gy1, dots, accs, acc_y0, acc_y1, 'error NaN')
    assert int(torch.isnan(gy0).sum()) == 3 and int(torch.isnan(gy1).sum()) == 3


# ------------------------------------------------------------------------------------------------------------------------ rms
def _rms(a, b, y, coef, ga, gb, gy):
    _ok(_L().load().ndcn_rk_rms_bwd_f32(_p(a), _p(b), _p(y), RTOL, ATOL, coef, _p(ga), _p(gb), _p(gy), a.numel(), _stream()))
    return _route()


def _rms_ref(a, b, y, g_o, same_ay=False):
    """fp64 autograd through misc.py:71-76: ||(a - b) / (atol + |y| rtol)|| / sqrt(N), upstream g_o; coef = g_o / (||.|| sqrt(N)) in fp32"""
    ad = a.double().requires_grad_(True)
    bd = b.double().requires_grad_(True) if b is not None else None
    yd = ad if same_ay else y.double().requires_grad_(True)
    scale = ATOL + yd.abs() * RTOL
    v = ((ad - bd) if bd is not None else ad) / scale
    nrm = v.norm()
    (nrm / v.numel() ** 0.5).backward(torch.tensor(g_o, dtype=torch.float64, device=a.device))
    coef = F32(g_o / (float(nrm) * v.numel() ** 0.5))
    with torch.no_grad():
        sc = ATOL + y.double().abs() * RTOL
        V = (a.double().abs() + (b.double().abs() if b is not None else 0.0)) / sc
        # the kernel's coef is fl32 of the exact one: one more rounding on every output
        bga = 9 * U * abs(coef) * V / sc
        bgy = 17 * U * abs(coef) * V * V * RTOL / sc
    return coef, ad.grad, (bd.grad if bd is not None else None), (None if same_ay else yd.grad), bga, bgy


@pytest.mark.parametrize('n', DENSE_CASES)
def test_rms_bwd(dev, n):
    """with and without b, every subset of outputs, zeros and a NaN in y, a == y (tape.hip: the norm of y0 itself), a view"""
    if n == 0:
        e = torch.empty(0, device=dev)
        _rms(e, e, e, 1.0, e, e, e)
        assert _route() == (_L().RKB_RMS, 1)
        _expect(_L().RKB_RMS, 0, False, 2048)
        return
    gen = torch.Generator(device=dev).manual_seed(n + 9)
    a, b, y = _panel(n, gen, dev, zero_every=0), _panel(n, gen, dev, zero_every=0), _panel(n, gen, dev, zero_every=3)
    for has_b in (True, False):
        bb = b if has_b else None
        coef, ra, rb, ry, bga, bgy = _rms_ref(a, bb, y, 1.3)
        outs = [torch.empty_like(a) for _ in range(3)]
        _rms(a, bb, y, coef, outs[0], outs[1] if has_b else None, outs[2])
        _expect(_L().RKB_RMS, n, False, 2048)
        _within(outs[0], ra, bga, 'rms ga')
        _within(outs[2], ry, bgy, 'rms gy')
        if has_b:
            _within(outs[1], rb, bga, 'rms gb')
        for need in range(8):
            o = [torch.empty_like(a) if need >> i & 1 and (i != 1 or has_b) else None for i in range(3)]
            _rms(a, bb, y, coef, *o)
            for got, full in zip(o, outs):
                assert got is None or torch.equal(got, full), need
        if n % 4 == 0:
            o = [torch.empty_like(a), torch.empty_like(a) if has_b else None, torch.empty_like(a)]
            _rms(_view(a), bb, y, coef, *o)
            assert all(x is None or torch.equal(x, z) for x, z in zip(o, outs))
    # a IS y (tape.hip: rms_bwd(y_in, nullptr, y_in)): the caller adds ga and gy - their sum against the one-leaf autograd
    y = y.clone()
    y[0] = 1.5                                              # (n = 1: a nonzero norm)
    coef, ra, _, _, bga, bgy = _rms_ref(y, None, y, 0.9, same_ay=True)
    ga, gy = torch.empty_like(y), torch.empty_like(y)
    _rms(y, None, y, coef, ga, None, gy)
    _within(ga + gy, ra, bga + bgy + U * (ga.double().abs() + gy.double().abs()), 'rms a=y')
    yn = y.clone()
    if n > 7:
        yn[[3, 7]] = float('nan')
        coef_nan = F32(0.25)
        ga = torch.empty_like(y)
        _rms(a, b, yn, coef_nan, ga, None, None)
        assert bool(torch.isnan(ga[[3, 7]]).all()) and int(torch.isnan(ga).sum()) == 2


# ------------------------------------------------------------------------------------------------------------------------ dense output
def _cmid():
    from ndcn_amd.torchdiffeq._impl import core
    return [float(c) for c in core.DP_C_MID]


def _dense_ref(g_list, y0, y1, ks, dt, xs):
    """fp64 autograd through interp.py:21-65 / dopri5.py:39-45 summed over ticks: (gy0, gy1, gk, [d/dx_t], d/ddt) and the magnitudes"""
    cm = _cmid()
    dev = y0.device
    kd = [k.double().requires_grad_(True) for k in ks]
    a0, a1 = y0.double().requires_grad_(True), y1.double().requires_grad_(True)
    dtd = torch.tensor(dt, dtype=torch.float64, device=dev, requires_grad=True)
    xds = [torch.tensor(x, dtype=torch.float64, device=dev, requires_grad=True) for x in xs]
    ym = a0 + sum((dtd * c) * k for k, c in zip(kd, cm))
    f0, f1 = kd[0], kd[6]
    ca = (-2 * dtd) * f0 + (2 * dtd) * f1 + -8 * a0 + -8 * a1 + 16 * ym
    cb = (5 * dtd) * f0 + (-3 * dtd) * f1 + 18 * a0 + 14 * a1 + -32 * ym
    cc = (-4 * dtd) * f0 + dtd * f1 + -11 * a0 + -5 * a1 + 16 * ym
    loss = 0
    for g, xd in zip(g_list, xds):
        o = ca * xd ** 4 + cb * xd ** 3 + cc * xd ** 2 + (dtd * f0) * xd + a0
        loss = loss + (o * g.double()).sum()
    loss.backward()
    with torch.no_grad():
        ad, Y0, Y1 = abs(dt), y0.double().abs(), y1.double().abs()
        K = [k.double().abs() for k in ks]
        sc = sum(abs(c) * k for c, k in zip(cm, K))
        ymb = Y0 + ad * sc
        Ca = 2 * ad * (K[6] + K[0]) + 8 * Y0 + 8 * Y1 + 16 * ymb
        Cb = ad * (5 * K[0] + 3 * K[6]) + 18 * Y0 + 14 * Y1 + 32 * ymb
        Cc = ad * (K[6] + 4 * K[0]) + 11 * Y0 + 5 * Y1 + 16 * ymb
        Wy0 = Wy1 = 0.0
        Wk = [0.0] * 7
        mx, mdt = [], 0.0
        for g, x in zip(g_list, xs):
            G, a = g.double().abs(), abs(x)
            wym = 16 * a ** 4 + 32 * a ** 3 + 16 * a ** 2
            Wy0 = Wy0 + (8 * a ** 4 + 18 * a ** 3 + 11 * a ** 2 + 1 + wym) * G
            Wy1 = Wy1 + (8 * a ** 4 + 14 * a ** 3 + 5 * a ** 2) * G
            for j in range(7):
                w = wym * ad * abs(cm[j]) + (ad * (2 * a ** 4 + 5 * a ** 3 + 4 * a ** 2 + a) if j == 0 else 0.0) + \
                    (ad * (2 * a ** 4 + 3 * a ** 3 + a ** 2) if j == 6 else 0.0)
                Wk[j] = Wk[j] + w * G
            mx.append(float((G * (4 * Ca * a ** 3 + 3 * Cb * a ** 2 + 2 * Cc * a + ad * K[0])).sum()))
            mdt += float((G * (a ** 4 * (2 * (K[6] + K[0]) + 16 * sc) + a ** 3 * (5 * K[0] + 3 * K[6] + 32 * sc) +
                               a ** 2 * (K[6] + 4 * K[0] + 16 * sc) + a * K[0])).sum())
    return (a0.grad, a1.grad, [k.grad for k in kd], [float(x.grad) for x in xds], float(dtd.grad)), (Wy0, Wy1, Wk, mx, mdt)


def _check_dense(ref, mag, outs, dots_x, dot_dt, accs, acc_y0, acc_y1, nt, n, what):
    (r0, r1, rk, rx, rdt), (W0, W1, Wk, mx, mdt) = ref, mag
    f = (16 + (3 * nt if nt > 1 else 0)) * U
    acc = lambda a: (a.double(), a.double().abs()) if a is not None else (0.0, 0.0)
    gy0, gy1, gk = outs
    for got, r, W, ac, name in ((gy0, r0, W0, acc_y0, 'gy0'), (gy1, r1, W1, acc_y1, 'gy1')):
        if got is not None:
            a, am = acc(ac)
            _within(got, a + r, f * (W + am), '%s %s' % (what, name))
    for j in range(7):
        if gk[j] is not None:
            a, am = acc(accs[j] if accs else None)
            _within(gk[j], a + rk[j], f * (Wk[j] + am), '%s gk%d' % (what, j))
    for t in range(nt):
        _within_s(dots_x[t], rx[t], 1.01 * (32 * U + n * E53) * mx[t], '%s d/dx%d' % (what, t))
    _within_s(dot_dt, rdt, 1.01 * (32 * U + n * nt * E53) * mdt, what + ' d/ddt')


def _dense_inputs(n, seed, dev, nt=1):
    gen = torch.Generator(device=dev).manual_seed(seed)
    gs = [_panel(n, gen, dev) for _ in range(nt)]
    y0, y1 = _panel(n, gen, dev), _panel(n, gen, dev)
    ks = [_panel(n, gen, dev, zero_every=9 + j) for j in range(7)]
    accs = [_panel(n, gen, dev) for _ in range(7)]
    return gs, y0, y1, ks, accs, _panel(n, gen, dev), _panel(n, gen, dev)


def _dense(g, y0, y1, ks, dt, x, gy0, gy1, gk, accs=None, acc_y0=None, acc_y1=None):
    ws, dots = _scratch(y0.device)
    _ok(_L().load().ndcn_dopri5_interp_bwd_f32(_p(g), _p(y0), _p(y1), _pa(ks), dt, x, _p(gy0), _p(gy1), _pa(gk), _p(acc_y0), _p(acc_y1),
                                               _pa(accs) if accs else None, _p(dots), _p(ws), y0.numel(), _stream()))
    return dots.cpu().tolist()


def _dense_multi(gs, y0, y1, ks, dt, xs, gy0, gy1, gk, accs=None, acc_y0=None, acc_y1=None):
    ws, dots = _scratch(y0.device)
    _ok(_L().load().ndcn_dopri5_interp_bwd_multi_f32(_pa(gs), len(gs), _p(y0), _p(y1), _pa(ks), dt, _fa(xs), _p(gy0), _p(gy1), _pa(gk),
                                                     _p(acc_y0), _p(acc_y1), _pa(accs) if accs else None, _p(dots), _p(ws), y0.numel(),
                                                     _stream()))
    return dots.cpu().tolist()


XS = [0.0, 1.0, 0.5, F32(0.6180339887)]


@pytest.mark.parametrize('n', DENSE_CASES)
@pytest.mark.parametrize('dt', [F32(0.37), F32(-0.125)])
def test_dense_bwd(dev, n, dt):
    """x in {0, 1, 0.5, random}, dt > 0 and dt < 0 (a decreasing grid), acc given or not, every subset of outputs, a view"""
    gs, y0, y1, ks, accs, acc_y0, acc_y1 = _dense_inputs(n, n + 13, dev)
    for x in XS:
        ref, mag = _dense_ref(gs, y0, y1, ks, dt, [x])
        for with_acc in (False, True):
            outs = (torch.empty_like(y0), torch.empty_like(y0), [torch.empty_like(y0) for _ in range(7)])
            A = (accs, acc_y0, acc_y1) if with_acc else (None, None, None)
            d = _dense(gs[0], y0, y1, ks, dt, x, *outs, *A)
            _expect(_L().RKB_DENSE, n, False, 2048)
            _check_dense(ref, mag, outs, d[:1], d[1], *A, 1, n, 'dense n=%d x=%r acc=%d' % (n, x, with_acc))
            o2 = (torch.empty_like(y0), torch.empty_like(y0), [torch.empty_like(y0) for _ in range(7)])
            d2 = _dense(gs[0], y0, y1, ks, dt, x, *o2, *A)
            assert d2[:2] == d[:2] and torch.equal(o2[0], outs[0]) and torch.equal(o2[1], outs[1])
            assert all(torch.equal(a, b) for a, b in zip(o2[2], outs[2]))
            if with_acc and x == XS[-1]:
                for need in range(8):
                    o = (torch.empty_like(y0) if need & 1 else None, torch.empty_like(y0) if need & 2 else None,
                         [torch.empty_like(y0) if need & 4 and j % 3 else None for j in range(7)])
                    d3 = _dense(gs[0], y0, y1, ks, dt, x, *o, *A)
                    assert d3[:2] == d[:2]
                    assert (o[0] is None or torch.equal(o[0], outs[0])) and (o[1] is None or torch.equal(o[1], outs[1]))
                    assert all(a is None or torch.equal(a, b) for a, b in zip(o[2], outs[2]))
                al, a0, a1 = [a.clone() for a in accs], acc_y0.clone(), acc_y1.clone()
                _dense(gs[0], y0, y1, ks, dt, x, a0, a1, al, al, a0, a1)
                assert torch.equal(a0, outs[0]) and torch.equal(a1, outs[1]) and all(torch.equal(a, b) for a, b in zip(al, outs[2]))
                if n % 4 == 0 and n:
                    o = (torch.empty_like(y0), torch.empty_like(y0), [torch.empty_like(y0) for _ in range(7)])
                    d4 = _dense(_view(gs[0]), y0, _view(y1), ks, dt, x, *o, *A)
                    assert d4[:2] == d[:2] and torch.equal(o[0], outs[0]) and all(torch.equal(a, b) for a, b in zip(o[2], outs[2]))


@pytest.mark.parametrize('nt', range(1, 8))
@pytest.mark.parametrize('n', [1023, DENSE_EDGE + 1])
def test_dense_bwd_multi(dev, n, nt):
    """nt = 1..7 ticks of one step, abscissae including 0, 1 and a repeated one; dt < 0 for odd nt; acc and aliasing"""
    gs, y0, y1, ks, accs, acc_y0, acc_y1 = _dense_inputs(n, 17 * nt + n, dev, nt)
    xs = ([0.0, 1.0, 0.5, F32(0.3), F32(0.3), F32(0.9), 0.5])[:nt][::-1]
    dt = F32(-0.21) if nt % 2 else F32(0.44)
    ref, mag = _dense_ref(gs, y0, y1, ks, dt, xs)
    for with_acc in (False, True):
        A = (accs, acc_y0, acc_y1) if with_acc else (None, None, None)
        outs = (torch.empty_like(y0), torch.empty_like(y0), [torch.empty_like(y0) for _ in range(7)])
        d = _dense_multi(gs, y0, y1, ks, dt, xs, *outs, *A)
        _expect(_L().RKB_DENSE_MULTI, n, False, 2048)
        _check_dense(ref, mag, outs, d[:nt], d[7], *A, nt, n, 'dense multi nt=%d acc=%d' % (nt, with_acc))
        o2 = (torch.empty_like(y0), torch.empty_like(y0), [torch.empty_like(y0) for _ in range(7)])
        assert _dense_multi(gs, y0, y1, ks, dt, xs, *o2, *A) == d
        assert torch.equal(o2[0], outs[0]) and torch.equal(o2[1], outs[1]) and all(torch.equal(a, b) for a, b in zip(o2[2], outs[2]))
    al, a0, a1 = [a.clone() for a in accs], acc_y0.clone(), acc_y1.clone()
    _dense_multi(gs, y0, y1, ks, dt, xs, a0, a1, al, al, a0, a1)
    assert torch.equal(a0, outs[0]) and torch.equal(a1, outs[1]) and all(torch.equal(a, b) for a, b in zip(al, outs[2]))
    for need in (1, 2, 4, 6):
        o = (torch.empty_like(y0) if need & 1 else None, torch.empty_like(y0) if need & 2 else None,
             [torch.empty_like(y0) if need & 4 and j % 2 else None for j in range(7)])
        assert _dense_multi(gs, y0, y1, ks, dt, xs, *o, *A) == d
        assert all(a is None or torch.equal(a, b) for a, b in zip(o[2], outs[2]))


# ------------------------------------------------------------------------------------------------------------------------ M-scale panel
def test_m_scale_panel(dev):
    """one 1M x 256 panel (2^28 elements): combine, pull, dot_diff and error on the VEC path (grid at its cap, 256 loop trips), the dense
    VJP on its 2048-block grid - elements and dots against fp64 in chunks"""
    n = (1 << 20) * 256
    gen = torch.Generator(device=dev).manual_seed(1 << 20)
    g, k0, k1, y1 = (_panel(n, gen, dev) for _ in range(4))
    cs = [F32(0.3), F32(-0.7)]
    C = 1 << 24
    # combine
    gk = [torch.empty_like(g), torch.empty_like(g)]
    dots, _ = _combine(g, [k0, k1], cs, gk, [None, y1])
    _expect(_L().RKB_COMBINE, n, True)
    assert _combine(g, [k0, k1], cs, [None, None])[0] == dots
    rd, md = [0.0, 0.0], [0.0, 0.0]
    for s in range(0, n, C):
        sl = slice(s, s + C)
        gd = g[sl].double()
        _within(gk[0][sl], cs[0] * gd, U * (cs[0] * gd).abs(), 'M gk0')
        a = y1[sl].double()
        _within(gk[1][sl], a + cs[1] * gd, 2.01 * U * (a.abs() + (cs[1] * gd).abs()), 'M gk1')
        for j, k in enumerate((k0, k1)):
            pr = gd * k[sl].double()
            rd[j] += float(pr.sum())
            md[j] += float(pr.abs().sum())
    for j in range(2):
        _within_s(dots[j], rd[j], 1.01 * (U + n * E53) * md[j], 'M combine dot%d' % j)
    del gk
    # pull (bits) and dot_diff
    out = torch.empty_like(g)
    d, _ = _pull(out, y1, [k0, k1], cs, g, k1, y1)
    _expect(_L().RKB_PULL, n, True)
    ws, dd = _scratch(dev)
    _ok(_L().load().ndcn_rk_dot_diff_f32(_p(k0), _p(k1), _p(y1), _p(dd), _p(ws), n, _stream()))
    _expect(_L().RKB_DOT_DIFF, n, True)
    d_diff = dd.cpu().tolist()[0]
    r, m = 0.0, 0.0
    for s in range(0, n, C):
        sl = slice(s, s + C)
        assert torch.equal(out[sl], _pull_ref32(y1[sl], [k0[sl], k1[sl]], cs, g[sl])), s
        e = k1[sl].double() - y1[sl].double()
        r += float((k0[sl].double() * e).sum())
        m += float((k0[sl].double().abs() * (k1[sl].double().abs() + y1[sl].double().abs())).sum())
    _within_s(d, r, 1.01 * (2 * U + n * E53) * m, 'M pull dot')
    _within_s(d_diff, r, 1.01 * (2 * U + n * E53) * m, 'M dot_diff')
    del out
    # error ratio over the whole panel: inv_n = 1 / n, checked in chunks
    gy0 = torch.empty_like(g)
    gke = [torch.empty_like(g), torch.empty_like(g)]
    ed, _ = _error(g, y1, [k0, k1], cs, gy0, None, gke)
    _expect(_L().RKB_ERROR, n, True)
    rsum = [0.0, 0.0]
    msum = [0.0, 0.0]
    for s in range(0, n, C):
        sl = slice(s, s + C)
        rgk, rdots, rg0, _, E, T, S = _error_ref(g[sl], y1[sl], [k0[sl], k1[sl]], cs, n)
        for j in range(2):
            _within(gke[j][sl], rgk[j], 14 * U * abs(G_R * cs[j]) * S, 'M error gk%d' % j)
            rsum[j] += rdots[j]
            msum[j] += float((S * (k0, k1)[j][sl].double().abs()).sum())
        _within(gy0[sl], rg0, 20 * U * abs(G_R) * RTOL * (E / T) * S, 'M error gy0')
    for j in range(2):
        _within_s(ed[j], rsum[j], 1.01 * (11 * U + n * E53) * msum[j], 'M error dot%d' % j)


# ------------------------------------------------------------------------------------------------------------------------ past 2^32 bytes
def test_combine_and_pull_beyond_4_gib(dev):
    """combine_bwd and pull on panels of 2^30 + 1024 (VEC, and scalar through a view) and 2^30 + 1023 elements (> 4 GiB each): the tail
    and a strided sample bit for bit against the fp32 torch expression at those positions, the dots against fp64 in chunks"""
    free, _ = torch.cuda.mem_get_info()
    assert free > 40 * 2 ** 30, 'needs ~40 GiB of device memory, %.1f GiB free' % (free / 2 ** 30)
    N = (1 << 30) + 1024
    gen = torch.Generator(device=dev).manual_seed(4096)
    gb = torch.randn(N + 4, generator=gen, device=dev)
    k0 = torch.randn(N, generator=gen, device=dev)
    k1 = torch.randn(N, generator=gen, device=dev) * 1e-3
    mask = _relu_mask(N, gen, dev)
    out = torch.empty(N, device=dev)
    cs = [F32(0.375), F32(-1.3)]
    C = 1 << 26
    for n, mode in ((N, 'vec'), (N, 'view'), (N - 1, 'scalar')):
        g = gb[1:n + 1] if mode == 'view' else gb[:n]
        ks = [k0[:n], k1[:n]]
        idx = torch.cat([torch.arange(0, n, 4099, device=dev), torch.arange(n - 4096, n, device=dev)])
        tail = torch.arange(n - 4096, n, device=dev)
        # combine: gk_0 = c_0 g (one rounding: bits), gk_1 into `out`
        gk0 = out[:n]
        dots, _ = _combine(g, ks, cs, [gk0, None])
        _expect(_L().RKB_COMBINE, n, mode == 'vec')
        assert torch.equal(gk0[idx], g[idx] * torch.tensor(cs[0], device=dev)), mode
        assert torch.equal(gk0[tail], g[tail] * torch.tensor(cs[0], device=dev)), mode
        for j in range(2):
            r = m = 0.0
            for s in range(0, n, C):
                pr = g[s:s + C].double() * ks[j][s:s + C].double()
                r += float(pr.sum())
                m += float(pr.abs().sum())
            _within_s(dots[j], r, 1.01 * (U + n * E53) * m, 'combine > 4 GiB %s dot%d' % (mode, j))
        # pull: out = mask ? g + (c0 k0 + c1 k1); dot <k0, g>
        po = out[:n]
        d, _ = _pull(po, g, ks, cs, mask[:n], g, None)
        _expect(_L().RKB_PULL, n, mode == 'vec')
        assert torch.equal(po[idx], _pull_ref32(g[idx], [k0[idx], k1[idx]], cs, mask[idx])), mode
        r = m = 0.0
        for s in range(0, n, C):
            pr = ks[0][s:s + C].double() * g[s:s + C].double()
            r += float(pr.sum())
            m += float(pr.abs().sum())
        _within_s(d, r, 1.01 * (2 * U + n * E53) * m, 'pull > 4 GiB %s' % mode)
    del gb, k0, k1, mask, out
    torch.cuda.empty_cache()
