"""Every forward solver panel kernel of rk.hip through the C ABI, at its size and order edges, each case asserting kernel, element path,
reduction route and grid through ndcn_debug_last_rk_path.

ORACLES (never the device, never a torch reduction):
  element-wise kernels   the reference's expression in numpy float32, every product, sum and quotient rounded on its own, Python's
                         sum() starting from 0 (misc.py:22-30): BIT equality, NaNs at the same positions (a NaN's payload and sign are
                         not compared: x86 and the GPU create different default NaNs), +0 and -0 told apart
  ATen-order reductions  tests/_aten_order.py (cascade_sum, lane8_fma_sumsq) of the host-formed float32 elements: d_out[0] BIT-equal
  parallel fp64 route    ref = float64 sum of the host-formed float32 elements (all >= 0): |got - ref| <= 1.01 n 2^-53 ref, the bound of
                         ANY summation tree of n non-negative terms (each of its <= n - 1 roundings is relative 2^-53 of a partial sum
                         <= the total); nothing in it is measured.  The reference itself is a pairwise float64 sum within the same bound.
  non-finite record      d_out[1] equals the planted count exactly on both routes

Sizes of the element-wise kernels: n in SIZES at the aligned phase; for n % 4 == 0 additionally with each operand in turn a view at a
float offset 1..3 into a larger allocation, which must report the scalar path and give the bits of the aligned call.  The 2^24-block
cap of stream_grid_full needs 64 GiB panels (2^24 blocks x 256 lanes x 16 bytes): left out.  One panel of 2^27 elements (grid 2^17
float4 blocks, beyond 16 bits) runs combine and copy.
The interp kernels drop terms whose h_cmid coefficient is zero (DPS_C_MID[1]; the header says so): with the dopri5 coefficients the
special values stay out of that stage's panel, and a second coefficient set without zeros plants them in all seven.

KERNEL TEMPLATE INSTANCES of rk.hip reachable through the C ABI, and the case that reaches each:
  combine_kernel<true / false>                 test_combine (aligned / n % 4 != 0 and every misaligned operand), test_combine_terms
  rk_error_aten_kernel                         test_aten_order_* , test_bound_selects_the_route, test_nonfinite_record
  rk_error_kernel<true / false>                test_parallel_route (aligned n % 4 == 0 / misaligned and n % 4 != 0), n < 8 of test_aten_order_every_small_n
  scaled_sumsq_aten_kernel<true / false>       test_aten_order_* (b given / NULL)     
  scaled_sumsq_kernel<true|false, true|false>  test_parallel_route (element path x b given / NULL)
  reduce_finish_kernel                         every parallel-route case
  interp_fit_kernel<true / false>              test_interp_fit
  interp_eval_kernel<true / false>             test_interp_eval (also e aliasing another input panel, as the header allows for y0)
  interp_direct_kernel<true / false>           test_interp_direct
  interp_direct_multi_kernel<true / false>     test_interp_direct_multi (n_t 1..7)
  fixed_stage_kernel<0..5, true / false>       test_fixed_stage (out == y included)
  tick_emit_kernel<true / false>               test_tick_emit (1, 8, 9, 17 ticks)
  fixed_stage_emit_kernel<0 | 5, true / false> test_fixed_stage_emit (out == y included)
  scale_kernel, copy_kernel, relu_bwd_kernel   test_scale_copy_relu_bwd
NOT reachable through the C ABI: scaled_sumsq_pair_kernel<true / false> (the initial step of the device-resident dopri5 solver:
tests/test_gpu_odeint.py), the dt_dev forms of combine / error / fixed_stage and scale_coef_kernel (the solver's captured hipGraph
replay: tests/test_gpu_odeint.py, tests/test_gpu_substep.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _aten_order as ao

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = [0, 1, 3, 4, 5, 7, 8, 1020, 1023, 1024, 1025, 1028, 256 * 4 * 3 + 4, 1000003]
INF, NAN = float('inf'), float('nan')
# +0, -0, a subnormal, values whose product / sum lands in the subnormal range, overflow to Inf, Inf, NaN
SPECIALS = [0.0, -0.0, 1e-40, -1e-40, 1e-20, -1.5e-19, 3e38, -3e38, INF, -INF, NAN]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def _L():
    from ndcn_amd import _lib
    return _lib


def _lib():
    return _L().load()


class _Empty:
    buf = None
    slot = 0


def _addr(t):
    """device address of t; an empty view gets one inside a spare allocation at the same 16-byte phase - a fresh 16-byte slot per
    request, so that the empty panels of one call are distinct (the tick entry points refuse a tick panel that aliases the state)"""
    if t.numel():
        return t.data_ptr()
    if _Empty.buf is None:
        _Empty.buf = torch.zeros(4 * 256, device=t.device)
    _Empty.slot = (_Empty.slot + 1) % 255
    return _Empty.buf.data_ptr() + 16 * _Empty.slot + 4 * (t.storage_offset() % 4)


def _p(t):
    return None if t is None else ctypes.c_void_p(_addr(t))


def _pa(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else _addr(t) for t in ts])


def _fa(cs):
    return (ctypes.c_float * len(cs))(*[float(c) for c in cs])


def _ia(v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc):
    assert rc == 0, (rc, _lib().ndcn_last_error())


def _einval(rc):
    assert rc == _L().EINVAL, rc
    assert _route() == 0


def _route():
    return int(_lib().ndcn_debug_last_rk_path())


def _expect(kernel, items, vec, op=0, extra=0, grid=None):
    """the reporter's word: kernel, op, element path, reduction bits, grid (default: one item per lane, 256 lanes per workgroup)"""
    L = _L()
    if grid is None:
        grid = max(1, -(-items // 256))
    want = kernel | (op << L.RKF_OP_SHIFT) | (L.RKF_VEC if vec else 0) | extra | (grid << L.RKF_GRID_SHIFT)
    got = _route()
    assert got == want, 'route %#x, expected %#x (kernel %d op %d vec %s extra %#x grid %d)' % (got, want, kernel, op, vec, extra, grid)


def _up(x, dev, off=0):
    """x (numpy float32) on the device as a view at float offset `off` (0..3) into a larger allocation"""
    x = np.ascontiguousarray(x, dtype=F)
    buf = torch.full((x.size + 8,), 7.0, device=dev)
    v = buf[off:off + x.size]
    if x.size:
        v.copy_(torch.from_numpy(x))
        assert v.data_ptr() % 16 == 4 * off
    return v


def _out(n, dev, off=0):
    return torch.full((n + 8,), -5.0, device=dev)[off:off + n]


def _np(t):
    return t.detach().cpu().numpy().copy()


def _same(got, ref, what):
    got, ref = np.asarray(got, F), np.asarray(ref, F)
    assert got.shape == ref.shape, what
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), '%s: NaN positions differ (%d vs %d), first at %s' % (what, gn.sum(), rn.sum(), np.nonzero(gn != rn)[0][:4])
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~rn
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        pytest.fail('%s: %d elements differ in bits; first %d: got %r (%#x) ref %r (%#x)' % (
            what, int(bad.sum()), i, float(got[i]), int(got.view(np.uint32)[i]), float(ref[i]), int(ref.view(np.uint32)[i])))


def _panels(n, count, seed, specials=True, skip=()):
    """`count` panels of randn times 2^j, j in [-6, 6]; SPECIALS at the first element, the last and both sides of the first float4
    boundary (3 | 4), a different one per panel and position; panels listed in `skip` stay finite and normal"""
    rs = np.random.default_rng(seed)
    out = []
    for j in range(count):
        x = (rs.standard_normal(n, dtype=F) * np.exp2(rs.integers(-6, 7, n)).astype(F)).astype(F)
        if specials and j not in skip:
            for q, pos in enumerate((0, n - 1, 3, 4)):
                if 0 <= pos < n:
                    x[pos] = F(SPECIALS[(3 * j + 5 * q + seed) % len(SPECIALS)])
        out.append(x)
    return out


def _phases(n, n_operands):
    """the aligned phase, then (n % 4 == 0) each operand in turn at a float offset 1..3"""
    yield None, [0] * n_operands
    if n % 4 == 0:
        for j in range(n_operands):
            offs = [0] * n_operands
            offs[j] = 1 + j % 3
            yield j, offs


def _elementwise(n, dev, host_in, n_out, call, oracle, kernel, what, op=0):
    """run `call(ins, outs)` at every phase; oracle(host_in) -> list of n_out arrays"""
    with np.errstate(all='ignore'):
        ref = oracle(*host_in)
    first = None
    for which, offs in _phases(n, len(host_in) + n_out):
        ins = [_up(x, dev, o) for x, o in zip(host_in, offs)]
        outs = [_out(n, dev, o) for o in offs[len(host_in):]]
        _ok(call(ins, outs))
        vec = n % 4 == 0 and which is None
        if n == 0:
            assert _route() == 0, what
        else:
            _expect(kernel, n // 4 if vec else n, vec, op)
        got = [_np(o) for o in outs]
        for g, r, i in zip(got, ref, range(n_out)):
            _same(g, r, '%s n=%d out%d misaligned=%s' % (what, n, i, which))
        if first is None:
            first = got
        else:
            for g, a in zip(got, first):
                _same(g, a, '%s n=%d scalar vs 16-byte path' % (what, n))


# ------------------------------------------------------------------------------------------------------------------ numpy oracles
def o_combine(y0, ks, cs):
    s = ao.wsum(ks, cs)
    return s if y0 is None else y0 + s


def o_fit(y0, y1, ks, cmid, dt):
    dt = F(dt)
    ms = ao.wsum(ks, cmid)
    ym = y0 + ms
    f0, f1 = ks[0], ks[6]
    a = ((((F(0) + (F(-2) * dt) * f0) + (F(2) * dt) * f1) + F(-8) * y0) + F(-8) * y1) + F(16) * ym
    b = ((((F(0) + (F(5) * dt) * f0) + (F(-3) * dt) * f1) + F(18) * y0) + F(14) * y1) + F(-32) * ym
    c = ((((F(0) + (F(-4) * dt) * f0) + dt * f1) + F(-11) * y0) + F(-5) * y1) + F(16) * ym
    d = dt * f0
    return [a, b, c, d]


def o_eval(a, b, c, d, e, xp):
    xp = [F(v) for v in xp]
    return ((((F(0) + a * xp[0]) + b * xp[1]) + c * xp[2]) + d * xp[3]) + e * xp[4]


def o_stage(op, y, k1, k2, k3, k4, dt):
    dt = F(dt)
    if op == 0:
        return y + dt * k1
    if op == 1:
        return y + k1 * dt / F(2)
    if op == 2:
        return y + dt * k1 / F(3)
    if op == 3:
        return y + dt * (k1 / F(-3) + k2)
    if op == 4:
        return y + dt * (k1 - k2 + k3)
    return y + (k1 + F(3) * k2 + F(3) * k3 + k4) * (dt / F(8))


def o_emit(v, dt, tm, same):
    return v.copy() if same else v + ((v - v) / F(dt)) * F(tm)


def _xp(x):
    x = F(x)
    return [F(x * x * x * x), F(x * x * x), F(x * x), x, F(1)]


def _cmids():
    """dt * DPS_C_MID rounded to fp32 (its second entry is 0: that stage is dropped), and a set without zeros"""
    from ndcn_amd.torchdiffeq._impl import core
    dt = F(0.37)
    real = [F(dt * F(c)) for c in core.DP_C_MID]
    assert real[1] == 0 and all(c != 0 for j, c in enumerate(real) if j != 1)
    dense = [F(0.11 * (j + 1) * (-1) ** j) for j in range(7)]
    return dt, (('dopri5', real, (3,)), ('no zero', dense, ()))          # panel 3 = ks[1] (after y0, y1, ks[0])


# ------------------------------------------------------------------------------------------------------------------ element-wise
@pytest.mark.parametrize('n', SIZES)
def test_combine(dev, n):
    """3 terms with and without y0; every operand (out, y0, each k) misaligned in turn"""
    cs = [F(0.37), F(-1.3), F(1e-3)]
    for with_y0 in (True, False):
        host = _panels(n, 4 if with_y0 else 3, n + 1)

        def call(ins, outs):
            y0 = ins[0] if with_y0 else None
            ks = ins[1:] if with_y0 else ins
            return _lib().ndcn_rk_combine_f32(_p(outs[0]), _p(y0), _pa(ks), _fa(cs), 3, n, _stream())
        oracle = (lambda y0, *ks: [o_combine(y0, ks, cs)]) if with_y0 else (lambda *ks: [o_combine(None, ks, cs)])
        _elementwise(n, dev, host, 1, call, oracle, _L().RKF_COMBINE, 'combine y0=%s' % with_y0)


@pytest.mark.parametrize('nk', range(1, 9))
def test_combine_terms(dev, nk):
    """n_k = 1..8 with and without y0 on both element paths; 0 terms, 9 terms and a null term are NDCN_EINVAL"""
    for n in (1023, 1024):
        host = _panels(n, nk + 1, 10 * nk + n)
        cs = [F(0.3 * (-1) ** j / (j + 1)) for j in range(nk)]
        d = [_up(x, dev) for x in host]
        for y0 in (d[0], None):
            out = _out(n, dev)
            _ok(_lib().ndcn_rk_combine_f32(_p(out), _p(y0), _pa(d[1:]), _fa(cs), nk, n, _stream()))
            _expect(_L().RKF_COMBINE, n // 4 if n % 4 == 0 else n, n % 4 == 0)
            with np.errstate(all='ignore'):
                _same(_np(out), o_combine(None if y0 is None else host[0], host[1:], cs), 'combine nk=%d n=%d' % (nk, n))
    if nk == 1:
        out = _out(n, dev)
        nine = [d[1]] * 9
        _einval(_lib().ndcn_rk_combine_f32(_p(out), _p(d[0]), _pa(nine), _fa([1.0] * 9), 0, n, _stream()))
        _einval(_lib().ndcn_rk_combine_f32(_p(out), _p(d[0]), _pa(nine), _fa([1.0] * 9), 9, n, _stream()))
        _einval(_lib().ndcn_rk_combine_f32(_p(out), _p(d[0]), _pa([d[1], None, d[1]]), _fa([1.0] * 3), 3, n, _stream()))


def test_combine_and_copy_on_a_panel_of_2_to_the_27(dev):
    """grid 2^17 float4 workgroups: beyond the 16 bits an int-packed reporter could hold"""
    n = 1 << 27
    host = _panels(n, 3, 27)
    cs = [F(0.25), F(-0.7)]
    d = [_up(x, dev) for x in host]
    out = _out(n, dev)
    _ok(_lib().ndcn_rk_combine_f32(_p(out), _p(d[0]), _pa(d[1:]), _fa(cs), 2, n, _stream()))
    _expect(_L().RKF_COMBINE, n // 4, True, grid=1 << 17)
    with np.errstate(all='ignore'):
        _same(_np(out), o_combine(host[0], host[1:], cs), 'combine 2^27')
    _ok(_lib().ndcn_copy_f32(_p(out), _p(d[1]), n, _stream()))
    _expect(_L().RKF_COPY, n // 4, True, grid=1 << 17)
    _same(_np(out), host[1], 'copy 2^27')


@pytest.mark.parametrize('n', SIZES)
def test_interp_fit(dev, n):
    dt, sets = _cmids()
    for name, cmid, skip in sets:
        host = _panels(n, 9, n + 2, skip=skip)

        def call(ins, outs):
            return _lib().ndcn_dopri5_interp_fit_f32(_p(ins[0]), _p(ins[1]), _pa(ins[2:]), _fa(cmid), dt, _p(outs[0]), _p(outs[1]),
                                                     _p(outs[2]), _p(outs[3]), n, _stream())
        keep = [j for j in range(7) if cmid[j] != 0]
        oracle = lambda y0, y1, *ks: o_fit(y0, y1, ks, cmid, dt) if len(keep) == 7 else _fit_dropped(y0, y1, ks, cmid, dt, keep)
        _elementwise(n, dev, host, 4, call, oracle, _L().RKF_INTERP_FIT, 'interp_fit ' + name)


def _fit_dropped(y0, y1, ks, cmid, dt, keep):
    """the terms with a zero coefficient are not formed (ndcn_hip.h); f0, f1 stay stages 0 and 6"""
    dtf = F(dt)
    ym = y0 + ao.wsum([ks[j] for j in keep], [cmid[j] for j in keep])
    f0, f1 = ks[0], ks[6]
    a = ((((F(0) + (F(-2) * dtf) * f0) + (F(2) * dtf) * f1) + F(-8) * y0) + F(-8) * y1) + F(16) * ym
    b = ((((F(0) + (F(5) * dtf) * f0) + (F(-3) * dtf) * f1) + F(18) * y0) + F(14) * y1) + F(-32) * ym
    c = ((((F(0) + (F(-4) * dtf) * f0) + dtf * f1) + F(-11) * y0) + F(-5) * y1) + F(16) * ym
    return [a, b, c, dtf * f0]


def _fit_any(y0, y1, ks, cmid, dt):
    return _fit_dropped(y0, y1, ks, cmid, dt, [j for j in range(7) if cmid[j] != 0])


@pytest.mark.parametrize('n', SIZES)
def test_interp_eval(dev, n):
    """out = a x^4 + b x^3 + c x^2 + d x + e; then e passed as the SAME panel as another input (the header: e aliases y0, a panel the
    caller also reads elsewhere): the bits of separate panels with equal contents"""
    xp = _xp(0.3)
    host = _panels(n, 5, n + 3)

    def call(ins, outs):
        return _lib().ndcn_interp_eval_f32(*[_p(t) for t in ins], _fa(xp), _p(outs[0]), n, _stream())
    _elementwise(n, dev, host, 1, call, lambda a, b, c, d, e: [o_eval(a, b, c, d, e, xp)], _L().RKF_INTERP_EVAL, 'interp_eval')
    d = [_up(x, dev) for x in host[:4]]
    out = _out(n, dev)
    _ok(_lib().ndcn_interp_eval_f32(_p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), _p(d[0]), _fa(xp), _p(out), n, _stream()))
    with np.errstate(all='ignore'):
        _same(_np(out), o_eval(host[0], host[1], host[2], host[3], host[0], xp), 'interp_eval e == a n=%d' % n)


@pytest.mark.parametrize('n', SIZES)
def test_interp_direct(dev, n):
    dt, sets = _cmids()
    xp = _xp(0.6180339887)
    for name, cmid, skip in sets:
        host = _panels(n, 9, n + 4, skip=skip)

        def call(ins, outs):
            return _lib().ndcn_dopri5_interp_direct_f32(_p(ins[0]), _p(ins[1]), _pa(ins[2:]), _fa(cmid), dt, _fa(xp), _p(outs[0]), n, _stream())

        def oracle(y0, y1, *ks):
            a, b, c, d = _fit_any(y0, y1, ks, cmid, dt)
            return [o_eval(a, b, c, d, y0, xp)]
        _elementwise(n, dev, host, 1, call, oracle, _L().RKF_INTERP_DIRECT, 'interp_direct ' + name)


@pytest.mark.parametrize('nt', range(1, 8))
def test_interp_direct_multi(dev, nt):
    """n_t = 1..7: every tick bit-equal to the oracle AND to ndcn_dopri5_interp_direct_f32 at that tick; 0, 8 and 9 ticks: NDCN_EINVAL (the header: n_t <= 7)"""
    dt, sets = _cmids()
    name, cmid, skip = sets[nt % 2]
    xs = [0.0, 1.0, 0.5, 0.3, 0.3, 0.9, 0.123][:nt]
    xps = [_xp(x) for x in xs]
    flat = [v for xp in xps for v in xp]
    for n in SIZES[:-1] if nt not in (1, 7) else SIZES:
        host = _panels(n, 9, 31 * nt + n, skip=skip)

        def call(ins, outs):
            return _lib().ndcn_dopri5_interp_direct_multi_f32(_p(ins[0]), _p(ins[1]), _pa(ins[2:]), _fa(cmid), dt, _fa(flat), _pa(outs), nt, n,
                                                              _stream())

        def oracle(y0, y1, *ks):
            a, b, c, d = _fit_any(y0, y1, ks, cmid, dt)
            return [o_eval(a, b, c, d, y0, xp) for xp in xps]
        _elementwise(n, dev, host, nt, call, oracle, _L().RKF_INTERP_DIRECT_MULTI, 'interp_direct_multi nt=%d' % nt)
        d = [_up(x, dev) for x in host]
        outs = [_out(n, dev) for _ in range(nt)]
        _ok(call(d, outs))
        for t in range(nt):
            one = _out(n, dev)
            _ok(_lib().ndcn_dopri5_interp_direct_f32(_p(d[0]), _p(d[1]), _pa(d[2:]), _fa(cmid), dt, _fa(xps[t]), _p(one), n, _stream()))
            _same(_np(outs[t]), _np(one), 'direct_multi tick %d vs direct n=%d' % (t, n))
    if nt == 1:
        eight = [_out(n, dev) for _ in range(8)]
        for bad in (0, 8, 9):
            _einval(_lib().ndcn_dopri5_interp_direct_multi_f32(_p(d[0]), _p(d[1]), _pa(d[2:]), _fa(cmid), dt, _fa(flat * 9), _pa(eight + eight[:1]),
                                                               bad, n, _stream()))


@pytest.mark.parametrize('op', range(6))
@pytest.mark.parametrize('n', SIZES)
def test_fixed_stage(dev, n, op):
    """ops 0..5, every needed operand misaligned in turn; then out == y (in place) gives the same bits"""
    need = 1 if op <= 2 else op - 1
    dt = F(0.37)
    host = _panels(n, 1 + need, 7 * op + n)

    def call(ins, outs):
        ks = list(ins[1:]) + [None] * (4 - need)
        return _lib().ndcn_fixed_stage_f32(op, _p(outs[0]), _p(ins[0]), _p(ks[0]), _p(ks[1]), _p(ks[2]), _p(ks[3]), dt, n, _stream())

    def oracle(y, *ks):
        ks = list(ks) + [None] * (4 - need)
        return [o_stage(op, y, ks[0], ks[1], ks[2], ks[3], dt)]
    _elementwise(n, dev, host, 1, call, oracle, _L().RKF_FIXED_STAGE, 'fixed_stage op %d' % op, op=op)
    d = [_up(x, dev) for x in host]
    _ok(call(d, [d[0]]))
    with np.errstate(all='ignore'):
        _same(_np(d[0]), oracle(*host)[0], 'fixed_stage op %d in place n=%d' % (op, n))


def _ticks(nt):
    """coincident and non-coincident ticks mixed"""
    same = [int(q % 3 == 1) for q in range(nt)]
    tm = [F(0.05 * (q + 1)) for q in range(nt)]
    return tm, same


@pytest.mark.parametrize('nt', [1, 8, 9, 17])
def test_tick_emit(dev, nt):
    """one launch per 8 ticks; -0.0 becomes +0.0 and Inf becomes NaN on an interpolated tick, a coincident tick is a copy"""
    dt = F(0.1)
    tm, same = _ticks(nt)
    for n in SIZES[:-1] if nt != 9 else SIZES:
        (y,) = _panels(n, 1, n + nt)

        def call(ins, outs):
            return _lib().ndcn_tick_emit_f32(_p(ins[0]), dt, _fa(tm), _ia(same), _pa(outs), nt, n, _stream())
        with np.errstate(all='ignore'):
            ref = [o_emit(y, dt, tm[q], same[q]) for q in range(nt)]
        first = None
        for which, offs in _phases(n, 1 + nt):
            if which is not None and nt > 9 and which not in (0, 1, 8, 16, 17):
                continue
            yd = _up(y, dev, offs[0])
            outs = [_out(n, dev, o) for o in offs[1:]]
            _ok(call([yd], outs))
            # the LAST launch: ticks 8 * ((nt - 1) // 8) ..; its element path depends on y and on ITS tick panels only
            lo = 8 * ((nt - 1) // 8)
            vec = n % 4 == 0 and offs[0] == 0 and all(o == 0 for o in offs[1 + lo:])
            if n == 0:
                assert _route() == 0
            else:
                _expect(_L().RKF_TICK_EMIT, n // 4 if vec else n, vec)
            got = [_np(o) for o in outs]
            for q in range(nt):
                _same(got[q], ref[q], 'tick_emit nt=%d n=%d tick %d misaligned=%s' % (nt, n, q, which))
            first = first or got
        if n >= 5:
            q_interp = same.index(0)
            got = first[q_interp]
            for i in np.nonzero((y == 0) & np.signbit(y))[0]:
                assert got[i] == 0 and not np.signbit(got[i])
            assert np.isnan(got[np.isinf(y)]).all()
            if 1 in same:
                _same(first[same.index(1)], y, 'coincident tick is a copy')
    assert _lib().ndcn_tick_emit_f32(_p(yd), dt, _fa(tm), _ia(same), _pa([yd] + outs[1:]), nt, n, _stream()) == _L().EINVAL


@pytest.mark.parametrize('op', [0, 5])
@pytest.mark.parametrize('nt', [1, 8, 9])
def test_fixed_stage_emit(dev, op, nt):
    """the stage that ends a step writes the state and its ticks in one pass (the ticks past the eighth by a tick_emit launch behind
    it); the state equals ndcn_fixed_stage_f32's, the ticks are o_emit of it; out == y gives the same bits"""
    need = 1 if op == 0 else 4
    dt = F(0.2)
    tm, same = _ticks(nt)
    for n in SIZES[:-1] if nt != 8 else SIZES:
        host = _panels(n, 1 + need, n + 3 * nt + op)
        with np.errstate(all='ignore'):
            ks = list(host[1:]) + [None] * (4 - need)
            y1 = o_stage(op, host[0], ks[0], ks[1], ks[2], ks[3], dt)
            ref = [y1] + [o_emit(y1, dt, tm[q], same[q]) for q in range(nt)]

        def call(ins, outs):
            kd = list(ins[1:]) + [None] * (4 - need)
            return _lib().ndcn_fixed_stage_emit_f32(op, _p(outs[0]), _p(ins[0]), _p(kd[0]), _p(kd[1]), _p(kd[2]), _p(kd[3]), dt, _fa(tm), _ia(same),
                                                    _pa(outs[1:]), nt, n, _stream())
        for which, offs in _phases(n, 1 + need + 1 + nt):
            ins = [_up(x, dev, o) for x, o in zip(host, offs)]
            outs = [_out(n, dev, o) for o in offs[1 + need:]]
            _ok(call(ins, outs))
            o_ticks = offs[2 + need:]
            if n == 0:
                assert _route() == 0
            elif nt <= 8:
                vec = n % 4 == 0 and which is None
                _expect(_L().RKF_FIXED_STAGE_EMIT, n // 4 if vec else n, vec, op)
            else:                                   # the tick_emit launch behind the stage reads the new state: out and ticks 8..
                vec = n % 4 == 0 and offs[1 + need] == 0 and all(o == 0 for o in o_ticks[8:])
                _expect(_L().RKF_TICK_EMIT, n // 4 if vec else n, vec)
            for q, (o, r) in enumerate(zip(outs, ref)):
                _same(_np(o), r, 'fixed_stage_emit op %d nt=%d n=%d out %d misaligned=%s' % (op, nt, n, q, which))
        ins = [_up(x, dev) for x in host]
        outs = [ins[0]] + [_out(n, dev) for _ in range(nt)]
        _ok(call(ins, outs))
        for q, (o, r) in enumerate(zip(outs, ref)):
            _same(_np(o), r, 'fixed_stage_emit in place op %d out %d' % (op, q))
    assert call(ins, [outs[0], ins[0]] + outs[2:]) == _L().EINVAL          # a tick panel aliases the state
    assert _lib().ndcn_fixed_stage_emit_f32(3, _p(outs[0]), _p(ins[0]), _p(ins[1]), None, None, None, dt, _fa(tm), _ia(same), _pa(outs[1:]), nt, n,
                                            _stream()) == _L().EINVAL


@pytest.mark.parametrize('n', SIZES)
def test_scale_copy_relu_bwd(dev, n):
    """scale and copy take 16 bytes per lane whenever both panels are aligned (any n >= 4: the n % 4 tail by single elements)"""
    L = _L()
    x, g = _panels(n, 2, n + 9)
    w = F(-0.37)
    for offs in ([0, 0], [1, 0], [0, 2], [3, 3]):
        vec = offs == [0, 0] and n >= 4
        items = n // 4 if vec else n
        xd, out = _up(x, dev, offs[0]), _out(n, dev, offs[1])
        _ok(_lib().ndcn_scale_f32(_p(out), _p(xd), w, n, _stream()))
        if n == 0:
            assert _route() == 0
        else:
            _expect(L.RKF_SCALE, items, vec, grid=-(-(items + 1) // 256))
        with np.errstate(all='ignore'):
            _same(_np(out), w * x, 'scale n=%d offs=%s' % (n, offs))
        out = _out(n, dev, offs[1])
        _ok(_lib().ndcn_copy_f32(_p(out), _p(xd), n, _stream()))
        if n == 0:
            assert _route() == 0
        else:
            _expect(L.RKF_COPY, items, vec)
        _same(_np(out), x, 'copy n=%d offs=%s' % (n, offs))
        gd, out = _up(g, dev, offs[1]), _out(n, dev, offs[0])
        _ok(_lib().ndcn_relu_bwd_f32(_p(out), _p(gd), _p(xd), n, _stream()))
        if n == 0:
            assert _route() == 0
        else:
            _expect(L.RKF_RELU_BWD, n, False)
        with np.errstate(all='ignore'):
            _same(_np(out), np.where(x <= 0, F(0), g), 'relu_bwd n=%d offs=%s' % (n, offs))      # a NaN output passes the gradient


# ------------------------------------------------------------------------------------------------------------------ reductions
RTOL, ATOL = F(1e-2), F(1e-3)
CS2 = [F(0.1), F(-0.07)]
N_BASE = (1 << 26) + 8


class _Base:
    host = dev = ws = out = None


def _base(dev):
    """y0, y1, a, b, k0, k1: finite panels of N_BASE elements, host and device (offset 0 and, for y1 and a, float offset 1)"""
    if _Base.host is None:
        rs = np.random.default_rng(2026)
        _Base.host = [(rs.standard_normal(N_BASE, dtype=F) * np.exp2(rs.integers(-4, 5, N_BASE)).astype(F)).astype(F) for _ in range(6)]
        _Base.dev = [_up(x, dev) for x in _Base.host]
        _Base.mis = {1: _up(_Base.host[1], dev, 1), 2: _up(_Base.host[2], dev, 3)}
        _Base.ws = torch.empty(int(_lib().ndcn_reduce_ws_bytes()), dtype=torch.uint8, device=dev)
        _Base.out = torch.zeros(2, dtype=torch.float64, device=dev)
    return _Base


def _rk_error(y0, y1, ks, cs, n, rtol=RTOL, atol=ATOL):
    B = _Base
    B.out.fill_(-7.0)
    _ok(_lib().ndcn_rk_error_f32(_p(y0), _p(y1), _pa(ks), _fa(cs), len(ks), rtol, atol, n, _p(B.out), _p(B.ws), _stream()))
    return B.out.cpu().tolist()


def _sumsq(a, b, y, n, rtol=RTOL, atol=ATOL):
    B = _Base
    B.out.fill_(-7.0)
    _ok(_lib().ndcn_scaled_sumsq_f32(_p(a), _p(b), _p(y), rtol, atol, n, _p(B.out), _p(B.ws), _stream()))
    return B.out.cpu().tolist()


def _eq(got, ref, what):
    assert (math.isnan(got) and math.isnan(float(ref))) or got == float(ref), '%s: got %r, model %r' % (what, got, float(ref))


class _bound:
    """ndcn_set_aten_norm_max(v) for the block; the previous override comes back"""
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.prev = int(_lib().ndcn_set_aten_norm_max(self.v))

    def __exit__(self, *exc):
        _lib().ndcn_set_aten_norm_max(self.prev)
        return False


def _aten_case(B, n):
    L = _L()
    h, d = B.host, B.dev
    y0, y1, a, b, k0, k1 = (x[:n] for x in h)
    dy0, dy1, da, db, dk0, dk1 = (x[:n] for x in d)
    if n >= 8:
        got = _rk_error(dy0, dy1, [dk0, dk1], CS2, n)
        _expect(L.RKF_ERROR, 1, False, extra=L.RKF_ATEN, grid=1)
        _eq(got[0], ao.cascade_sum(ao.error_elements(y0, y1, [k0, k1], CS2, RTOL, ATOL)), 'error n=%d' % n)
        assert got[1] == 0
    for bb, dbb in ((b, db), (None, None)):
        got = _sumsq(da, dbb, dy0, n)
        _expect(L.RKF_SUMSQ, 1, False, extra=L.RKF_ATEN, grid=1)
        _eq(got[0], ao.lane8_fma_sumsq(ao.scaled_q(a, bb, y0, RTOL, ATOL)), 'sumsq n=%d b=%s' % (n, bb is not None))
        assert got[1] == 0


def test_aten_order_every_small_n(dev):
    """n = 1..300: left-over vectors 0..3 and every n % 8 tail (error from 8: below that it takes the parallel route by design)"""
    B = _base(dev)
    for n in range(1, 301):
        _aten_case(B, n)
    for n in range(1, 8):
        got = _rk_error(B.dev[0][:n], B.dev[1][:n], [B.dev[4][:n], B.dev[5][:n]], CS2, n)
        _expect(_L().RKF_ERROR, n, n % 4 == 0, extra=_L().RKF_PAR64, grid=1)           # n = 4: one float4 item
        ref = float(ao.error_elements(*(x[:n] for x in B.host[:2]), [B.host[4][:n], B.host[5][:n]], CS2, RTOL, ATOL).astype(np.float64).sum())
        assert abs(got[0] - ref) <= 1.01 * n * 2.0 ** -53 * ref


@pytest.mark.parametrize('center', [512, 2048, 4096, 8192, 131072])
def test_aten_order_at_the_cascade_and_buffer_edges(dev, center):
    """the level hand-overs at 16 steps (512 elements), 256 (8192) and 4096 (131072), the 2048-element double-buffer edges, each with
    a partial trailing run, left-over vectors and a tail on either side"""
    B = _base(dev)
    for d in ao.EDGE_OFFSETS:
        _aten_case(B, center + d)


@pytest.mark.parametrize('n', [8000, 16401, 65536, 65569, 173312, (1 << 18) - 1, 1 << 18])
def test_aten_order_reference_sized(dev, n):
    _aten_case(_base(dev), n)


@pytest.mark.parametrize('n', ao.ATEN_SIZES_RAISED_BOUND)
def test_aten_order_with_the_bound_raised(dev, n):
    B = _base(dev)
    with _bound(1 << 24):
        _aten_case(B, n)
    assert int(_lib().ndcn_set_aten_norm_max(-1)) == -1              # the override was restored: none


def test_the_size_lists_are_the_host_tests(dev):
    got = set(range(1, 301)) | {c + d for c in (512, 2048, 4096, 8192, 131072) for d in ao.EDGE_OFFSETS} | \
        {8000, 16401, 65536, 65569, 173312, (1 << 18) - 1, 1 << 18}
    assert got == set(ao.ATEN_SIZES)


def test_aten_order_seven_terms_and_subnormal_operands(dev):
    """dopri5's own 7-term error estimate; then panels of subnormal magnitude with rtol 1, atol 0: numerator and denominator of the
    quotient are subnormal, the quotient is not - a division that is not correctly rounded shows in the sum's bits"""
    L = _L()
    for n in (63, 1000, 8000):
        host = _panels(n, 9, n, specials=False)
        d = [_up(x, dev) for x in host]
        cs = [F(0.01 * (j + 1) * (-1) ** j) for j in range(7)]
        _base(dev)
        got = _rk_error(d[0], d[1], d[2:], cs, n)
        _expect(L.RKF_ERROR, 1, False, extra=L.RKF_ATEN, grid=1)
        _eq(got[0], ao.cascade_sum(ao.error_elements(host[0], host[1], host[2:], cs, RTOL, ATOL)), '7-term error n=%d' % n)
        tiny = [(x * F(2.0 ** -140)).astype(F) for x in host[:5]]
        assert all((np.abs(t[t != 0]) < 1.2e-38).all() for t in tiny)
        td = [_up(x, dev) for x in tiny]
        got = _rk_error(td[0], td[1], td[2:4], [F(1), F(-1)], n, rtol=F(1), atol=F(0))
        _eq(got[0], ao.cascade_sum(ao.error_elements(tiny[0], tiny[1], tiny[2:4], [F(1), F(-1)], F(1), F(0))), 'subnormal error n=%d' % n)
        for bb, dbb in ((tiny[3], td[3]), (None, None)):
            got = _sumsq(td[2], dbb, td[0], n, rtol=F(1), atol=F(0))
            _eq(got[0], ao.lane8_fma_sumsq(ao.scaled_q(tiny[2], bb, tiny[0], F(1), F(0))), 'subnormal sumsq n=%d' % n)


def test_bound_selects_the_route(dev):
    """n at the bound and one past it take different routes - default bound (2^18) and an override of 4096; n = 0 gives {0, 0}"""
    L = _L()
    B = _base(dev)
    d = B.dev
    for override, bound in ((None, 1 << 18), (4096, 4096)):
        with _bound(-1 if override is None else override):
            for n, aten in ((bound, True), (bound + 1, False)):
                _rk_error(d[0][:n], d[1][:n], [d[4][:n], d[5][:n]], CS2, n)
                r_err = _route()
                _sumsq(d[2][:n], d[3][:n], d[0][:n], n)
                r_sq = _route()
                for r in (r_err, r_sq):
                    assert bool(r & L.RKF_ATEN) == aten and bool(r & L.RKF_PAR64) == (not aten), (n, hex(r))
                    assert (r >> L.RKF_GRID_SHIFT) == (1 if aten else min(-(-(n) // 256), 2048))      # bound + 1 is odd: scalar items
    e = d[0][:0]
    assert _rk_error(e, e, [e, e], CS2, 0) == [0.0, 0.0]
    _expect(L.RKF_ERROR, 0, True, extra=L.RKF_PAR64, grid=1)            # aligned empty panels: the 16-byte path, no items
    assert _sumsq(e, e, e, 0) == [0.0, 0.0]
    _expect(L.RKF_SUMSQ, 0, True, extra=L.RKF_PAR64, grid=1)


PAR_SIZES = [(1 << 18) + 1, 2048 * 256 * 4 - 4, 2048 * 256 * 4, 2048 * 256 * 4 + 4, 2048 * 256 + 1, 1000003, 1 << 26]


@pytest.mark.parametrize('n', PAR_SIZES)
def test_parallel_route(dev, n):
    """the fp64 pair on both element paths: grid = min(ceil(items / 256), 2048) where it begins to bind, the bound of any summation
    tree of n non-negative terms, two runs the same bits"""
    L = _L()
    B = _base(dev)
    y0, y1, a, b, k0, k1 = (x[:n] for x in B.host)
    ref_e = float(ao.error_elements(y0, y1, [k0, k1], CS2, RTOL, ATOL).astype(np.float64).sum())
    ref_q = {True: float((ao.scaled_q(a, b, y0, RTOL, ATOL).astype(np.float64) ** 2).astype(F).astype(np.float64).sum())}
    qn = ao.scaled_q(a, None, y0, RTOL, ATOL)
    ref_q[False] = float((qn * qn).astype(np.float64).sum())
    qb = ao.scaled_q(a, b, y0, RTOL, ATOL)
    ref_q[True] = float((qb * qb).astype(np.float64).sum())
    tol = 1.01 * n * 2.0 ** -53
    for mis in (False, True):
        vec = n % 4 == 0 and not mis
        items = n // 4 if vec else n
        grid = min(-(-items // 256), 2048)
        dy0, dk0, dk1, db = B.dev[0][:n], B.dev[4][:n], B.dev[5][:n], B.dev[3][:n]
        dy1 = (B.mis[1] if mis else B.dev[1])[:n]
        da = (B.mis[2] if mis else B.dev[2])[:n]
        got = _rk_error(dy0, dy1, [dk0, dk1], CS2, n)
        _expect(L.RKF_ERROR, items, vec, extra=L.RKF_PAR64, grid=grid)
        assert abs(got[0] - ref_e) <= tol * ref_e and got[1] == 0, ('error', n, mis, got, ref_e)
        assert _rk_error(dy0, dy1, [dk0, dk1], CS2, n) == got
        for hasb in (True, False):
            got = _sumsq(da, db if hasb else None, dy0, n)
            _expect(L.RKF_SUMSQ, items, vec, extra=L.RKF_PAR64, grid=grid)
            assert abs(got[0] - ref_q[hasb]) <= tol * ref_q[hasb] and got[1] == 0, ('sumsq', n, mis, hasb, got, ref_q[hasb])
            assert _sumsq(da, db if hasb else None, dy0, n) == got


# n = 181: 5 interleaved steps (160 elements), 2 left-over vectors (160..175), a tail of 5 (176..180)
NF_N = 181
NF_PLANTS = [[0], [180], [178], [165], [0, 180], [177, 161], [0, 161, 170, 177, 180]]


@pytest.mark.parametrize('where', NF_PLANTS)
def test_nonfinite_record(dev, where):
    """1, 2 and 5 non-finite values (Inf, -Inf, NaN in turn) at the first element, the last, inside the n % 8 tail and inside the
    left-over vectors - in y1 for error, in a for sumsq: d_out[1] is the count on both routes, d_out[0] the model's (ATen route);
    a NaN in y0 only gives a NaN sum and count 0"""
    L = _L()
    n = NF_N
    host = _panels(n, 6, 181, specials=False)
    y0, y1, a, b, k0, k1 = host
    for j, i in enumerate(where):
        y1[i] = a[i] = F((INF, -INF, NAN)[(j + len(where)) % 3])
    d = [_up(x, dev) for x in host]
    _base(dev)
    for override, flag in ((-1, L.RKF_ATEN), (0, L.RKF_PAR64)):
        with _bound(override):
            got = _rk_error(d[0], d[1], d[4:], CS2, n)
            assert _route() & flag
            assert got[1] == len(where), (got, where)
            el = ao.error_elements(y0, y1, [k0, k1], CS2, RTOL, ATOL)
            if flag == L.RKF_ATEN:
                _eq(got[0], ao.cascade_sum(el), 'error sum with non-finite y1')
            else:
                assert math.isnan(got[0]) == bool(np.isnan(el).any())
            for bb, dbb in ((b, d[3]), (None, None)):
                got = _sumsq(d[2], dbb, d[0], n)
                assert _route() & flag
                assert got[1] == len(where), (got, where)
                q = ao.scaled_q(a, bb, y0, RTOL, ATOL)
                if flag == L.RKF_ATEN:
                    _eq(got[0], ao.lane8_fma_sumsq(q), 'sumsq with non-finite a')
                else:
                    assert math.isnan(got[0]) == bool(np.isnan(q).any()) and (math.isinf(got[0]) == bool(np.isinf(q).any() and not np.isnan(q).any()))
            y0n = y0.copy()
            y0n[where[0]] = NAN
            got = _rk_error(_up(y0n, dev), _up(np.ones(n, F), dev), d[4:], CS2, n)
            assert math.isnan(got[0]) and got[1] == 0
