"""fixed_adams (the reference's AdamsBashforthMoulton, torchdiffeq/_impl/fixed_adams.py:151-205) on a real MI355X: the two kernels
ndcn_abm_predict_f32 / ndcn_abm_correct_f32 bit for bit against the numpy restatement (tests/_adams_moulton.py) with exact failure
counts, the library solve (ndcn_solve_fixed_adams_f32) and the generic branch (core.integrate_fixed over the panel ops) against the
fixtures captured from the reference (tests/golden/moulton_*.npz) and against each other, a tuple state, gradients against float64
autograd, and the drivers."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import _adams_bashforth as ab
import _adams_moulton as am
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = (0, 1, 3, 5, 1027, 2 ** 18 + 5)
WARNING = 'Warning: Functional iteration did not converge. Solution may be incorrect.'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.asarray(a))


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'moulton_*.npz')))


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same_bits(t, a):
    return np.array_equal(bits(t.cpu().numpy()), bits(a))


def at_offset(a, off, dev):
    """a copy of the 1-d array on the device that starts `off` elements behind a 16-byte boundary"""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.size]
    v.copy_(T(a))
    return v


def P(v):
    """the device address of a view's first element (an EMPTY view reports a null data_ptr; the kernels are handed real addresses)"""
    return ctypes.c_void_p(v.untyped_storage().data_ptr() + 4 * v.storage_offset())


def raw_predict(dev, y, fs, a, m, dt, offs):
    """ndcn_abm_predict_f32 through ctypes with every panel at its own offset: offs = (y, outputs, [history])"""
    from ndcn_amd import _lib
    lib = _lib.load()
    n, size = len(fs), y.size
    yd = at_offset(y, offs[0], dev)
    outs = [at_offset(np.full(size, 7.0, dtype=f32), offs[1], dev) for _ in range(3)]
    fd = [at_offset(f, o, dev) for f, o in zip(fs, offs[2])]
    arr_f = (ctypes.c_void_p * n)(*[P(d).value for d in fd])
    arr_a = (ctypes.c_float * n)(*[float(x) for x in a])
    arr_m = (ctypes.c_float * n)(*[float(x) for x in m])
    rc = lib.ndcn_abm_predict_f32(P(outs[0]), P(outs[1]), P(outs[2]), P(yd), arr_f, arr_a, arr_m, n, float(dt), size, _lib.stream_ptr())
    assert rc == 0, lib.ndcn_last_error()
    torch.cuda.synchronize()
    return outs, yd, fd


def raw_correct(dev, f, delta, y, dy, c0, rtol, atol, offs):
    """ndcn_abm_correct_f32 through ctypes: offs = (f, delta, y, dy, u); returns (dy, u, count)"""
    from ndcn_amd import _lib
    lib = _lib.load()
    size = y.size
    fd, dd, yd, dyd = (at_offset(v, o, dev) for v, o in zip((f, delta, y, dy), offs[:4]))
    u = at_offset(np.full(size, 7.0, dtype=f32), offs[4], dev)
    count = torch.full((1,), 99, dtype=torch.int64, device=dev)
    rc = lib.ndcn_abm_correct_f32(P(dyd), P(u), P(fd), P(dd), P(yd), float(c0), float(rtol), float(atol), size, _lib.ptr(count),
                                  _lib.stream_ptr())
    assert rc == 0, lib.ndcn_last_error()
    torch.cuda.synchronize()
    assert same_bits(fd, f) and same_bits(dd, delta) and same_bits(yd, y)            # the inputs are only read
    return dyd, u, int(count.cpu()[0])


def layouts(n):
    """name -> (offset of y, of the outputs, of every history panel), in elements: all on a 16-byte boundary, all 4 / all 12 bytes behind
    one, and mixed"""
    return {'aligned': (0, 0, [0] * n), 'plus4': (1, 1, [1] * n), 'plus12': (3, 3, [3] * n),
            'mixed': (0, 2, [q % 4 for q in range(n)])}


# ------------------------------------------------------------------------------------------------------------------------ the kernels

@pytest.mark.parametrize('layout', ['aligned', 'plus4', 'plus12', 'mixed'])
@pytest.mark.parametrize('n', [3, 4, 11])
def test_predict_bit_for_bit(dev, n, layout):
    rng = np.random.RandomState(300 + n)
    a, (lead, m) = ab.weights(n), am.weights(n)
    oy, oo, of = layouts(n)[layout]
    for size in SIZES:
        y = rng.randn(size).astype(f32)
        fs = [rng.randn(size).astype(f32) for _ in range(n)]
        dt = f32(0.0371)
        dy, delta, u = am.predict(y, fs, dt)
        outs, yd, fd = raw_predict(dev, y, fs, a, m, dt, (oy, oo, of))
        assert same_bits(outs[0], dy) and same_bits(outs[1], delta) and same_bits(outs[2], u), (n, size, layout)
        assert same_bits(yd, y) and all(same_bits(d, f) for d, f in zip(fd, fs))


def test_predict_through_the_ops_and_signed_zero(dev):
    from ndcn_amd import hip
    n = 3
    a, (_, m) = ab.weights(n), am.weights(n)
    y = np.array([1.0, -0.0, 0.0, 2.0, -3.0], dtype=f32)
    fs = [np.array([-0.0, 0.0, 1.0, np.inf, np.nan], dtype=f32), np.zeros(5, dtype=f32), np.array([0, 0, -2.0, 1, 1], dtype=f32)]
    want = am.predict(y, fs, f32(0.5))
    got = hip.abm_predict(T(y).to(dev), [T(f).to(dev) for f in fs], a, m, 0.5)
    for g, w in zip(got, want):
        assert same_bits(g, w)


@pytest.mark.parametrize('layout', ['aligned', 'plus4', 'plus12', 'mixed'])
def test_correct_bit_for_bit_with_the_exact_count(dev, layout):
    rng = np.random.RandomState(17)
    offs = {'aligned': (0,) * 5, 'plus4': (1,) * 5, 'plus12': (3,) * 5, 'mixed': (0, 1, 2, 3, 0)}[layout]
    for size in SIZES:
        f, delta, y = (rng.randn(size).astype(f32) for _ in range(3))
        c0 = f32(0.0123)
        dy = (c0 * f + delta + rng.randn(size).astype(f32) * f32(1e-3)).astype(f32)      # near the fixed point: some pass, some fail
        rtol, atol = 1e-3, 1e-4
        new, u, bad = am.correct(f, delta, y, dy, c0, rtol, atol)
        got_dy, got_u, count = raw_correct(dev, f, delta, y, dy, c0, rtol, atol, offs)
        assert same_bits(got_dy, new) and same_bits(got_u, u), (size, layout)
        assert count == bad, (size, layout)
        if size > 100:
            assert 0 < bad < size


def planted(size, where, dev, offset):
    """a pass in which every element converges (dy is already the fixed point) except the planted ones"""
    rng = np.random.RandomState(size)
    f, delta, y = (rng.randn(size).astype(f32) for _ in range(3))
    c0 = f32(0.05)
    dy = (c0 * f + delta).astype(f32)
    for e in where:
        dy[e] += f32(1.0)
    new, u, bad = am.correct(f, delta, y, dy, c0, 1e-3, 1e-4)
    assert bad == len(where)
    got_dy, got_u, count = raw_correct(dev, f, delta, y, dy, c0, 1e-3, 1e-4, (offset,) * 5)
    assert same_bits(got_dy, new) and same_bits(got_u, u)
    return count


def test_count_of_planted_failures(dev):
    size = 2 ** 18 + 5
    # panels 4 bytes behind a boundary: a head of three elements, a 16-byte body of 2^18, a tail of two
    assert (size - 3) % 4 == 2
    assert planted(size, [], dev, 1) == 0
    assert planted(size, [0], dev, 1) == 1                                        # the first element
    assert planted(size, [1], dev, 1) == 1 and planted(size, [2], dev, 1) == 1    # inside the head
    assert planted(size, [3], dev, 1) == 1 and planted(size, [12345], dev, 1) == 1 and planted(size, [size - 3], dev, 1) == 1   # the body
    assert planted(size, [size - 2], dev, 1) == 1                                 # inside the tail
    assert planted(size, [size - 1], dev, 1) == 1                                 # the last element
    assert planted(size, [0, 1, 2, 7777, 2 ** 17, size - 2, size - 1], dev, 1) == 7
    # 12 bytes behind: a head of one; aligned; single-element sizes
    assert planted(1027, [0], dev, 3) == 1 and planted(1027, [1, 1025, 1026], dev, 3) == 3
    assert planted(1027, [0, 1024, 1026], dev, 0) == 3
    assert planted(5, [4], dev, 0) == 1 and planted(1, [0], dev, 0) == 1 and planted(3, [1], dev, 2) == 1


def test_count_nan_equality_and_zero_tolerances(dev):
    size = 1027
    rng = np.random.RandomState(4)
    f, delta, y = (rng.randn(size).astype(f32) for _ in range(3))
    c0 = f32(0.05)
    fixed = (c0 * f + delta).astype(f32)
    # a NaN in f: dy' is NaN there, the comparison is false
    f_nan = f.copy()
    f_nan[500] = np.nan
    new, u, bad = am.correct(f_nan, delta, y, fixed, c0, 1e-3, 1e-4)
    got_dy, got_u, count = raw_correct(dev, f_nan, delta, y, fixed, c0, 1e-3, 1e-4, (0,) * 5)
    assert bad == 1 == count and same_bits(got_dy, new) and same_bits(got_u, u)
    # err == tol exactly: f = 0, delta = 0 -> dy' = 0; dy_old = 0.5, rtol = 1, atol = 0 -> tol = 0.5 = err: the strict `<` fails
    z = np.zeros(size, dtype=f32)
    old = z.copy()
    old[[0, 600, size - 1]] = f32(0.5)
    new, u, bad = am.correct(z, z, y, old, c0, 1.0, 0.0)
    assert bad == size                                                            # (0 < 0 is false too: every other element has err = tol = 0)
    assert raw_correct(dev, z, z, y, old, c0, 1.0, 0.0, (0,) * 5)[2] == size
    old2 = np.full(size, f32(0.25), dtype=f32)                                    # err = 0.25 < tol = 0.25 + atol everywhere ...
    old2[[0, 600, size - 1]] = f32(0.5)                                           # ... with atol = 0.25: tol = 0.25 + 0.5 * 0.5 = 0.5 = err at three
    new, u, bad = am.correct(z, z, y, old2, c0, 0.5, 0.25)
    assert bad == 3
    assert raw_correct(dev, z, z, y, old2, c0, 0.5, 0.25, (0,) * 5)[2] == 3
    # rtol = atol = 0: err < 0 never holds
    assert raw_correct(dev, f, delta, y, fixed, c0, 0.0, 0.0, (0,) * 5)[2] == size
    assert raw_correct(dev, f, delta, y, fixed, c0, 0.0, 0.0, (1,) * 5)[2] == size


def test_kernels_refuse_bad_arguments_before_any_launch(dev):
    from ndcn_amd import _lib
    lib = _lib.load()
    size = 64
    y = torch.ones(size, device=dev)
    outs = [torch.full((size,), 7.0, device=dev) for _ in range(3)]
    fs = [torch.ones(size, device=dev) for _ in range(12)]
    coef = (ctypes.c_float * 12)(*([0.1] * 12))

    def predict(n, ptrs, o=None):
        o = o or [x.data_ptr() for x in outs]
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        return lib.ndcn_abm_predict_f32(o[0], o[1], o[2], _lib.ptr(y), arr, coef, coef, n, 0.1, size, _lib.stream_ptr())
    good = [f.data_ptr() for f in fs]
    assert predict(2, good[:2]) == _lib.EINVAL and predict(12, good) == _lib.EINVAL        # the orders are 3..11
    assert predict(3, [good[0], None, good[2]]) == _lib.EINVAL                           # a null panel
    for q in range(3):                                                                   # an output that is a history panel
        o = [x.data_ptr() for x in outs]
        o[q] = good[1]
        assert predict(3, good[:3], o) == _lib.EINVAL
        assert b'aliases' in lib.ndcn_last_error()
    o = [x.data_ptr() for x in outs]
    assert predict(3, good[:3], [o[0], o[0], o[2]]) == _lib.EINVAL                       # outputs that alias each other
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def correct(dy, u, f, delta, yy, cnt=count):
        return lib.ndcn_abm_correct_f32(_lib.ptr(dy), _lib.ptr(u), _lib.ptr(f), _lib.ptr(delta), _lib.ptr(yy), 0.1, 1e-3, 1e-4, size,
                                        _lib.ptr(cnt), _lib.stream_ptr())
    assert correct(outs[0], outs[1], fs[0], fs[1], None) == _lib.EINVAL
    assert correct(outs[0], outs[1], fs[0], fs[1], y, cnt=None) == _lib.EINVAL
    assert correct(outs[0], fs[0], fs[0], fs[1], y) == _lib.EINVAL                       # u aliases f
    assert correct(outs[0], outs[0], fs[0], fs[1], y) == _lib.EINVAL                     # u aliases dy
    torch.cuda.synchronize()
    assert all(bool((x == 7.0).all()) for x in outs) and int(count.cpu()[0]) == 0        # nothing was written
    assert predict(3, good[:3]) == 0 and correct(outs[0], outs[1], fs[0], fs[1], y) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------- the solves

def make_func(d, dev):
    from ndcn_amd import CsrOperator
    from ndcn_amd.neural_dynamics import ODEFunc
    A = CsrOperator.from_arrays(d['indptr'], d['indices'], d['data'], d['shape'], dev)
    f = ODEFunc(d['W'].shape[0], A).to(dev)
    f.load_state_dict({'wt.weight': T(d['W']), 'wt.bias': T(d['b'])})
    return f.eval()


def options_of(d):
    o = {}
    for k in ('max_order', 'max_iters'):
        if 'opt_' + k in d:
            o[k] = int(d['opt_' + k])
    if 'opt_step_size' in d:
        o['step_size'] = float(d['opt_step_size'])
    return o


def solve(func, x0, t, d_or_tol, opts, capfd):
    """(solution, [(iterations, converged)], nfe, warning lines on stderr)"""
    from ndcn_amd import torchdiffeq as ode
    rtol, atol = d_or_tol
    log = []
    capfd.readouterr()
    with torch.no_grad():
        y = ode.odeint(func, x0, t, rtol=rtol, atol=atol, method='fixed_adams', options=dict(opts) or None, step_log=log)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert log[-1][0] == 'nfe'
    return y, log[:-1], log[-1][1], [l for l in err.splitlines() if l == WARNING]


@pytest.mark.parametrize('name', names())
def test_golden_on_both_paths(dev, name, monkeypatch, capfd):
    """the library solve (the ODEFunc itself) and the generic branch (a lambda around it: the library route declines) against the
    reference's trajectory, iteration counts, flags, evaluation count and warning lines; the two bit for bit equal on every tick and on
    every grid step; the warm-up the bits of method='rk4' on the same path"""
    from ndcn_amd import torchdiffeq as ode
    import importlib
    impl = importlib.import_module('ndcn_amd.torchdiffeq._impl.odeint')
    d = load_golden(name)
    f = make_func(d, dev)
    x0, t, opts, tol = T(d['x0']).to(dev), T(d['t']).to(dev), options_of(d), (float(d['rtol']), float(d['atol']))
    taken = []
    real = impl._fixed_adams_solve
    monkeypatch.setattr(impl, '_fixed_adams_solve', lambda *a: taken.append(real(*a)) or taken[-1])
    calls = []

    def wrapped(tt, y):
        calls.append(1)
        return f(tt, y)
    gen, gen_log, gen_nfe, gen_warn = solve(wrapped, x0, t, tol, opts, capfd)
    assert not taken
    res, res_log, res_nfe, res_warn = solve(f, x0, t, tol, opts, capfd)
    assert len(taken) == 1 and taken[0] is not None                                # the library's solve ran for the plain ODEFunc
    want_log = list(zip(d['iters'].tolist(), [bool(c) for c in d['converged']]))
    bound = 1e-6 * max(1.0, np.abs(d['traj']).max())                              # the fixed-grid bound (tests/test_oracle_golden.py)
    for y, log, nfe, warn in ((gen, gen_log, gen_nfe, gen_warn), (res, res_log, res_nfe, res_warn)):
        assert y.shape == d['traj'].shape and np.array_equal(y[0].cpu().numpy(), d['x0'])
        err = np.abs(y.cpu().numpy() - d['traj']).max()
        print('%s: max |y - reference| = %.3e (bound %.3e)' % (name, err, bound))
        assert err <= bound
        assert log == want_log
        assert nfe == int(d['nfe'])
        assert len(warn) == int(d['n_warnings'])
    assert len(calls) == int(d['nfe'])
    assert torch.equal(gen, res)
    # every grid step: the solves on the explicit grid (each grid point a tick), again on both paths
    grid = T(ab.grid_of(d['t'], opts.get('step_size'))).to(dev)
    o2 = {k: v for k, v in opts.items() if k != 'step_size'}
    gen_g = solve(wrapped, x0, grid, tol, o2, capfd)[0]
    res_g = solve(f, x0, grid, tol, o2, capfd)[0]
    with torch.no_grad():
        rk_gen = ode.odeint(lambda tt, y: f(tt, y), x0, grid[:3], method='rk4')
        rk_res = ode.odeint(f, x0, grid[:3], method='rk4')
    assert torch.equal(gen_g, res_g)
    assert torch.equal(gen_g[:3], rk_gen) and torch.equal(res_g[:3], rk_res)


def test_implicit_false_is_explicit_adams(dev):
    from ndcn_amd import torchdiffeq as ode
    d = load_golden('moulton_default')
    f = make_func(d, dev)
    x0, t = T(d['x0']).to(dev), T(d['t']).to(dev)
    with torch.no_grad():
        for func in (f, lambda tt, y: f(tt, y)):
            a = ode.odeint(func, x0, t, method='fixed_adams', options={'implicit': False, 'max_order': 6})
            b = ode.odeint(func, x0, t, method='explicit_adams', options={'max_order': 6})
            assert torch.equal(a, b)
        c = ode.odeint(f, x0, t, rtol=1e-2, atol=1e-3, method='fixed_adams', options={'max_order': 6})
    assert not torch.equal(a, c)                                                   # (the corrector does something)


def lattice_func(side, H, dev, seed=0):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(seed)
    f = ODEFunc(H, graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(side)), dev)).to(dev).eval()
    return f, torch.rand(side * side, H).to(dev)


@pytest.mark.parametrize('H,mid', [(20, 0), (20, 2), (64, 2)], ids=['H20-composed', 'H20-rhs_mid', 'H64-rhs_mid'])
def test_larger_graph_library_solve_equals_generic_branch(dev, H, mid, capfd):
    """a 40 x 40 lattice - beyond the one-launch solves - with the right-hand side dispatched to the composed launches and to rhs_mid:
    the same bits, iteration counts and flags on both routes, with tolerances that make some steps iterate"""
    from ndcn_amd import _lib
    lib = _lib.load()
    f, x0 = lattice_func(40, H, dev)
    t = (torch.arange(15) / 128.0).to(dev)
    prev = lib.ndcn_set_rhs_mid(mid)
    try:
        res, res_log, res_nfe, res_warn = solve(f, x0, t, (1e-4, 1e-5), {}, capfd)
        path = int(lib.ndcn_debug_last_rhs_path())
        gen, gen_log, gen_nfe, gen_warn = solve(lambda tt, y: f(tt, y), x0, t, (1e-4, 1e-5), {}, capfd)
        sub = solve(f, x0, t[[0, 5, 14]], (1e-2, 1e-3), {'step_size': 1.0 / 128, 'max_order': 6, 'max_iters': 2}, capfd)
        sub_gen = solve(lambda tt, y: f(tt, y), x0, t[[0, 5, 14]], (1e-2, 1e-3), {'step_size': 1.0 / 128, 'max_order': 6, 'max_iters': 2}, capfd)
    finally:
        lib.ndcn_set_rhs_mid(prev)
    assert bool(path & _lib.PATH_MID) == (mid == 2)
    assert bool(torch.isfinite(res).all()) and torch.equal(res, gen)
    assert res_log == gen_log and res_nfe == gen_nfe and len(res_warn) == len(gen_warn) == sum(1 for _, c in res_log if not c)
    assert res_log[:2] == [(0, True)] * 2 and all(1 <= i <= 4 for i, _ in res_log[2:])
    assert res_nfe == 14 + 6 + sum(i for i, _ in res_log)
    assert torch.equal(sub[0], sub_gen[0]) and sub[1:3] == sub_gen[1:3] and len(sub[3]) == len(sub_gen[3])


def test_tuple_state_on_the_generic_branch(dev, capfd):
    """a 2-tuple state: both tensors must pass the test; against the restatement on the concatenated state (every operation is
    elementwise and the all-elements decision is the conjunction over the tensors)"""
    from ndcn_amd import torchdiffeq as ode
    rng = np.random.RandomState(8)
    a0, b0 = rng.rand(37).astype(f32), rng.rand(5, 3).astype(f32)
    ca, cb = f32(-0.7), f32(-1.3)

    def func(tt, y):
        return (y[0] * float(ca), y[1] * float(cb))

    def rhs(x):
        return np.concatenate([(x[:37] * ca).astype(f32), (x[37:] * cb).astype(f32)])
    t = np.linspace(0., 0.8, 17).astype(f32)
    for rtol, atol in ((1e-3, 1e-5), (0.0, 0.0)):
        want, nfe, wlog, _ = am.solve(rhs, np.concatenate([a0, b0.ravel()]), t, rtol=rtol, atol=atol)
        log = []
        capfd.readouterr()
        with torch.no_grad():
            ya, yb = ode.odeint(func, (T(a0).to(dev), T(b0).to(dev)), T(t).to(dev), rtol=rtol, atol=atol, method='fixed_adams', step_log=log)
        n_warn = capfd.readouterr().err.count(WARNING)
        assert same_bits(ya, want[:, :37]) and same_bits(yb.reshape(17, 15), want[:, 37:])
        assert log[:-1] == wlog and log[-1] == ('nfe', nfe) and n_warn == sum(1 for _, c in wlog if not c)
    assert wlog[2:] == [(4, False)] * 14


# --------------------------------------------------------------------------------------------------------------------------- gradients

def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def fp64_solve(A, W, b, y0, t, iters):
    """fixed_adams in float64 torch on the CPU with the exact rational weights and the iteration counts FIXED to `iters` (what the device
    solve ran): the function whose autograd is the truth - the counts are constants of the graph"""
    f = lambda x: torch.relu((A @ x) @ W.t() + b)
    hist, y, sol = [], y0, [y0]
    for i in range(len(t) - 1):
        dt = t[i + 1] - t[i]
        hist.insert(0, f(y))
        del hist[11:]
        k = len(hist)
        if k < 3:
            k1 = hist[0]
            k2 = f(y + dt * k1 / 3)
            k3 = f(y + dt * (k1 / -3 + k2))
            k4 = f(y + dt * (k1 - k2 + k3))
            y = y + (k1 + 3 * k2 + 3 * k3 + k4) * (dt / 8)
        else:
            mu = [float(x) for x in am.mus(k)]
            dy = dt * sum(float(bi) * fi for bi, fi in zip(ab.betas(k), hist))
            delta = dt * sum(mi * fi for mi, fi in zip(mu[1:], hist))
            assert iters[i][0] >= 1 and iters[i][1]
            for _ in range(iters[i][0]):
                dy = dt * mu[0] * f(y + dy) + delta
            y = y + dy
        sol.append(y)
    return torch.stack(sol)


def test_gradients_against_fp64_autograd(dev, capfd):
    """6 x 6 lattice, H = 8, 12 steps, tolerances that make the later steps iterate twice: the gradients of y0, W and b of
    backpropagation through the solve (core.integrate_fixed over autograd_ops: predictor and corrector are linear maps, the count comes
    from the kernel) against torch autograd through the float64 restatement with the same iteration counts.  The bound of
    tests/test_gpu_autograd.py for backpropagation through a fixed grid: 2e-4 of each tensor's maximum."""
    from ndcn_amd import graphs
    from ndcn_amd import torchdiffeq as ode
    f, x0 = lattice_func(6, 8, dev, seed=3)
    x = x0.clone().requires_grad_(True)
    t = torch.arange(13) * (2.0 / 128)
    target = torch.rand(13, 36, 8, generator=torch.Generator().manual_seed(9))
    log = []
    y = ode.odeint(f, x, t.to(dev), rtol=1e-4, atol=1e-5, method='fixed_adams', step_log=log)
    loss = torch.nn.functional.l1_loss(y, target.to(dev))
    loss.backward()
    iters = log[:-1]
    print('iterations under the gradient:', iters)
    assert len(iters) == 12 and all(c for _, c in iters) and max(i for i, _ in iters) >= 2
    # the same solve without a gradient (the library route) takes the same decisions and gives the same bits
    plain, plain_log, _, _ = solve(f, x0, t.to(dev), (1e-4, 1e-5), {}, capfd)
    assert plain_log == iters and torch.equal(plain, y.detach())
    L = graphs.normalized_laplacian(graphs.grid_8_neighbor(6))
    A = torch.from_numpy(np.asarray(L.todense())).double()
    W = f.wt.weight.detach().cpu().double().requires_grad_(True)
    b = f.wt.bias.detach().cpu().double().requires_grad_(True)
    xc = x0.detach().cpu().double().requires_grad_(True)
    yo = fp64_solve(A, W, b, xc, t.double(), iters)
    lo = torch.nn.functional.l1_loss(yo, target.double())
    assert float((y.detach().cpu().double() - yo.detach()).abs().max()) < 1e-5
    lo.backward()
    for got, ref, what in zip((x.grad, f.wt.weight.grad, f.wt.bias.grad), (xc.grad, W.grad, b.grad), ('y0', 'W', 'b')):
        print('gradient of %s: %.3e of its maximum' % (what, rel(got.cpu().double(), ref)))
        assert rel(got.cpu().double(), ref) < 2e-4


# ----------------------------------------------------------------------------------------------------------------- drivers and the rest

def test_driver_runs_an_epoch_with_fixed_adams(dev, capsys):
    from ndcn_amd.drivers.dynamics import main
    out = main('heat', ['--network', 'grid', '--sampled_time', 'equal', '--baseline', 'ndcn', '--gpu', '0', '--n', '100',
                        '--niters', '1', '--test_freq', '1', '--time_tick', '20', '--method', 'fixed_adams'])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('Iter ')]
    assert len(lines) >= 1 and 'Train Loss' in lines[0] and 'nan' not in lines[0].lower()
    assert out['params'] == 901


def test_host_state_and_sharded_solve_are_refused(dev):
    from ndcn_amd import _lib, hip, sharding
    from ndcn_amd import torchdiffeq as ode
    with pytest.raises(_lib.NdcnHostStateError):
        ode.odeint(lambda tt, y: -y, torch.ones(4), torch.tensor([0., .1, .2], device=dev), method='fixed_adams')
    with pytest.raises(NotImplementedError, match='fixed_adams'):
        sharding.sharded_odeint(hip, None, None, 4, torch.zeros(4, 2, device=dev), torch.tensor([0., 1.], device=dev), method='fixed_adams')
    with pytest.raises(TypeError):
        ode.odeint(lambda tt, y: -y, torch.ones(4, device=dev), torch.tensor([0., .1, .2], device=dev), method='fixed_adams',
                   options={'rtol': 1e-3})
