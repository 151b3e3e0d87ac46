"""explicit_adams / fixed_adams inference with the decoder inside the solve, on a real MI355X (csrc/adams_readout.hip, csrc/adams.hip).
Every comparison is on the raw int32 words of the output against hip.linear applied to what the un-decoded form writes - the state
panel of ndcn_ab_step_f32 for the kernel, the trajectory of the same solve with the switch off (hip.set_adams_readout(0)) for the
solves; NaN positions must coincide, payloads are not compared.  ndcn_last_readout_path() says what ran: 16 the fused step + decode
kernel (8 beside it at H < 64), 4 a staged decode of the state's panel, 0 decode-after."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adams_bashforth as ab                                        # noqa: E402
import _adams_readout as aro                                         # noqa: E402

pytestmark = pytest.mark.gpu

FIXED, NARROW, ADAMS = 4, 8, 16


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def switch_back():
    from ndcn_amd import hip
    yield
    hip.set_adams_readout(-1)


def same_words(got, ref):
    """equal as int32 words wherever the reference is not a NaN, a NaN exactly where the reference has one"""
    got, ref = got.contiguous(), ref.contiguous()
    assert got.shape == ref.shape
    nan_g, nan_r = torch.isnan(got), torch.isnan(ref)
    if not torch.equal(nan_g, nan_r):
        return False
    return bool(torch.equal(got.view(torch.int32)[~nan_r], ref.view(torch.int32)[~nan_r]))


def path():
    from ndcn_amd import _lib
    return int(_lib.load().ndcn_last_readout_path())


def make_decoder(H, C, bias, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    Wd = ((torch.rand(C, H, generator=g) - .5) * (2. / H ** .5)).to(dev)
    bd = (torch.rand(C, generator=g) - .5).to(dev) if bias else None
    return Wd, bd


# ---------------------------------------------------------------------------------------------------------- 1. the kernel
# (rows, H, C, bias, n, emit_off, special): every listed value of the issue at least once per kernel family -
# narrow (H = 16, 20, 60: 1, 2, 4 quads per thread) and wide (H = 64, 68, 100, 256, 512: NV = 1, 2, 2, 4, 8, surplus lanes at 68 / 100)
NARROW_CASES = [(1, 16, 1, True, 3, 0., False), (63, 20, 4, False, 7, 0., False), (64, 60, 5, True, 11, 0., False),
                (65, 20, 15, True, 11, .03, False), (130, 16, 5, False, 7, 0., True), (130, 60, 15, True, 3, .07, True),
                (64, 20, 1, False, 3, .05, False)]
WIDE_CASES = [(1, 64, 1, True, 3, 0., False), (63, 68, 4, False, 7, 0., False), (64, 100, 5, True, 11, 0., False),
              (65, 256, 15, True, 7, .03, False), (130, 512, 1, False, 11, 0., True), (130, 68, 15, True, 3, .07, True),
              (64, 512, 5, True, 11, .05, False), (65, 64, 4, False, 11, 0., False)]


def kernel_inputs(rows, H, n, special, dev):
    g = torch.Generator().manual_seed(rows * 1000 + H + n)
    y = torch.rand(rows, H, generator=g) - .5
    fs = [torch.rand(rows, H, generator=g) - .5 for _ in range(n)]
    if special:
        r = rows - 1
        # a row whose new state holds -0.0 (-0 + -0; from evaluations that are all zero the sum would be +0 and the state +0) and +Inf
        y[r] = 0.
        for f in fs:
            f[r] = 0.
        y[r, 0] = -0.
        fs[0][r, 0] = -1.4e-45            # the smallest denormal under the (positive) newest weight: dt * sum underflows to -0.0
        y[r, H - 1] = float('inf')
    return y.to(dev), [f.to(dev) for f in fs]


def run_fused(y, fs, a, dt, Wd, bd, emit_off, out=None):
    from ndcn_amd import _lib
    lib = _lib.load()
    rows, H = y.shape
    C = Wd.shape[0]
    out = torch.full_like(y, 7.) if out is None else out
    dec = torch.full((rows, C), 7., device=y.device)
    n = len(fs)
    arr_f = (ctypes.c_void_p * n)(*[f.data_ptr() for f in fs])
    arr_a = (ctypes.c_float * n)(*[float(v) for v in a])
    rc = lib.ndcn_ab_step_readout_f32(_lib.ptr(out), _lib.ptr(y), arr_f, arr_a, n, float(dt), rows, H, _lib.ptr(Wd), _lib.ptr(bd), C,
                                      _lib.ptr(dec), float(emit_off), _lib.stream_ptr())
    return rc, out, dec


@pytest.mark.parametrize('rows,H,C,bias,n,emit_off,special', NARROW_CASES + WIDE_CASES, ids=lambda v: str(v))
def test_step_and_decode_equal_the_two_calls(dev, rows, H, C, bias, n, emit_off, special):
    from ndcn_amd import hip
    y, fs = kernel_inputs(rows, H, n, special, dev)
    a = ab.weights(n)
    dt = np.float32(0.1)
    Wd, bd = make_decoder(H, C, bias, dev)
    state = hip.ab_step(y, fs, a, dt)
    tick = hip.tick_emit(state, dt, [emit_off])[0] if emit_off != 0 else state
    ref = hip.linear(tick, Wd, bd)
    rc, out, dec = run_fused(y, fs, a, dt, Wd, bd, emit_off)
    torch.cuda.synchronize()
    assert rc == 0
    assert same_words(out, state) and same_words(dec, ref)
    if special:
        r = rows - 1
        # the STORED state keeps -0.0 and Inf; the decoded tick of a step's inside sees +0.0 and NaN
        assert out[r, 0].item() == 0 and np.signbit(out[r, 0].item()) and out[r, H - 1].item() == float('inf')
        if emit_off != 0:
            assert bool(torch.isnan(dec[r]).all())                                    # Inf became NaN before the decoder
        else:
            assert bool(torch.isinf(dec[r]).all())
    # in place: out == y is allowed
    y2 = y.clone()
    rc, out2, dec2 = run_fused(y2, fs, a, dt, Wd, bd, emit_off, out=y2)
    torch.cuda.synchronize()
    assert rc == 0 and same_words(y2, state) and same_words(dec2, ref)


@pytest.mark.parametrize('H', [20, 68])
def test_kernel_against_the_numpy_order_of_operations(dev, H):
    """the composed restatement (tests/_adams_readout.py over _adams_bashforth and _readout_chain), with and without an inside tick"""
    rows, C, n = 65, 5, 7
    y, fs = kernel_inputs(rows, H, n, False, dev)
    a = ab.weights(n)
    dt = np.float32(0.1)
    Wd, bd = make_decoder(H, C, True, dev)
    for off in (0., .03):
        rc, out, dec = run_fused(y, fs, a, dt, Wd, bd, off)
        torch.cuda.synchronize()
        want_state, want_dec = aro.step_readout(y.cpu().numpy(), [f.cpu().numpy() for f in fs], a, dt, Wd.cpu().numpy(), bd.cpu().numpy(), off)
        assert rc == 0
        assert np.array_equal(out.cpu().numpy().view(np.int32), want_state.view(np.int32))
        assert np.array_equal(dec.cpu().numpy().view(np.int32), want_dec.view(np.int32))


def test_kernel_refuses_before_any_launch(dev):
    """NDCN_EINVAL for C outside 1..15, H outside the two sets, n outside 3..11, a null panel, out aliasing a history panel"""
    from ndcn_amd import _lib
    lib = _lib.load()
    y, fs = kernel_inputs(5, 20, 3, False, dev)
    Wd, bd = make_decoder(516, 16, True, dev)                                         # (room for every H and C the calls name)
    out, dec = torch.full((5, 516), 7., device=dev), torch.full((5, 16), 7., device=dev)
    big = [torch.zeros(5, 516, device=dev) for _ in range(3)]

    def call(H=20, C=1, n=3, fs_=big, out_=out, y_=big[0], Wd_=Wd, dec_=dec):
        arr_f = (ctypes.c_void_p * len(fs_))(*[None if f is None else f.data_ptr() for f in fs_])
        arr_a = (ctypes.c_float * 12)(*([.1] * 12))
        return lib.ndcn_ab_step_readout_f32(_lib.ptr(out_), _lib.ptr(y_), arr_f, arr_a, n, .1, 5, H, _lib.ptr(Wd_), _lib.ptr(bd), C,
                                            _lib.ptr(dec_), 0., _lib.stream_ptr())
    for H in (12, 18, 62, 516):
        assert call(H=H) == _lib.EINVAL, H
    for C in (0, 16):
        assert call(C=C) == _lib.EINVAL, C
    assert call(n=2, fs_=big[:2]) == _lib.EINVAL and call(n=12, fs_=big * 4) == _lib.EINVAL
    assert call(fs_=[big[0], None, big[2]]) == _lib.EINVAL                            # a null panel
    assert call(y_=None) == _lib.EINVAL and call(Wd_=None) == _lib.EINVAL and call(dec_=None) == _lib.EINVAL and call(out_=None) == _lib.EINVAL
    assert call(out_=big[1]) == _lib.EINVAL                                           # out aliases a history panel
    torch.cuda.synchronize()
    assert bool((out == 7.).all()) and bool((dec == 7.).all())                        # nothing was launched
    assert call(y_=y, fs_=fs) == 0                                                    # (the same call with admissible arguments runs)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- 2. whole solves
_OPS = {}
RECTS = {63: (7, 9), 64: (8, 8), 130: (10, 13)}


def make_func(rows, H, dev, no_control=False, seed=0):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    if rows not in _OPS:
        _OPS[rows] = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor_rect(*RECTS[rows])), dev)
    torch.manual_seed(seed)
    f = ODEFunc(H, _OPS[rows], no_control=no_control).to(dev).eval()
    x0 = torch.rand(rows, H, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    return f, x0


def both(f, x0, t, Wd, bd, method, options, capfd, **kw):
    """(decoded inside the solve, route bits, step log, stderr) and (hip.linear of the switch-off trajectory, its log, its stderr)"""
    from ndcn_amd import hip
    from ndcn_amd import torchdiffeq as ode
    res = []
    for on in (1, 0):
        hip.set_adams_readout(on)
        log = []
        capfd.readouterr()
        with torch.no_grad():
            if on:
                y = ode.odeint(f, x0, t, method=method, options=dict(options) if options else None, readout=(Wd, bd), step_log=log, **kw)
                bits = path()
            else:
                y = hip.linear(ode.odeint(f, x0, t, method=method, options=dict(options) if options else None, step_log=log, **kw), Wd, bd)
        torch.cuda.synchronize()
        res.append((y, log, capfd.readouterr().err))
    hip.set_adams_readout(-1)
    return res[0], bits, res[1]


# h = 1/8 is exact in float32: the grid is 0, .125, .. 1.  Step 0 ends at the tick .125, step 1 (a warm-up step) holds .2 inside, step 3
# = [.375, .5] holds .4 and .45 inside and ends at the tick .5, step 4 ends at the tick .625, steps 5 and 6 hold none, step 7 holds .9
# inside and ends at the last tick
SUB_T = [0., .125, .2, .4, .45, .5, .625, .9, 1.]
OPTION_CASES = [('default', None), ('max_order_4', {'max_order': 4}), ('step_size', {'step_size': .125}), ('max_order_2', {'max_order': 2}),
                ('max_order_3', {'max_order': 3})]


def test_the_step_size_grid_has_the_shape_the_cases_rely_on():
    from ndcn_amd.torchdiffeq._impl import core
    plan = core.fixed_plan(np.asarray(SUB_T, np.float32), .125)
    steps = [int(s) for s in plan.tick_step[1:]]
    same = [bool(c) for c in plan.tick_coincident[1:]]
    assert steps == [0, 1, 3, 3, 3, 4, 7, 7] and same == [True, False, False, False, True, True, False, True]


@pytest.mark.parametrize('rows', [63, 64, 130])
@pytest.mark.parametrize('H', [20, 64])
@pytest.mark.parametrize('method', ['explicit_adams', 'fixed_adams'])
@pytest.mark.parametrize('case,options', OPTION_CASES, ids=[c for c, _ in OPTION_CASES])
def test_solves_equal_decode_after(dev, capfd, rows, H, method, case, options):
    f, x0 = make_func(rows, H, dev)
    Wd, bd = make_decoder(H, 3, True, dev)
    t = torch.tensor(SUB_T) if case == 'step_size' else torch.linspace(0., 1.5, 16)
    kw = dict(rtol=1e-3, atol=1e-4) if method == 'fixed_adams' else {}
    (got, la, ea), bits, (ref, lb, eb) = both(f, x0, t.to(dev), Wd, bd, method, options, capfd, **kw)
    assert got.shape == (len(t), rows, 3) and same_words(got, ref)
    assert la == lb and ea == eb
    warm_only = case in ('max_order_2', 'max_order_3')
    if method == 'fixed_adams' or warm_only:
        assert bits == FIXED, bits
    else:
        assert bits == (ADAMS | FIXED | (NARROW if H < 64 else 0)), bits               # (FIXED: the two warm-up steps' ticks)


def test_implicit_false_is_explicit_adams_with_the_decoder(dev, capfd):
    f, x0 = make_func(130, 20, dev)
    Wd, bd = make_decoder(20, 3, True, dev)
    t = torch.linspace(0., 1.5, 16).to(dev)
    (got, _, _), bits, (ref, _, _) = both(f, x0, t, Wd, bd, 'fixed_adams', {'implicit': False}, capfd)
    (exp, _, _), bits_e, _ = both(f, x0, t, Wd, bd, 'explicit_adams', None, capfd)
    assert bits == bits_e == ADAMS | FIXED | NARROW
    assert same_words(got, ref) and same_words(got, exp)


@pytest.mark.parametrize('H', [20, 64])
def test_fixed_adams_iterations_and_warnings_are_those_of_the_plain_solve(dev, capfd, H):
    from ndcn_amd.torchdiffeq._impl import core
    f, x0 = make_func(130, H, dev)
    Wd, bd = make_decoder(H, 3, True, dev)
    t = torch.linspace(0., 1.5, 16).to(dev)
    # tolerances below the first correction's change: several iterations on some step
    (got, la, ea), bits, (ref, lb, eb) = both(f, x0, t, Wd, bd, 'fixed_adams', None, capfd, rtol=1e-6, atol=1e-7)
    its = [r[0] for r in la if r[0] != 'nfe']
    print('iterations per step', its)
    assert max(its) > 1 and same_words(got, ref) and la == lb and ea == eb and bits == FIXED
    # one iteration allowed, tolerances it cannot meet: steps that do not converge drop their oldest evaluation and warn
    (got, la, ea), bits, (ref, lb, eb) = both(f, x0, t, Wd, bd, 'fixed_adams', {'max_iters': 1}, capfd, rtol=1e-9, atol=1e-12)
    conv = [r[1] for r in la if r[0] != 'nfe']
    assert not all(conv) and ea.count(core.NOT_CONVERGED) == conv.count(False) > 0
    assert same_words(got, ref) and la == lb and ea == eb and bits == FIXED


def test_non_finite_states_decode_to_the_same_words(dev, capfd):
    f, x0 = make_func(130, 20, dev)
    x0 = x0.clone()
    x0[129, 3] = float('nan')
    x0[64, 19] = float('inf')
    Wd, bd = make_decoder(20, 3, True, dev)
    for t, options in ((torch.linspace(0., 1.5, 16), None), (torch.tensor(SUB_T), {'step_size': .125})):
        (got, _, _), bits, (ref, _, _) = both(f, x0, t.to(dev), Wd, bd, 'explicit_adams', options, capfd)
        assert bits & ADAMS and not torch.isfinite(ref).all() and torch.isfinite(ref).any()
        assert same_words(got, ref)


# ---------------------------------------------------------------------------------------------------------- 3. route
def test_ndcn_forward_takes_the_fused_step(dev):
    """fails without the feature: the route word stays 0 there"""
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import NDCN
    torch.manual_seed(0)
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(12)), dev)
    m = NDCN(input_size=1, hidden_size=20, A=A, num_classes=1, method='explicit_adams').to(dev).eval()
    x = torch.rand(144, 1, generator=torch.Generator().manual_seed(1)).to(dev)
    vt = torch.linspace(0., 1., 12).to(dev)
    with torch.no_grad():
        got = m(vt, x)
        bits = path()
        ref = m.output_layer(m.neural_dynamic_layer(vt, m.input_layer(x)))
    assert bits & ADAMS and bits & NARROW, bits
    assert got.shape == (12, 144, 1) and same_words(got, ref)


@pytest.mark.parametrize('H,C,no_control', [(24, 16, False), (20, 3, True), (22, 3, False)])
def test_shapes_and_operators_without_a_form_decode_after(dev, capfd, H, C, no_control):
    f, x0 = make_func(130, H, dev, no_control=no_control)
    Wd, bd = make_decoder(H, C, True, dev)
    t = torch.linspace(0., 1.5, 16).to(dev)
    for method in ('explicit_adams', 'fixed_adams'):
        kw = dict(rtol=1e-3, atol=1e-4) if method == 'fixed_adams' else {}
        (got, la, ea), bits, (ref, lb, eb) = both(f, x0, t, Wd, bd, method, None, capfd, **kw)
        assert bits == 0 and same_words(got, ref) and la == lb and ea == eb


def test_a_gradient_keeps_decode_after(dev):
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd import _lib
    f, x0 = make_func(130, 20, dev)
    Wd, bd = make_decoder(20, 3, True, dev)
    Wd.requires_grad_(True)
    t = torch.linspace(0., 1.5, 16).to(dev)
    _lib.load().ndcn_clear_readout_path()
    for p in f.parameters():
        p.requires_grad_(False)
    out = ode.odeint(f, x0, t, method='explicit_adams', readout=(Wd, bd))
    assert path() == 0 and out.requires_grad


# ---------------------------------------------------------------------------------------------------------- 4. memory
@pytest.mark.parametrize('method', ['explicit_adams', 'fixed_adams'])
def test_peak_memory_does_not_grow_with_the_hidden_trajectory(dev, method):
    """N = 4096, H = 64, C = 1: the peak of a solve over 40 ticks minus that over 10 ticks stays below half of what 30 more hidden
    panels take - the expected growth is the (T, N, C) output alone.  A condition; fails without the feature (the growth is the
    trajectory's)."""
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    from ndcn_amd import torchdiffeq as ode
    N, H = 4096, 64
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(64)), dev)
    torch.manual_seed(0)
    f = ODEFunc(H, A).to(dev).eval()
    x0 = torch.rand(N, H, generator=torch.Generator().manual_seed(1)).to(dev)
    Wd, bd = make_decoder(H, 1, True, dev)
    kw = dict(rtol=1e-3, atol=1e-4) if method == 'fixed_adams' else {}
    peaks = {}
    with torch.no_grad():
        ode.odeint(f, x0, torch.linspace(0., .1, 3).to(dev), method=method, readout=(Wd, bd), **kw)      # plans built before measuring
        for T in (10, 40):
            t = (torch.arange(T) * .02).to(dev)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            y = ode.odeint(f, x0, t, method=method, readout=(Wd, bd), **kw)
            bits = path()
            torch.cuda.synchronize()
            peaks[T] = torch.cuda.max_memory_allocated(dev) - base
            assert y.shape == (T, N, 1) and bool(torch.isfinite(y).all())
            assert bits == (FIXED if method == 'fixed_adams' else ADAMS | FIXED), bits
            del y
    growth, hidden = peaks[40] - peaks[10], 30 * N * H * 4
    print('%s: peak %d B at 10 ticks, %d B at 40: growth %d B, the hidden trajectory would grow by %d B' % (method, peaks[10], peaks[40], growth, hidden))
    assert growth < hidden / 2
