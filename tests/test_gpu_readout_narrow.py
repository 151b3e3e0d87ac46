"""Inference with the decoder inside the solve at the narrow widths (H = 16, 20, .. 60: the drivers' defaults) on a real MI355X.
There ndcn_linear_f32 runs one in-order fma chain per (row, output) (linear_small_kernel), and the fused dense-output kernel for
those widths (rk.hip readout_narrow_kernel: a workgroup per tile of 64 rows) keeps that order, so every comparison is torch.equal
against the un-fused pair `hip.linear(odeint(f, x0, t, ...), Wd, bd)`.  ndcn_last_readout_path() proves which route ran
(1: a fused dense-output kernel, 8 beside it: the narrow one, 2: a tick staged through the scratch, 4: fixed-grid per-step decode,
0: the two-step fallback).  The helpers follow tests/test_gpu_readout.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FUSED, STAGED, FIXED, NARROW = 1, 2, 4, 8


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


_OPS = {}


def lattice(S, dev):
    from ndcn_amd import graphs
    if S not in _OPS:
        _OPS[S] = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(S)), dev)
    return _OPS[S]


def make_func(S, H, dev, variant='default', seed=0):
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(seed)
    f = ODEFunc(H, lattice(S, dev), no_graph=variant == 'no_graph', no_control=variant == 'no_control').to(dev).eval()
    x0 = torch.rand(S * S, H, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    return f, x0


def make_decoder(H, C, bias, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    Wd = ((torch.rand(C, H, generator=g) - .5) * (2. / H ** .5)).to(dev)
    bd = (torch.rand(C, generator=g) - .5).to(dev) if bias else None
    return Wd, bd


def path():
    from ndcn_amd import _lib
    return int(_lib.load().ndcn_last_readout_path())


def clear_path():
    from ndcn_amd import _lib
    _lib.load().ndcn_clear_readout_path()


def both(f, x0, t, Wd, bd, **kw):
    """(fused, its step log, route bits, two-step, its step log) under no_grad"""
    from ndcn_amd import hip
    from ndcn_amd import torchdiffeq as ode
    la, lb = [], []
    with torch.no_grad():
        got = ode.odeint(f, x0, t, readout=(Wd, bd), step_log=la, **kw)
        bits = path()
        ref = hip.linear(ode.odeint(f, x0, t, step_log=lb, **kw), Wd, bd)
    return got, la, bits, ref, lb


def ticks_per_step(log, ticks):
    """how many of `ticks` (after the first) each accepted step of a dopri5 log covers, as the solver assigns them"""
    counts, j = [], 1
    for t0, dt, ok, _, _ in (r for r in log if len(r) == 5):
        if not ok:
            continue
        n = 0
        while j < len(ticks) and not ticks[j] > t0 + dt:
            j += 1
            n += 1
        counts.append(n)
    return counts


def one_launch(f, H, method):
    """does the one-launch solve (ndcn_solve_small_f32) take this state?"""
    from ndcn_amd import _lib
    from ndcn_amd.csr import as_csr
    flags = _lib.F_RELU | (_lib.F_NO_GRAPH if f.no_graph else 0) | (_lib.F_NO_CONTROL if f.no_control else 0)
    return int(_lib.load().ndcn_solve_small_supported(as_csr(f.A).view_ref(), H, flags, _lib.METHODS[method], 0))


def solver_pair(f, x0, method, ticks, Wd, bd, **kw):
    """(accepted?, fused (T, N, C) or None, route bits, two-step (T, N, C)) through DeviceSolver directly"""
    from ndcn_amd import hip
    from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver
    n, H = x0.shape
    C = Wd.shape[0]
    s = DeviceSolver(f, n, method, **kw)
    try:
        hidden = torch.empty((len(ticks), n, H), device=x0.device)
        s.begin(x0, 0.)
        s.advance_many(ticks, hidden)
        ref = hip.linear(hidden, Wd, bd)
        out = torch.full((len(ticks), n, C), 7., device=x0.device)
        scratch = torch.empty((2, n, H), device=x0.device)
        s.begin(x0, 0.)
        ok = s.advance_many_readout(ticks, Wd, bd, out, scratch)
        bits = path()
        torch.cuda.synchronize()
    finally:
        s.close()
    return ok, out, bits, ref


# ---------------------------------------------------------------------------------------------------------- 1. dopri5, fused route
DOPRI5_CASES = [(16, 1, True, 'default'), (20, 1, True, 'default'), (20, 3, False, 'default'), (32, 15, True, 'default'),
                (60, 15, True, 'default'), (20, 3, False, 'no_control'), (36, 1, True, 'no_graph')]


@pytest.mark.parametrize('H,C,bias,variant', DOPRI5_CASES, ids=lambda v: str(v))
def test_dopri5_narrow_fused_readout_equals_the_two_step_form(dev, H, C, bias, variant):
    """33 x 33 lattice: 1089 rows = 17 tiles of 64 and one more row, so the last tile holds a single live row; 1 to 4 quads per
    thread (H = 16; 20, 32; 36; 60), one to four chains per lane (C = 1, 3, 15).  (a) 23 ticks over [0, 5]: some accepted step
    covers more than 8 of them - two launches; (b) [0, 5]: steps without ticks, the last tick strictly inside the final step;
    (c) the last tick exactly at the end of an accepted step of (a)."""
    f, x0 = make_func(33, H, dev, variant)
    Wd, bd = make_decoder(H, C, bias, dev)
    kw = dict(rtol=.01, atol=.001, method='dopri5')
    ta = torch.linspace(0., 5., 23)
    got, la, bits, ref, lb = both(f, x0, ta.to(dev), Wd, bd, **kw)
    per = ticks_per_step(la, ta.double().tolist())
    print('(a) ticks per accepted step', per, 'path', bits)
    assert bits & FUSED and bits & NARROW, bits
    assert got.shape == (23, 1089, C) and torch.equal(got, ref) and la == lb
    assert max(per) > 8 and sum(per) == 22, per

    got, l2, bits, ref, lb = both(f, x0, torch.tensor([0., 5.]).to(dev), Wd, bd, **kw)
    steps = [r for r in l2 if len(r) == 5 and r[2]]
    print('(b) accepted steps', len(steps), 'last', steps[-1][:2], 'path', bits)
    assert torch.equal(got, ref) and l2 == lb and bits & FUSED and bits & NARROW
    assert len(steps) > 1 and steps[-1][0] < 5. < steps[-1][0] + steps[-1][1]

    acc = [r for r in la if len(r) == 5 and r[2]]
    end = acc[1][0] + acc[1][1]                              # the fp64 sum the solver forms for t1
    tc = torch.tensor([0., acc[0][0] + .5 * acc[0][1], .5 * (acc[1][0] + end), end], dtype=torch.float64)
    got, l3, bits, ref, lb = both(f, x0, tc.to(dev), Wd, bd, **kw)
    print('(c) ticks', tc.tolist(), 'path', bits)
    assert torch.equal(got, ref) and l3 == lb and bits & FUSED and bits & NARROW
    assert [r[:2] for r in l3 if len(r) == 5 and r[2]][-1] == acc[1][:2]       # the solve ended with that step: no step beyond the tick


# ---------------------------------------------------------------------------------------------------------- 2. tiny row counts
@pytest.mark.parametrize('n', [1, 5])
def test_tiny_row_counts_without_a_graph(dev, n):
    """one tile with 1 or 5 live rows, all four chains per lane.  rk4: a state this small at H <= 64 is the one-launch solve's
    (asserted), and ndcn_solver_advance_many_readout declines those at every width - at H = 20 as it does at H = 64
    (test_gpu_readout.py test_the_one_launch_state_declines) - so no tiny state reaches the per-step decode at these widths"""
    from ndcn_amd import _lib
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(3)
    f = ODEFunc(20, None, no_graph=True).to(dev).eval()
    x0 = torch.rand(n, 20, generator=torch.Generator().manual_seed(4)).to(dev)
    Wd, bd = make_decoder(20, 15, True, dev)
    ok, out, bits, ref = solver_pair(f, x0, 'dopri5', [.3, .6, 1.], Wd, bd, rtol=.01, atol=.001)
    assert ok and bits == FUSED | NARROW and torch.equal(out, ref)
    assert _lib.load().ndcn_solve_small_supported(_lib.empty_csr(n), 20, _lib.F_RELU | _lib.F_NO_GRAPH, _lib.M_RK4, 0) == 1
    ok, out, bits, ref = solver_pair(f, x0, 'rk4', [.3, .6, 1.], Wd, bd)
    assert not ok and bits == 0 and bool((out == 7.).all())


# ---------------------------------------------------------------------------------------------------------- 3. stored fit
def test_a_tick_under_a_stored_fit_is_staged_through_the_scratch(dev):
    """two single-tick evaluations inside one accepted step leave a stored fit (ndcn_solver_advance); the next tick of that step has
    no fresh step to read and goes through the scratch panel, the one after it through the narrow fused kernel"""
    from ndcn_amd import hip
    from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver
    f, x0 = make_func(33, 20, dev)
    Wd, bd = make_decoder(20, 3, True, dev)
    s = DeviceSolver(f, 1089, 'dopri5', rtol=.01, atol=.001)
    try:
        res = []
        for fused in (False, True):
            s.begin(x0, 0.)
            tmp = torch.empty(2, 1089, 20, device=dev)
            assert s.advance(2.0, tmp[0]) and s.advance(2.001, tmp[1])
            if fused:
                out = torch.empty(2, 1089, 3, device=dev)
                assert s.advance_many_readout([2.002, 4.9], Wd, bd, out, torch.empty(2, 1089, 20, device=dev))
                bits = path()
            else:
                hidden = torch.empty(2, 1089, 20, device=dev)
                s.advance_many([2.002, 4.9], hidden)
                out = hip.linear(hidden, Wd, bd)
            res.append((out, s.steplog()))
        torch.cuda.synchronize()
    finally:
        s.close()
    assert bits == STAGED | FUSED | NARROW, bits
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]


# ---------------------------------------------------------------------------------------------------------- 4. fixed grids
@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4'])
def test_fixed_grid_readout_equals_the_two_step_form(dev, method):
    """65 x 65 lattice (4225 rows, 338 KB of state): beyond the one-launch solve, so each step's state is decoded by ndcn_linear_f32"""
    f, x0 = make_func(65, 20, dev)
    assert one_launch(f, 20, method) == 0
    Wd, bd = make_decoder(20, 3, True, dev)
    for t in (torch.linspace(0., 1., 9), torch.tensor([0., .05, .3, .35, .8, 1.])):
        got, _, bits, ref, _ = both(f, x0, t.to(dev), Wd, bd, method=method)
        assert got.shape == (len(t), 4225, 3) and torch.equal(got, ref) and bits == FIXED, bits


# ---------------------------------------------------------------------------------------------------------- 5. non-finite values
def test_non_finite_states_decode_to_the_same_bits(dev):
    """a NaN in the last row - the only live row of the last tile of 64 (4225 = 66 * 64 + 1) - and an Inf in column H - 1 of y0 (fixed
    grid: no step assertion fires): equal as bit patterns, non-finite ones included"""
    f, x0 = make_func(65, 20, dev)
    x0 = x0.clone()
    x0[4224, 3] = float('nan')
    x0[500, 19] = float('inf')
    Wd, bd = make_decoder(20, 3, True, dev)
    for method in ('euler', 'rk4'):
        assert one_launch(f, 20, method) == 0
        ok, out, bits, ref = solver_pair(f, x0, method, [.1, .2, .3], Wd, bd)
        assert ok and bits == FIXED
        assert not torch.isfinite(ref).all() and torch.isfinite(ref).any()
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- 6. declines
@pytest.mark.parametrize('H,C', [(12, 1), (18, 1), (62, 1), (20, 16)])
def test_shapes_outside_both_routes_decline(dev, H, C):
    from ndcn_amd import _lib
    f, x0 = make_func(33, H, dev)
    Wd, bd = make_decoder(H, C, True, dev)
    ok, out, bits, _ = solver_pair(f, x0, 'dopri5', [.5, 1.], Wd, bd, rtol=.01, atol=.001)
    assert not ok and bits == 0 and bool((out == 7.).all())                 # NDCN_EINVAL, nothing written
    assert 'row-dot' in _lib.load().ndcn_last_error().decode()
    t = torch.tensor([0., .5, 1.]).to(dev)
    got, la, bits, ref, lb = both(f, x0, t, Wd, bd, rtol=.01, atol=.001, method='dopri5')
    assert torch.equal(got, ref) and la == lb and bits == 0


# ---------------------------------------------------------------------------------------------------------- 7. NDCN.forward
def test_ndcn_forward_decodes_inside_the_solve(dev):
    from ndcn_amd.neural_dynamics import NDCN
    torch.manual_seed(0)
    m = NDCN(input_size=1, hidden_size=20, A=lattice(33, dev), num_classes=1, rtol=.01, atol=.001, method='dopri5').to(dev).eval()
    x = torch.rand(1089, 1, generator=torch.Generator().manual_seed(1)).to(dev)
    vt = torch.linspace(0., 5., 12).to(dev)
    with torch.no_grad():
        got = m(vt, x)
        bits = path()
        ref = m.output_layer(m.neural_dynamic_layer(vt, m.input_layer(x)))
    assert bits & FUSED and bits & NARROW, bits
    assert got.shape == (12, 1089, 1) and torch.equal(got, ref)
    clear_path()
    out = m(vt, x)                                           # grad enabled: the parameters ask for one - the two-step form
    assert path() == 0 and out.requires_grad and torch.equal(out.detach(), ref)


# ---------------------------------------------------------------------------------------------------------- 8. memory
def _big(dev, method, S, H):
    from ndcn_amd.neural_dynamics import NDCN
    from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver
    torch.manual_seed(0)
    m = NDCN(input_size=1, hidden_size=H, A=lattice(S, dev), num_classes=1, rtol=.01, atol=.001, method=method).to(dev).eval()
    x = torch.rand(S * S, 1, generator=torch.Generator().manual_seed(1)).to(dev)
    f = m.neural_dynamic_layer.odefunc
    s = DeviceSolver(f, S * S, method, rtol=.01, atol=.001)
    ws = s.workspace.numel()
    s.close()
    return m, x, f, ws


@pytest.mark.parametrize('method', ['dopri5', 'rk4'])
def test_inference_memory_does_not_grow_with_the_ticks(dev, method):
    """650 x 650 lattice, H = 20: 34 MB panels, N H > 2^23 (no per-step hipGraph: the eager form); T = 24, C = 1.  Conditions, not
    measurements - the bounds of the H = 128 test (tests/test_gpu_readout.py): the two-step form holds at least T = 24 hidden panels;
    with the decoder inside the solve the peak stays below the solver's workspace + 4 panels (2 of scratch, 2 of slack) + the output
    for odeint, + 8 panels + the output for NDCN.forward (its encoder's intermediates)"""
    from ndcn_amd import torchdiffeq as ode
    S, T, H = 650, 24, 20
    m, x, f, ws = _big(dev, method, S, H)
    N = S * S
    panel, out_bytes = N * H * 4, T * N * 4
    assert N * H > 1 << 23
    want = (FUSED | NARROW) if method == 'dopri5' else FIXED
    vt = torch.linspace(0., 5., T).to(dev)
    Wd, bd = m.output_layer.weight.detach(), m.output_layer.bias.detach()
    kw = dict(rtol=.01, atol=.001, method=method)
    with torch.no_grad():
        h0 = m.input_layer(x)
        ode.odeint(f, h0, vt[:2], readout=(Wd, bd), **kw)                      # operator plans, weight packs: built before measuring
        m(vt[:2], x)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        y = ode.odeint(f, h0, vt, readout=(Wd, bd), **kw)
        bits = path()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - base
        print('%s odeint(readout): peak %.1f MB = %.2f panels beyond the workspace (%.1f MB) and the output; bound 4'
              % (method, peak / 2 ** 20, (peak - ws - out_bytes) / panel, ws / 2 ** 20))
        assert y.shape == (T, N, 1) and bool(torch.isfinite(y).all()) and (bits & want) == want, bits
        assert peak < ws + 4 * panel + out_bytes
        del y, h0
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        y = m(vt, x)
        bits = path()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - base
        print('%s NDCN.forward: peak %.1f MB = %.2f panels beyond the workspace and the output; bound 8'
              % (method, peak / 2 ** 20, (peak - ws - out_bytes) / panel))
        assert y.shape == (T, N, 1) and bool(torch.isfinite(y).all()) and (bits & want) == want, bits
        assert peak < ws + 8 * panel + out_bytes
