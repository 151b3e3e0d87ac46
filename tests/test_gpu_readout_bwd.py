"""Fixed-grid training with the decoder inside the solve (ABI 27): ndcn_readout_bwd_f32 against its numpy restatement
(tests/_readout_chain.py), ndcn_fixed_grid_backward_readout_f32 bit for bit against ndcn_fixed_grid_backward_f32 on the materialised
gradient, odeint(..., readout=) under a gradient against the two-step form and float64 autograd through the oracle's fixed-grid solve,
the routing, an NDCN Adam step, and the peak memory of one step."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _philox
from _readout_chain import combine, decoder_sums, tick_gradient
from oracle import ndcn_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need a ROCm device'
    return torch.device('cuda:0')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# --------------------------------------------------------------------------------------------------- 1. the kernel

_KERNEL_NS = (1, 31, 257, 1000)


@pytest.fixture(scope='module')
def kernel_inputs():
    """per (H, C): gd, Wd, y, base and five addends at the largest N (the smaller N are its leading rows), made once"""
    made = {}

    def get(H, C):
        if (H, C) not in made:
            rng = np.random.RandomState(1000 * H + C)
            N = max(_KERNEL_NS)
            f = lambda *s: (rng.randn(*s) * 2.0 ** rng.randint(-6, 6, s)).astype(np.float32)
            made[(H, C)] = dict(gd=f(N, C), Wd=f(C, H), y=f(N, H), base=f(N, H), adds=[f(N, H) for _ in range(5)])
        return made[(H, C)]
    return get


@pytest.mark.parametrize('C', [1, 2, 15])
@pytest.mark.parametrize('H', [1, 20, 64, 252, 256])
def test_kernel_against_numpy(dev, kernel_inputs, H, C):
    """out bit for bit the fma chain and rk_combine's unit-coefficient order; g_Wd / g_bd within one fp32 rounding of the float64
    sums plus 1e-12 of the magnitudes that enter them.  H = 1 / 20 / 252: a lane count that does not divide the block (tail lanes
    idle), H = 252 / 256: 16-byte lanes, H = 1: the scalar path; N = 1 .. 1000: one row, a partial block, several blocks with a
    masked tail.  The accumulator carries over the calls of one (H, C): it is checked as the running sum."""
    from ndcn_amd import hip
    d = kernel_inputs(H, C)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    acc = torch.zeros(C * H + C, dtype=torch.float64, device=dev)
    ref_W, ref_b, mag_W, mag_b = np.zeros((C, H)), np.zeros(C), np.zeros((C, H)), np.zeros(C)
    for N in _KERNEL_NS:
        gd, y, Wd = d['gd'][:N], d['y'][:N], d['Wd']
        gi = tick_gradient(gd, Wd)
        for with_base in (False, True):
            for n_add in (0, 1, 5):
                adds = [a[:N] for a in d['adds'][:n_add]]
                got = hip.readout_bwd(T(gd), T(Wd), y=T(y), base=T(d['base'][:N]) if with_base else None, addends=[T(a) for a in adds],
                                      acc=acc)
                want = combine(gi, d['base'][:N] if with_base else None, adds)
                assert got.shape == (N, H) and np.array_equal(bits(got.cpu().numpy()), bits(want)), (N, with_base, n_add)
                s = decoder_sums(gd, y)
                ref_W += s[0]; ref_b += s[1]; mag_W += s[2]; mag_b += s[3]
    f = acc.to(torch.float32).cpu().numpy().astype(np.float64)
    err_W, err_b = np.abs(f[:C * H].reshape(C, H) - ref_W), np.abs(f[C * H:] - ref_b)
    bound_W, bound_b = 2.0 ** -23 * np.abs(ref_W) + 1e-12 * mag_W, 2.0 ** -23 * np.abs(ref_b) + 1e-12 * mag_b
    print('H %d C %d: worst g_Wd error / bound %.3f, g_bd %.3f' % (H, C, float((err_W / bound_W).max()), float((err_b / bound_b).max())))
    assert np.all(err_W <= bound_W) and np.all(err_b <= bound_b)
    # without an accumulator nothing but `out` is touched, and the result is the same
    again = hip.readout_bwd(T(d['gd']), T(d['Wd']), base=T(d['base']), addends=[T(d['adds'][0])])
    assert np.array_equal(bits(again.cpu().numpy()), bits(combine(tick_gradient(d['gd'], d['Wd']), d['base'], [d['adds'][0]])))


def test_kernel_nan_stays_in_its_row_and_wide_decoders_are_refused(dev, kernel_inputs):
    from ndcn_amd import _lib, hip
    d = kernel_inputs(64, 2)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gd = d['gd'][:257].copy()
    gd[100, 1] = np.nan
    out = hip.readout_bwd(T(gd), T(d['Wd']), base=T(d['base'][:257]), addends=[T(d['adds'][0][:257])]).cpu().numpy()
    bad = np.isnan(out)
    assert bad[100].all() and not np.delete(bad, 100, axis=0).any()
    # C = 16: NDCN_EINVAL from the entry point itself
    lib = _lib.load()
    gd16, W16, o = torch.zeros(8, 16, device=dev), torch.zeros(16, 64, device=dev), torch.zeros(8, 64, device=dev)
    arr = (ctypes.c_void_p * 1)()
    rc = lib.ndcn_readout_bwd_f32(_lib.ptr(o), None, arr, 0, _lib.ptr(gd16), _lib.ptr(W16), None, 8, 64, 16, None, None, _lib.stream_ptr())
    assert rc == _lib.EINVAL
    assert lib.ndcn_readout_bwd_f32(_lib.ptr(o), None, arr, 0, _lib.ptr(gd16), _lib.ptr(W16), None, 8, 64, 0, None, None,
                                    _lib.stream_ptr()) == _lib.EINVAL
    with pytest.raises(_lib.NdcnHipError):
        hip.readout_bwd(gd16, W16)


# --------------------------------------------------------------------------------------------------- 2. the library sweep

def _operator(shape):
    from ndcn_amd import graphs
    if shape == 'lattice':
        return graphs.normalized_laplacian(graphs.grid_8_neighbor_rect(37, 29)).tocsr(), 64
    return graphs.normalized_laplacian(graphs.make_graph('random', 300, seed=0)).tocsr(), 20


@pytest.fixture(scope='module')
def sweep_case(dev):
    """per (shape, variant, method): the operator, weights and the forward trajectory, made once"""
    from ndcn_amd import _lib, graphs
    from ndcn_amd.torchdiffeq._impl import fixed_train
    made = {}

    def get(shape, variant, method):
        key = (shape, variant, method)
        if key not in made:
            L, H = _operator(shape)
            n = L.shape[0]
            flags = _lib.F_RELU | (_lib.F_NO_GRAPH if variant == 'no_graph' else 0) | (_lib.F_NO_CONTROL if variant == 'no_control' else 0)
            csr = None
            if variant != 'no_graph':
                csr = graphs.to_device(L, dev)
                csr.ensure_plans(H)
                csr.transpose().ensure_plans(H)
            g = torch.Generator().manual_seed(3)
            W = ((torch.rand(H, H, generator=g) - 0.5) * (2.0 / H ** 0.5)).to(dev)
            b = ((torch.rand(H, generator=g) - 0.3) * 0.2).to(dev)
            y0 = torch.rand(n, H, generator=g).to(dev)
            dts = [0.25, 0.125, 0.25, 0.5, 0.125]
            out, arr = fixed_train._fixed_grid_train(y0, W, b, csr, flags, method, dts)
            made[key] = (csr, flags, W, b, out, arr, len(dts))
        return made[key]
    return get


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('variant', ['default', 'no_control', 'no_graph'])
@pytest.mark.parametrize('shape', ['lattice', 'random300'])
def test_library_sweep_equals_its_partner_on_the_materialised_gradient(dev, sweep_case, shape, variant, method, C):
    """ndcn_fixed_grid_backward_readout_f32 on g_dec against ndcn_fixed_grid_backward_f32 on g = chain(g_dec, Wd) formed on the host:
    g_y0, g_W and g_b bit for bit; the decoder's gradients against the float64 sums over all ticks."""
    from ndcn_amd.torchdiffeq._impl import fixed_train
    csr, flags, W, b, out, arr, n_ticks = sweep_case(shape, variant, method)
    n, H = out.shape[1], out.shape[2]
    rng = np.random.RandomState(7 + C)
    g_dec = rng.randn(n_ticks + 1, n, C).astype(np.float32)
    Wd = (rng.randn(C, H) / H ** 0.5).astype(np.float32)
    g = np.stack([tick_gradient(g_dec[i], Wd) for i in range(n_ticks + 1)])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    a = fixed_train._fixed_grid_reverse(out, W, b, csr, flags, method, arr, n_ticks, T(g))
    r = fixed_train._fixed_grid_reverse(out, W, b, csr, flags, method, arr, n_ticks, T(g_dec), decoder=(T(Wd), True, True))
    for name, x, z in zip(('g_y0', 'g_W', 'g_b'), a[:3], r[:3]):
        if x is None:
            assert z is None
            continue
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0, name
        assert torch.equal(x, z), (name, float((x - z).abs().max()))
    traj = out.cpu().numpy()
    s = decoder_sums(g_dec.reshape(-1, C), traj.reshape(-1, H))
    gWd, gbd = r[3].cpu().numpy().astype(np.float64), r[4].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(gWd - s[0]) <= 2.0 ** -23 * np.abs(s[0]) + 1e-12 * s[2])
    assert np.all(np.abs(gbd - s[1]) <= 2.0 ** -23 * np.abs(s[1]) + 1e-12 * s[3])
    # the decoder's gradients not asked for: the same three, and nothing else written
    q = fixed_train._fixed_grid_reverse(out, W, b, csr, flags, method, arr, n_ticks, T(g_dec), decoder=(T(Wd), False, False))
    assert q[3] is None and q[4] is None and torch.equal(q[0], r[0])


# --------------------------------------------------------------------------------------------------- 3. through odeint

def _double_operator(L):
    return orc.coo_from_csr(L.indptr, L.indices, L.data, L.shape).to(torch.float64)


def _oracle(L, params, x0, t, method, G, grid_pick=None, masks=None):
    """float64 autograd through the oracle's fixed-grid solve and the decoder: (decoded, [gradients in the order of `params`] + g_x0).
    grid_pick = (fine grid, index of the fine state each tick reports): the step_size option; masks: the dropout factors per evaluation"""
    A = _double_operator(L)
    p = [None if v is None else v.detach().cpu().double().requires_grad_(True) for v in params]
    W, b, Wd, bd = p
    x = x0.detach().cpu().double().requires_grad_(True)
    count = [0]

    def f(tt, y):
        k = orc.odefunc_rhs(A, y, W, b)
        if masks is not None:
            k = k * masks[count[0]]
            count[0] += 1
        return k
    if grid_pick is None:
        h = orc.odeint(f, x, t.cpu().double(), method=method)
    else:
        fine = orc.odeint(f, x, grid_pick[0].double(), method=method)
        h = torch.stack([fine[i] for i in grid_pick[1]])
    dec = F.linear(h, Wd, bd)
    (dec * G.cpu().double()).sum().backward()
    return dec.detach(), [v.grad for v in p] + [x.grad]


def _err(a, ref):
    return float((a.detach().cpu().double() - ref).abs().max())


def _readout_case(dev, S0=37, S1=29, H=64, C=1, dropout=0.0):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    L = graphs.normalized_laplacian(graphs.grid_8_neighbor_rect(S0, S1)).tocsr()
    torch.manual_seed(4)
    f = ODEFunc(H, graphs.to_device(L, dev), dropout=dropout).to(dev)
    g = torch.Generator().manual_seed(5)
    x0 = torch.rand(L.shape[0], H, generator=g)
    Wd = (torch.rand(C, H, generator=g) - 0.5) * (2.0 / H ** 0.5)
    bd = torch.rand(C, generator=g) - 0.5
    return f, L, x0, Wd, bd


def _run_pair(dev, f, x0, Wd, bd, t, G, method, options=None, seed=None):
    """[(decoded, [g_W, g_b, g_Wd, g_bd, g_x0], node name)] for the readout form and the two-step form"""
    from ndcn_amd import autograd_ops
    from ndcn_amd import torchdiffeq as ode
    kw = dict(method=method, **({} if options is None else {'options': options}))
    res = []
    for fused in (True, False):
        f.zero_grad()
        if seed is not None:
            torch.manual_seed(seed)
        y0 = x0.to(dev).requires_grad_(True)
        W, b = Wd.to(dev).requires_grad_(True), bd.to(dev).requires_grad_(True)
        out = ode.odeint(f, y0, t.to(dev), readout=(W, b), **kw) if fused else autograd_ops.linear(ode.odeint(f, y0, t.to(dev), **kw), W, b)
        node = type(out.grad_fn).__name__
        (out * G.to(dev)).sum().backward()
        res.append((out.detach(), [f.wt.weight.grad.clone(), f.wt.bias.grad.clone(), W.grad.clone(), b.grad.clone(), y0.grad.clone()], node))
    return res


def _check_pair(res, ref_dec, ref_grads, want_node):
    (dec_r, gr_r, node_r), (dec_t, gr_t, node_t) = res
    assert node_r == want_node and node_t == '_LinearBackward', (node_r, node_t)
    assert torch.equal(dec_r, dec_t)
    assert _err(dec_r, ref_dec) < 1e-4
    for name, a, b, ref in zip(('g_W', 'g_b', 'g_Wd', 'g_bd', 'g_y0'), gr_r, gr_t, ref_grads):
        ea, eb = _err(a, ref), _err(b, ref)
        print('%s: readout form error %.3e, two-step form error %.3e (scale %.3e)' % (name, ea, eb, float(ref.abs().max())))
        assert ea <= 2.0 * eb, (name, ea, eb)


@pytest.mark.parametrize('route,method', [('native', 'euler'), ('native', 'rk4'), ('python', 'euler'), ('python', 'midpoint'),
                                          ('step_size', 'euler'), ('step_size', 'rk4'), ('dropout', 'euler')])
def test_odeint_readout_under_a_gradient(dev, route, method):
    """odeint(..., readout=(Wd, bd)) with requires_grad against autograd_ops.linear(odeint(...), Wd, bd): the same decoded bits; every
    gradient at most twice as far from float64 autograd through the oracle's solve as the two-step form's; two runs the same bits.
    Routes: the library's loops, the Python loops (NDCN_FIXED_GRID_NATIVE=0), step_size with ticks strictly inside steps
    (_SubstepSolve), active dropout with a fixed seed (the Python loops carry the masks)."""
    from ndcn_amd import dropout as _dropout
    from ndcn_amd.torchdiffeq._impl import core
    f, L, x0, Wd, bd = _readout_case(dev, dropout=0.5 if route == 'dropout' else 0.0)
    f.train()
    t = torch.tensor([0., .25, .375, .625, 1.125, 1.25])
    G = torch.randn(len(t), x0.shape[0], Wd.shape[0], generator=torch.Generator().manual_seed(8))
    options, grid_pick, masks, seed = None, None, None, None
    want = '_NativeFixedGridBackward'
    env = {}
    if route == 'python':
        env, want = {'NDCN_FIXED_GRID_NATIVE': '0'}, '_FixedGridSolveBackward'
    elif route == 'step_size':
        t = torch.tensor([0., .13, .5, .55, .6, 1.0])                 # .13, .55: strictly inside steps of 0.1; .5, .6: step ends
        options, want = {'step_size': 0.1}, '_SubstepSolveBackward'
        plan = core.fixed_plan(t.numpy(), 0.1)
        assert not all(plan.tick_coincident[1:])
        grid_pick = (torch.from_numpy(np.asarray(plan.grid, np.float32)), [0] + [int(s) + 1 for s in plan.tick_step[1:]])
    elif route == 'dropout':
        seed, want = 21, '_FixedGridSolveBackward'
        torch.manual_seed(seed)
        s = _dropout.draw_seed()
        masks = [torch.from_numpy(_philox.mask(0.5, s, e, x0.shape[0], x0.shape[1]).astype(np.float64)) for e in range(len(t) - 1)]
    os.environ.update(env)
    try:
        res = _run_pair(dev, f, x0, Wd, bd, t, G, method, options, seed)
        again = _run_pair(dev, f, x0, Wd, bd, t, G, method, options, seed)[0]
    finally:
        for k in env:
            del os.environ[k]
    ref_dec, ref_grads = _oracle(L, (f.wt.weight, f.wt.bias, Wd, bd), x0, t, method, G, grid_pick, masks)
    _check_pair(res, ref_dec, ref_grads, want)
    assert torch.equal(res[0][0], again[0]) and all(torch.equal(a, b) for a, b in zip(res[0][1], again[1]))


# --------------------------------------------------------------------------------------------------- 4. routing

def test_a_state_of_the_one_launch_solve_still_trains(dev):
    """400 x 20 on the README grid: the one-launch pair keeps the solve and the decoder stays a step of its own - the same forward
    bits and gradients as the two-step form, which it is"""
    f, L, x0, Wd, bd = _readout_case(dev, 20, 20, H=20)
    t = torch.linspace(0., 1.25, 6)
    G = torch.randn(6, 400, 1, generator=torch.Generator().manual_seed(8))
    (dec_r, gr_r, node_r), (dec_t, gr_t, node_t) = _run_pair(dev, f, x0, Wd, bd, t, G, 'euler')
    assert node_r == node_t == '_LinearBackward'
    assert torch.equal(dec_r, dec_t) and all(torch.equal(a, b) for a, b in zip(gr_r, gr_t))
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in gr_r)
    # a decoder the kernel does not take (C = 16) keeps the two-step form on the large state too
    f2, _, x2, _, _ = _readout_case(dev)
    W16 = (torch.rand(16, 64, generator=torch.Generator().manual_seed(2)) - 0.5) * 0.25
    G2 = torch.randn(6, x2.shape[0], 16, generator=torch.Generator().manual_seed(9))
    (d_r, g_r, n_r), (d_t, g_t, n_t) = _run_pair(dev, f2, x2, W16, torch.zeros(16), t, G2, 'euler')
    assert n_r == n_t == '_LinearBackward' and torch.equal(d_r, d_t) and all(torch.equal(a, b) for a, b in zip(g_r, g_t))


# --------------------------------------------------------------------------------------------------- 5. NDCN

def test_ndcn_adam_step_has_no_decoder_node(dev):
    """One Adam step of NDCN(1, 64, A, 1, method='euler') on the 20 x 20 grid over 10 ticks: the output comes straight from the
    solve's node (no autograd_ops Linear for the decoder in front of it); loss and parameter gradients against float64 autograd
    through the oracle, each gradient at most twice as far from it as the two-step form's."""
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import NDCN
    L = graphs.normalized_laplacian(graphs.grid_8_neighbor(20)).tocsr()
    torch.manual_seed(0)
    model = NDCN(input_size=1, hidden_size=64, A=graphs.to_device(L, dev), num_classes=1, method='euler').to(dev)
    x0 = torch.from_numpy(graphs.x0_blocks(20)[:400])
    t = torch.linspace(0., 2.5, 11)
    target = torch.rand(400, 11, generator=torch.Generator().manual_seed(1))
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def step(two_step):
        opt.zero_grad()
        if two_step:
            out = model.output_layer(model.neural_dynamic_layer(t.to(dev), model.input_layer(x0.to(dev))))
        else:
            out = model(t.to(dev), x0.to(dev))
        loss = F.l1_loss(out.squeeze().t(), target.to(dev))
        loss.backward()
        return out, loss, {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    out_t, loss_t, gr_t = step(True)
    out, loss, gr = step(False)
    names = []
    fn = out.grad_fn
    while fn is not None and len(names) < 4:
        names.append(type(fn).__name__)
        fn = fn.next_functions[0][0] if fn.next_functions else None
    assert names[0] == '_NativeFixedGridBackward' and '_LinearBackward' not in names[:1], names
    assert out.shape[-1] == model.output_layer.weight.shape[0] != model.hidden_size, out.shape      # (what the node returns is decoded: C columns)
    assert type(out_t.grad_fn).__name__ == '_LinearBackward'
    assert torch.equal(out.detach(), out_t.detach()) and float(loss) == float(loss_t)
    sd = {k: v.cpu().double().requires_grad_(True) for k, v in before.items()}
    lo = F.l1_loss(orc.ndcn_forward(sd, _double_operator(L), t.double(), x0.double(), 'euler').squeeze().t(), target.double())
    lo.backward()
    print('loss %.8f, oracle %.8f' % (float(loss), float(lo)))
    assert abs(float(loss) - float(lo)) <= 1e-5
    for k in gr:
        ea, eb = _err(gr[k], sd[k].grad), _err(gr_t[k], sd[k].grad)
        print('%s: readout form error %.3e, two-step form error %.3e (scale %.3e)' % (k, ea, eb, float(sd[k].grad.abs().max())))
        assert ea <= 2.0 * eb, (k, ea, eb)
    opt.step()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert any(not torch.equal(p.detach(), before[k]) for k, p in model.named_parameters())


# --------------------------------------------------------------------------------------------------- 6. memory

def test_peak_memory_of_a_training_step(dev):
    """370 x 370 lattice (136 900 nodes) x 64: 35 MB panels, 24 Euler ticks, C = 1.  Over forward + backward the readout form peaks at
    or below the saved trajectory ((T + 1) panels) + what the reverse sweep asked its allocator for + 3 panels, and strictly below
    the two-step form, which holds the trajectory and its gradient (>= 2 (T + 1) panels)."""
    from ndcn_amd import autograd_ops
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.torchdiffeq._impl import tape
    f, L, x0, Wd, bd = _readout_case(dev, 370, 370)
    n_t = 25
    t = torch.linspace(0., 3., n_t).to(dev)
    panel = x0.numel() * 4
    G = torch.randn(n_t, x0.shape[0], 1, generator=torch.Generator().manual_seed(8)).to(dev)
    y0 = x0.to(dev).requires_grad_(True)
    W, b = Wd.to(dev).requires_grad_(True), bd.to(dev).requires_grad_(True)
    asked = []
    plain = tape.Tape._alloc

    def counting(self, ctx, nbytes):
        asked.append((id(self), int(nbytes)))
        return plain(self, ctx, nbytes)
    peaks = {}
    tape.Tape._alloc = counting
    try:
        for form in ('two-step', 'readout'):
            f.zero_grad()
            y0.grad = W.grad = b.grad = None
            del asked[:]
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            if form == 'readout':
                out = ode.odeint(f, y0, t, method='euler', readout=(W, b))
            else:
                out = autograd_ops.linear(ode.odeint(f, y0, t, method='euler'), W, b)
            (out * G).sum().backward()
            torch.cuda.synchronize()
            peaks[form] = torch.cuda.max_memory_allocated(dev) - base
            sweep = sum(nb for who, nb in asked if who == asked[-1][0])       # the reverse sweep's object is the last one that asked
            del out
    finally:
        tape.Tape._alloc = plain
    bound = n_t * panel + sweep + 3 * panel
    print('peak memory over one step, %d ticks of %.1f MB panels: readout form %.1f MB (bound %.1f MB: sweep scratch %.1f MB), two-step form %.1f MB'
          % (n_t, panel / 2 ** 20, peaks['readout'] / 2 ** 20, bound / 2 ** 20, sweep / 2 ** 20, peaks['two-step'] / 2 ** 20))
    assert peaks['two-step'] >= 2 * n_t * panel
    assert peaks['readout'] <= bound and peaks['readout'] < peaks['two-step']
