"""Training through fixed_adams on one autograd node (NDCN_ADAMS_TRAIN=1), on a real MI355X: the paired gather kernel
ndcn_abm_adjoint_f32 bit for bit against the numpy float32 chain, the forward pass with a record (ndcn_fixed_adams_train_f32) against the
un-differentiated solve and against its own definition, the `cap` protocol, the gradients of the node
(fixed_train._FixedAdamsSolve) against torch autograd through a float64 restatement of the solve with the node's own iteration counts
and against the per-operation graph, and which solves take the node."""
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
SIZES = (1, 3, 7, 1027)                     # below a 16-byte lane, head + tail only, one lane + tail, several workgroups
TOL = 2e-4                                  # tests/test_gpu_autograd.py: backpropagation through a fixed grid, of each tensor's maximum
WARNING = 'Warning: Functional iteration did not converge. Solution may be incorrect.'
NODE = '_FixedAdamsSolveBackward'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.asarray(a))


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def at_offset(a, off, dev):
    """a copy of the 1-d array on the device that starts `off` elements behind a 16-byte boundary"""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.size]
    v.copy_(T(a))
    return v


# ---------------------------------------------------------------------------------------------------------------- the gather kernel

def chain(ps, cps, ds, cds, base=None):
    """[base +] ((((0 + cp_0 P_0) + cd_0 D_0) + cp_1 P_1) + cd_1 D_1 ...) in numpy float32: every product and sum rounded on its own, the
    base added last"""
    with np.errstate(all='ignore'):
        s = f32(0)
        for p, cp, d, cd in zip(ps, cps, ds, cds):
            s = (s + (f32(cp) * p).astype(f32)).astype(f32)
            s = (s + (f32(cd) * d).astype(f32)).astype(f32)
        return s if base is None else (base + s).astype(f32)


@pytest.mark.parametrize('offsets', ['aligned', 'all_plus_one', 'mixed', 'out_is_base', 'same_pointer'])
@pytest.mark.parametrize('n', range(1, 12))
def test_abm_adjoint_bit_for_bit(dev, n, offsets):
    """every pair count at sizes around the 16-byte lane, with and without a base, panels on / one element off / differently off a
    16-byte boundary, the base updated in place, and P_q and D_q the same panel; the inputs are left as they were"""
    from ndcn_amd import hip
    rng = np.random.RandomState(500 + n)
    for size in SIZES:
        for with_base in ((True,) if offsets == 'out_is_base' else (False, True)):
            ps = [rng.randn(size).astype(f32) for _ in range(n)]
            ds = ps if offsets == 'same_pointer' else [rng.randn(size).astype(f32) for _ in range(n)]
            cps, cds = (rng.randn(n) * 0.05).astype(f32), (rng.randn(n) * 0.05).astype(f32)
            base = rng.randn(size).astype(f32) if with_base else None
            want = chain(ps, cps, ds, cds, base)
            one = offsets == 'all_plus_one'
            oo = 1 if one else 0
            pd = [at_offset(p, 1 if one else (q % 4 if offsets == 'mixed' else 0), dev) for q, p in enumerate(ps)]
            dd = pd if offsets == 'same_pointer' else [at_offset(d, 1 if one else ((q + 2) % 4 if offsets == 'mixed' else 0), dev)
                                                       for q, d in enumerate(ds)]
            bd = at_offset(base, 2 if offsets == 'mixed' else oo, dev) if with_base else None
            if offsets == 'out_is_base':
                got = hip.abm_adjoint(pd, cps, dd, cds, base=bd, out=bd)
                assert got.data_ptr() == bd.data_ptr()
            else:
                out = at_offset(np.full(size, 7.0, dtype=f32), oo, dev)
                got = hip.abm_adjoint(pd, cps, dd, cds, base=bd, out=out)
                if with_base:
                    assert np.array_equal(bits(bd.cpu().numpy()), bits(base))     # the base is only read
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (n, size, offsets, with_base)
            for g, d in zip(ps + ds, pd + dd):
                assert np.array_equal(bits(d.cpu().numpy()), bits(g))             # ... and so are the terms


def test_abm_adjoint_starts_from_an_exact_zero(dev):
    from ndcn_amd import hip
    cps, cds = np.asarray([0.5, -0.25], dtype=f32), np.asarray([2.0, -1.0], dtype=f32)
    # every product is -0.0: the sum starts from +0, so it is +0.0 - and a -0.0 base plus +0.0 is +0.0
    ps = [np.full(8, -0.0 if c > 0 else 0.0, dtype=f32) for c in cps]
    ds = [np.full(8, -0.0 if c > 0 else 0.0, dtype=f32) for c in cds]
    for bb in (None, np.full(8, -0.0, dtype=f32)):
        want = chain(ps, cps, ds, cds, bb)
        assert not np.signbit(want).any()
        got = hip.abm_adjoint([T(p).to(dev) for p in ps], cps, [T(d).to(dev) for d in ds], cds, base=None if bb is None else T(bb).to(dev))
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))


def test_abm_adjoint_refuses_bad_arguments_before_any_launch(dev):
    from ndcn_amd import _lib
    lib = _lib.load()
    size = 260
    gs = [torch.randn(size, device=dev) for _ in range(24)]
    base = torch.randn(size, device=dev)
    out = torch.full((size,), 7.0, device=dev)
    coef = (ctypes.c_float * 12)(*([0.5] * 12))

    def call(n, pp, dp, o=out, bb=None, n_elem=size):
        ap = (ctypes.c_void_p * max(len(pp), 1))(*pp)
        ad = (ctypes.c_void_p * max(len(dp), 1))(*dp)
        with torch.cuda.device(dev):
            return lib.ndcn_abm_adjoint_f32(_lib.ptr(o), _lib.ptr(bb), ap, coef, ad, coef, n, n_elem, _lib.stream_ptr())
    P, D = [g.data_ptr() for g in gs[:12]], [g.data_ptr() for g in gs[12:]]
    for n in (0, 12, -1):
        assert call(n, P[:max(n, 1)], D[:max(n, 1)]) == _lib.EINVAL
    assert call(3, [P[0], None, P[2]], D[:3]) == _lib.EINVAL                      # a null panel, either side
    assert call(3, P[:3], [D[0], D[1], None]) == _lib.EINVAL
    assert call(3, [P[0], out.data_ptr(), P[2]], D[:3]) == _lib.EINVAL           # out aliases a term, either side
    assert b'aliases' in lib.ndcn_last_error()
    assert call(3, P[:3], [out.data_ptr(), D[1], D[2]]) == _lib.EINVAL
    assert call(2, P[:2], D[:2], n_elem=0) == 0                                   # nothing to do: no launch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                               # nothing was written
    keep = base.clone()
    assert call(1, P[:1], D[:1]) == 0 and call(2, P[:2], D[:2], o=base, bb=base) == 0     # one pair; out == base is allowed
    torch.cuda.synchronize()
    assert torch.equal(out, (0.0 + 0.5 * gs[0]) + 0.5 * gs[12])
    assert torch.equal(base, keep + ((((0.0 + 0.5 * gs[0]) + 0.5 * gs[12]) + 0.5 * gs[1]) + 0.5 * gs[13]))


# ----------------------------------------------------------------------------------------------------------- the forward with a record

def lattice_func(side, H, dev, seed=0):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(seed)
    f = ODEFunc(H, graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(side)), dev)).to(dev).eval()
    return f, torch.rand(side * side, H).to(dev)


def golden_func(d, dev):
    from ndcn_amd import CsrOperator
    from ndcn_amd.neural_dynamics import ODEFunc
    A = CsrOperator.from_arrays(d['indptr'], d['indices'], d['data'], d['shape'], dev)
    f = ODEFunc(d['W'].shape[0], A).to(dev)
    f.load_state_dict({'wt.weight': T(d['W']), 'wt.bias': T(d['b'])})
    return f.eval()


def record_case(name, dev):
    """(func, x0, t, step_size, max_order, rtol, atol, max_iters)"""
    if name.startswith('moulton_'):
        d = load_golden(name)
        return (golden_func(d, dev), T(d['x0']).to(dev), T(d['t']), float(d['opt_step_size']) if 'opt_step_size' in d else None,
                int(d['opt_max_order']) if 'opt_max_order' in d else 12, float(d['rtol']), float(d['atol']),
                int(d['opt_max_iters']) if 'opt_max_iters' in d else 4)
    f, x0 = lattice_func(40, 20, dev)
    if name == 'lattice40_step_size':
        return f, x0, torch.tensor([0., 4.5 / 128, 5.0 / 128, 14.0 / 128]), 1.0 / 128, 6, 1e-2, 1e-3, 2
    return f, x0, torch.arange(15) / 128.0, None, 12, 1e-4, 1e-5, 4


def run_record(dev, f, x0, t, step_size, max_order, rtol, atol, max_iters, cap=None, guard=0):
    """both entry points on the same arguments -> a dict of what they wrote"""
    from ndcn_amd import _lib
    from ndcn_amd.csr import as_csr
    from ndcn_amd.torchdiffeq._impl import core, fixed_train
    lib = _lib.load()
    H = x0.shape[1]
    plan = core.fixed_plan(t.numpy(), step_size)
    dts, n_steps, steps, same, offs, n_emit = fixed_train.plan_arrays(plan)
    csr = as_csr(f.A)
    csr.ensure_plans(H)
    W, b = f.wt.weight.detach().contiguous(), f.wt.bias.detach().contiguous()
    shape = tuple(x0.shape)

    def fresh():
        o = torch.full((n_emit + 1,) + shape, 7.0, device=dev)
        o[0].copy_(x0)
        return o, (ctypes.c_int * n_steps)(), (ctypes.c_int * n_steps)()
    want, w_it, w_cv = fresh()
    nb = int(lib.ndcn_fixed_adams_workspace_bytes(shape[0], H, max_order))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.ndcn_solve_fixed_adams_f32(csr.view_ref(), _lib.ptr(W), _lib.ptr(b), H, _lib.F_RELU, _lib.ptr(want[0]), dts, n_steps, steps,
                                                  same, offs, n_emit, max_order, rtol, atol, max_iters, _lib.ptr(want[1:]), w_it, w_cv,
                                                  _lib.ptr(ws), nb, _lib.stream_ptr()))
    out, it, cv = fresh()
    if cap is None:
        cap = n_steps * max_iters
    rec_f = torch.full((n_steps,) + shape, 7.0, device=dev)
    rec_y = out[1:] if plan.default else torch.full((n_steps,) + shape, 7.0, device=dev)
    rec_u = torch.full((cap + guard,) + shape, 7.0, device=dev)
    rec_c = torch.full((cap + guard,) + shape, 7.0, device=dev)
    slots = (ctypes.c_int64 * n_steps)()
    nbt = int(lib.ndcn_fixed_adams_train_workspace_bytes(shape[0], H))
    wst = torch.empty(nbt, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.ndcn_fixed_adams_train_f32(csr.view_ref(), _lib.ptr(W), _lib.ptr(b), H, _lib.F_RELU, _lib.ptr(out[0]), dts, n_steps, steps, same,
                                            offs, n_emit, max_order, rtol, atol, max_iters, _lib.ptr(out[1:]), it, cv, _lib.ptr(rec_f),
                                            _lib.ptr(rec_y), _lib.ptr(rec_u), _lib.ptr(rec_c), cap, slots, _lib.ptr(wst), nbt, _lib.stream_ptr())
    torch.cuda.synchronize()
    return dict(rc=rc, plan=plan, csr=csr, W=W, b=b, want=want, w_it=list(w_it), w_cv=list(w_cv), out=out, it=list(it), cv=list(cv),
                rec_f=rec_f, rec_y=rec_y, rec_u=rec_u, rec_c=rec_c, slots=list(slots), n_steps=n_steps, cap=cap)


RECORD_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'moulton_*.npz'))) + \
    ['lattice40', 'lattice40_rhs_mid', 'lattice40_step_size']


@pytest.mark.parametrize('name', RECORD_CASES)
def test_forward_record(dev, name):
    """out, the iteration counts and the flags are those of the un-differentiated solve bit for bit; rec_f[i] is the right-hand side at the
    state step i starts from, every corrector evaluation the right-hand side at its stored iterate, and the first iterate of a step the
    predictor's"""
    from ndcn_amd import _lib, hip
    from ndcn_amd.torchdiffeq._impl import core
    lib = _lib.load()
    f, x0, t, step_size, max_order, rtol, atol, max_iters = record_case(name, dev)
    prev = lib.ndcn_set_rhs_mid(1) if name == 'lattice40_rhs_mid' else None
    try:
        r = run_record(dev, f, x0, t, step_size, max_order, rtol, atol, max_iters)
        assert r['rc'] == 0, lib.ndcn_last_error()
        assert torch.equal(r['out'], r['want']) and r['it'] == r['w_it'] and r['cv'] == r['w_cv']
        assert bool(torch.isfinite(r['out']).all())
        plan, csr, W, b = r['plan'], r['csr'], r['W'], r['b']
        lengths = core.abm_history_lengths(r['n_steps'], max_order, r['cv'])
        used = 0
        for i in range(r['n_steps']):
            y = x0 if i == 0 else r['rec_y'][i - 1]
            assert torch.equal(r['rec_f'][i], hip.rhs(csr, y, W, b)), i
            assert r['slots'][i] == used
            if lengths[i] < 3:
                assert r['it'][i] == 0 and r['cv'][i] == 1
                continue
            assert 1 <= r['it'][i] <= max_iters
            n = lengths[i]
            _, _, u0 = hip.abm_predict(y, [r['rec_f'][i - q] for q in range(n)], core.ab_weights(n), core.am_weights(n)[1], plan.dts[i])
            assert torch.equal(r['rec_u'][used], u0), i
            for s in range(used, used + r['it'][i]):
                assert torch.equal(r['rec_c'][s], hip.rhs(csr, r['rec_u'][s], W, b)), (i, s)
            used += r['it'][i]
        assert bool((r['rec_u'][used:] == 7.0).all()) and bool((r['rec_c'][used:] == 7.0).all())       # no slot past the last one
        for j in range(1, len(t)):                                       # every tick is the state after the step that reports it
            y = r['rec_y'][plan.tick_step[j]]
            assert torch.equal(r['out'][j], y if plan.tick_coincident[j] else y + 0.0)
        if name in ('moulton_iterate', 'lattice40', 'moulton_never'):
            assert max(r['it']) >= 2
        if name == 'lattice40_step_size':
            assert not plan.tick_coincident[1] and plan.tick_coincident[2]
    finally:
        if prev is not None:
            lib.ndcn_set_rhs_mid(prev)


def test_a_record_one_slot_short_is_refused_and_nothing_past_it_is_written(dev):
    from ndcn_amd import _lib
    lib = _lib.load()
    case = record_case('moulton_iterate', dev)
    full = run_record(dev, *case)
    total = sum(full['it'])
    assert full['rc'] == 0 and total > full['n_steps'] - 2                   # some step iterates twice
    short = run_record(dev, *case, cap=total - 1, guard=1)
    assert short['rc'] == _lib.ECAPACITY == -7
    assert b'cap' in lib.ndcn_last_error()
    assert bool((short['rec_u'][total - 1:] == 7.0).all()) and bool((short['rec_c'][total - 1:] == 7.0).all())     # the guard panel
    assert torch.equal(short['rec_u'][:total - 1], full['rec_u'][:total - 1])                   # what fitted is what the full run wrote
    exact = run_record(dev, *case, cap=total, guard=1)
    assert exact['rc'] == 0 and torch.equal(exact['out'], full['want'])
    assert bool((exact['rec_u'][total:] == 7.0).all()) and bool((exact['rec_c'][total:] == 7.0).all())
    none = run_record(dev, *case, cap=0, guard=1)
    assert none['rc'] == _lib.ECAPACITY and bool((none['rec_u'] == 7.0).all())


# --------------------------------------------------------------------------------------------------------------------------- gradients

def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def fp64_solve(A, W, b, y0, dts, log, max_order=12):
    """fixed_adams in float64 torch on the CPU with the exact rational weights and the iteration counts and converged flags FIXED to
    `log` (what the device solve ran): the function whose autograd is the truth.  -> the states after every grid step, y0 first"""
    f = lambda x: torch.relu((A @ x) @ W.t() + b)
    hist, y, sol = [], y0, [y0]
    for i, dt in enumerate(dts):
        hist.insert(0, f(y))
        del hist[max_order - 1:]
        k = len(hist)
        if k < 3:
            assert log[i] == (0, True)
            k1 = hist[0]
            k2 = f(y + dt * k1 / 3)
            k3 = f(y + dt * (k1 / -3 + k2))
            k4 = f(y + dt * (k1 - k2 + k3))
            y = y + (k1 + 3 * k2 + 3 * k3 + k4) * (dt / 8)
        else:
            mu = [float(x) for x in am.mus(k)]
            dy = dt * sum(float(bi) * fi for bi, fi in zip(ab.betas(k), hist))
            delta = dt * sum(mi * fi for mi, fi in zip(mu[1:], hist))
            assert log[i][0] >= 1
            for _ in range(log[i][0]):
                dy = dt * mu[0] * f(y + dy) + delta
            y = y + dy
            if not log[i][1]:
                hist.pop()                                        # the oldest evaluation leaves
        sol.append(y)
    return torch.stack(sol)


_DENSE = {}


def dense_operator(side):
    from ndcn_amd import graphs
    if side not in _DENSE:
        _DENSE[side] = torch.from_numpy(np.asarray(graphs.normalized_laplacian(graphs.grid_8_neighbor(side)).todense())).double()
    return _DENSE[side]


def device_run(dev, monkeypatch, switch, side, H, t, rtol, atol, opts, C, seed, capfd):
    """one loss.backward() through odeint(method='fixed_adams') -> (name of the node, solution, gradients, step log, warning lines, the
    leaves' values)"""
    from ndcn_amd import torchdiffeq as ode
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '1' if switch else '0')
    f, x0 = lattice_func(side, H, dev, seed=seed)
    x = x0.clone().requires_grad_(True)
    gen = torch.Generator().manual_seed(9)
    Wd = bd = None
    if C is not None:
        Wd = (torch.randn(C, H, generator=gen) / 4).to(dev).requires_grad_(True)
        bd = torch.randn(C, generator=gen).to(dev).requires_grad_(True)
    target = torch.rand(len(t), side * side, C if C is not None else H, generator=gen)
    log = []
    capfd.readouterr()
    y = ode.odeint(f, x, t.to(dev), rtol=rtol, atol=atol, method='fixed_adams', options=dict(opts) or None, step_log=log,
                   readout=None if C is None else (Wd, bd))
    name = type(y.grad_fn).__name__
    torch.nn.functional.l1_loss(y, target.to(dev)).backward()
    torch.cuda.synchronize()
    warn = [l for l in capfd.readouterr().err.splitlines() if l == WARNING]
    grads = [x.grad, f.wt.weight.grad, f.wt.bias.grad] + ([Wd.grad, bd.grad] if C is not None else [])
    leaves = [x0, f.wt.weight.detach(), f.wt.bias.detach()] + ([Wd.detach(), bd.detach()] if C is not None else [])
    return name, y.detach(), [g.detach().cpu().double() for g in grads], log, warn, [v.cpu().double() for v in leaves], target


def check_gradients(dev, monkeypatch, capfd, side, H, t, rtol=1e-7, atol=1e-9, opts=None, C=None, seed=3):
    """the node against float64 autograd with the node's own iteration counts, and against the per-operation graph; -> the step log"""
    from ndcn_amd.torchdiffeq._impl import core
    opts = opts or {}
    name, y, got, log, warn, leaves, target = device_run(dev, monkeypatch, True, side, H, t, rtol, atol, opts, C, seed, capfd)
    assert name == NODE
    plan = core.fixed_plan(t.numpy(), opts.get('step_size'))
    assert log[-1][0] == 'nfe' and len(log) == len(plan.dts) + 1
    steps = log[:-1]
    assert len(warn) == sum(1 for _, c in steps if not c)
    assert log[-1][1] == len(steps) + 3 * sum(1 for i, _ in steps if i == 0) + sum(i for i, _ in steps)
    vs = [v.clone().requires_grad_(True) for v in leaves]
    states = fp64_solve(dense_operator(side), vs[1], vs[2], vs[0], [float(d) for d in plan.dts], steps, opts.get('max_order', 12))
    yo = states[[0] + [int(s) + 1 for s in plan.tick_step[1:]]]               # a tick is the state after the step that reports it
    if C is not None:
        yo = yo @ vs[3].t() + vs[4]
    assert float((y.cpu().double() - yo.detach()).abs().max()) < 1e-5
    torch.nn.functional.l1_loss(yo, target.double()).backward()
    worst = [rel(g, v.grad) for g, v in zip(got, vs)]
    with capfd.disabled():
        print('fixed_adams training, %d x %d, H = %d, %s, rtol %g, C %s, iterations %s: gradient errors of (y0, W, b%s) / max = %s'
              % (side, side, H, opts, rtol, C, [i for i, _ in steps], ', Wd, bd' if C is not None else '', ' '.join('%.2e' % w for w in worst)))
    assert all(w < TOL for w in worst), worst
    # the per-operation graph: the same decisions, the same bits forward, gradients within the same bound
    name2, y2, got2, log2, warn2, _, _ = device_run(dev, monkeypatch, False, side, H, t, rtol, atol, opts, C, seed, capfd)
    assert name2 != NODE and log2 == log and len(warn2) == len(warn)
    if C is None:
        assert torch.equal(y2, y)
    worst2 = [rel(g, g2) for g, g2 in zip(got, got2)]
    with capfd.disabled():
        print('    against the per-operation graph: %s' % ' '.join('%.2e' % w for w in worst2))
    assert all(w < TOL for w in worst2), worst2
    return steps


T13 = torch.arange(13) / 128.0
T13_WIDE = torch.arange(13) * (2.0 / 128)
T16 = torch.arange(16) / 128.0
LATTICES = {'6x6_H8': (6, 8), '40x40_H20': (40, 20)}


@pytest.mark.parametrize('lattice', sorted(LATTICES))
def test_gradients_default_tolerances(dev, monkeypatch, capfd, lattice):
    side, H = LATTICES[lattice]
    steps = check_gradients(dev, monkeypatch, capfd, side, H, T13 if side == 6 else T16)
    assert steps[:2] == [(0, True)] * 2 and all(1 <= i <= 4 for i, _ in steps[2:])


@pytest.mark.parametrize('lattice', sorted(LATTICES))
def test_gradients_of_a_solve_that_iterates_twice(dev, monkeypatch, capfd, lattice):
    side, H = LATTICES[lattice]
    steps = check_gradients(dev, monkeypatch, capfd, side, H, T13_WIDE, rtol=1e-4, atol=1e-5)
    assert all(c for _, c in steps) and max(i for i, _ in steps) >= 2


@pytest.mark.parametrize('lattice', sorted(LATTICES))
def test_gradients_when_every_step_fails(dev, monkeypatch, capfd, lattice):
    """rtol = atol = 0: no element ever passes the strict test - two iterations per step, a warning line per step, a history of three"""
    side, H = LATTICES[lattice]
    steps = check_gradients(dev, monkeypatch, capfd, side, H, T13, rtol=0.0, atol=0.0, opts={'max_iters': 2})
    assert steps == [(0, True)] * 2 + [(2, False)] * 10


@pytest.mark.parametrize('lattice', sorted(LATTICES))
def test_gradients_max_order_4(dev, monkeypatch, capfd, lattice):
    side, H = LATTICES[lattice]
    check_gradients(dev, monkeypatch, capfd, side, H, T13, rtol=1e-2, atol=1e-3, opts={'max_order': 4})


@pytest.mark.parametrize('lattice', sorted(LATTICES))
def test_gradients_on_a_step_size_plan_with_loose_and_coincident_ticks(dev, monkeypatch, capfd, lattice):
    from ndcn_amd.torchdiffeq._impl import core
    side, H = LATTICES[lattice]
    t = torch.tensor([0., 4.5 / 128, 5.0 / 128, 14.0 / 128])
    plan = core.fixed_plan(t.numpy(), 1.0 / 128)
    assert not plan.tick_coincident[1] and plan.tick_coincident[2] and plan.tick_coincident[3] and len(plan.dts) == 14
    check_gradients(dev, monkeypatch, capfd, side, H, t, rtol=1e-4, atol=1e-5, opts={'step_size': 1.0 / 128, 'max_order': 6})


@pytest.mark.parametrize('lattice', sorted(LATTICES))
def test_gradients_warm_up_only(dev, monkeypatch, capfd, lattice):
    side, H = LATTICES[lattice]
    assert check_gradients(dev, monkeypatch, capfd, side, H, T13[:3]) == [(0, True)] * 2


@pytest.mark.parametrize('grid', ['default', 'step_size'])
@pytest.mark.parametrize('C', [1, 3])
def test_gradients_with_the_decoder_inside_the_node(dev, monkeypatch, capfd, C, grid):
    t, opts = (T13_WIDE, {}) if grid == 'default' else (torch.tensor([0., 4.5 / 128, 5.0 / 128, 14.0 / 128]), {'step_size': 1.0 / 128, 'max_order': 6})
    check_gradients(dev, monkeypatch, capfd, 6, 8, t, rtol=1e-4, atol=1e-5, opts=opts, C=C)


def test_gradients_with_the_decoder_on_the_larger_lattice(dev, monkeypatch, capfd):
    check_gradients(dev, monkeypatch, capfd, 40, 20, T13_WIDE, rtol=1e-4, atol=1e-5, C=1)


# ------------------------------------------------------------------------------------------------------------------------------ routes

def test_the_node_takes_the_solve_and_its_forward_is_the_plain_solve(dev, monkeypatch):
    from ndcn_amd import torchdiffeq as ode
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '1')
    f, x0 = lattice_func(6, 8, dev, seed=3)
    t = T13_WIDE.to(dev)
    for opts in (None, {'max_order': 5}, {'step_size': 1.0 / 128, 'max_order': 6}, {'max_iters': 1}):
        with torch.no_grad():
            want = ode.odeint(f, x0, t, rtol=1e-4, atol=1e-5, method='fixed_adams', options=opts)
        y = ode.odeint(f, x0.clone().requires_grad_(True), t, rtol=1e-4, atol=1e-5, method='fixed_adams', options=opts)
        assert type(y.grad_fn).__name__ == NODE
        assert torch.equal(y.detach(), want)
    # implicit = False is explicit_adams: its node
    y = ode.odeint(f, x0.clone().requires_grad_(True), t, method='fixed_adams', options={'implicit': False})
    assert type(y.grad_fn).__name__ == '_ExplicitAdamsSolveBackward'


def test_everything_else_keeps_its_route_and_its_gradients(dev, monkeypatch):
    """the switch off, a lambda, a tuple state, no_control, an active dropout: not the node - and a gradient all the same"""
    from ndcn_amd import graphs
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.neural_dynamics import ODEFunc
    f, x0 = lattice_func(6, 8, dev, seed=3)
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(6)), dev)
    torch.manual_seed(5)
    f_nc = ODEFunc(8, A, no_control=True).to(dev).eval()
    f_drop = ODEFunc(8, A, dropout=0.5).to(dev).train()
    t = T13.to(dev)

    def run(func, tuple_state=False):
        x = x0.clone().requires_grad_(True)
        if tuple_state:
            y = ode.odeint(lambda tt, ys: (func(tt, ys[0]),), (x,), t, rtol=1e-2, atol=1e-3, method='fixed_adams')[0]
        else:
            y = ode.odeint(func, x, t, rtol=1e-2, atol=1e-3, method='fixed_adams')
        y.sum().backward()
        assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
        return type(y.grad_fn).__name__
    monkeypatch.delenv('NDCN_ADAMS_TRAIN', raising=False)
    assert run(f) != NODE
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '0')
    assert run(f) != NODE
    monkeypatch.setenv('NDCN_ADAMS_TRAIN', '1')
    assert run(f) == NODE
    assert run(lambda tt, y: f(tt, y)) != NODE
    assert run(f, tuple_state=True) != NODE
    assert run(f_nc) != NODE
    assert run(f_drop) != NODE
    f_drop.eval()                                                    # dropout that is not active does not keep the node away
    assert run(f_drop) == NODE


def test_the_second_attempt_runs_once_and_gives_the_same_gradients(dev, monkeypatch, capfd):
    """room for one corrector evaluation only: the library reports the full record, the solve runs again with room for max_iters per step"""
    from ndcn_amd import _lib
    from ndcn_amd.torchdiffeq._impl import fixed_train
    args = (dev, monkeypatch, True, 6, 8, T13, 1e-2, 1e-3, {}, None, 3, capfd)     # (the tolerances of the fixtures that iterate once)
    calls = []
    real = fixed_train._fixed_adams_attempt

    def counted(*a):
        res = real(*a)
        calls.append((a[-1], res[0]))
        return res
    monkeypatch.setattr(fixed_train, '_fixed_adams_attempt', counted)
    name, y, grads, log, _, _, _ = device_run(*args)
    assert name == NODE and calls == [(12, 0)] and log[:-1] == [(0, True)] * 2 + [(1, True)] * 10      # one attempt where one slot per step suffices
    del calls[:]
    monkeypatch.setattr(fixed_train, '_first_cap', lambda n_steps: 1)
    name2, y2, grads2, log2, _, _, _ = device_run(*args)
    assert name2 == NODE and calls == [(1, _lib.ECAPACITY), (12 * 4, 0)]
    assert torch.equal(y2, y) and log2 == log
    assert all(torch.equal(g, g2) for g, g2 in zip(grads, grads2))


def test_ndcn_training_step(dev, monkeypatch):
    """NDCN(method='fixed_adams') in training mode, one loss.backward() on the node: every parameter's gradient against the
    per-operation graph's"""
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import NDCN
    S, H = 6, 8
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(S)), dev)
    x0 = torch.from_numpy(graphs.x0_blocks(S)[:S * S]).to(dev)
    target = torch.rand(13, S * S, 1, generator=torch.Generator().manual_seed(2)).to(dev)
    res = {}
    for switch in ('1', '0'):
        monkeypatch.setenv('NDCN_ADAMS_TRAIN', switch)
        torch.manual_seed(1)
        m = NDCN(input_size=1, hidden_size=H, A=A, num_classes=1, rtol=1e-2, atol=1e-3, method='fixed_adams').to(dev).train()
        out = m(T13.to(dev), x0)
        assert (type(out.grad_fn).__name__ == NODE) == (switch == '1')
        loss = torch.nn.functional.l1_loss(out, target)
        loss.backward()
        res[switch] = (float(loss.detach()), {k: p.grad.detach().cpu().double() for k, p in m.named_parameters()})
    assert abs(res['1'][0] - res['0'][0]) < 1e-6
    for k in res['1'][1]:
        assert rel(res['1'][1][k], res['0'][1][k]) < TOL, k
