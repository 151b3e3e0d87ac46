"""Training through dopri5 with an ACTIVE dropout on the native tape (ndcn_tape_dopri5_drop_f32, NDCN_TAPE_DROPOUT=1) against the
per-operation autograd path (NDCN_GRAD_TAPE=0) under the same torch.manual_seed: the tape numbers its evaluations as that path makes
them (f0, the initial step's f1, six per attempted step), so every launch gets the same counter-based mask - trajectory and step log
bit for bit - and the gradients agree up to the order of float32 sums (the bound test_gpu_tape.py uses at p = 0)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

SWITCHES = ('NDCN_GRAD_TAPE', 'NDCN_TAPE_DROPOUT', 'NDCN_TAPE_BUDGET_MB')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need a ROCm device'
    return torch.device('cuda:0')


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-30))


def _solve(dev, mode, make_func, x0_host, ticks, rtol, atol, w_host, seed=5, budget=None, train=True):
    """mode 'tape': NDCN_TAPE_DROPOUT=1; 'per_op': NDCN_GRAD_TAPE=0; 'default': no switch.  -> (trajectory, log, grads, node name)"""
    from ndcn_amd import torchdiffeq as ode
    env = {'tape': {'NDCN_TAPE_DROPOUT': '1'}, 'per_op': {'NDCN_GRAD_TAPE': '0'}, 'default': {}}[mode]
    if budget is not None:
        env = dict(env, NDCN_TAPE_BUDGET_MB=str(budget))
    assert not any(k in os.environ for k in SWITCHES)
    os.environ.update(env)
    try:
        f = make_func()
        f.train(train)
        x0 = x0_host.clone().to(dev).requires_grad_(True)
        log = []
        torch.manual_seed(seed)
        y = ode.odeint(f, x0, torch.tensor(ticks).to(dev), rtol=rtol, atol=atol, method='dopri5', step_log=log)
        (y * w_host.to(dev)).sum().backward()
        grads = [x0.grad.cpu()] + [p.grad.cpu() for p in f.parameters() if p.grad is not None]
        return y.detach().cpu(), log, grads, type(y.grad_fn).__name__
    finally:
        for k in env:
            del os.environ[k]


def _check(a, b, bound=2e-4):
    """the three criteria: a = the tape's result, b = the per-operation path's"""
    ya, la, ga, na = a
    yb, lb, gb, nb = b
    assert na.startswith('_TapeDopri5'), na                        # (fails without the feature: the solve stays on the per-operation graph)
    assert not nb.startswith('_TapeDopri5')
    assert la == lb and torch.equal(ya, yb)
    assert len(ga) == len(gb)
    figures = [rel(x, y) for x, y in zip(ga, gb)]
    print('attempts %d, gradient rel %s' % (len([r for r in la if r[0] != 'nfe']), ['%.2e' % v for v in figures]))
    assert all(v < bound for v in figures), figures


def _reference_model(dev, variant, p):
    from ndcn_amd import CsrOperator
    from ndcn_amd.neural_dynamics import ODEFunc
    d = load_golden('fixed_rk4_equal')
    x0 = torch.from_numpy(np.asarray(d['x0'], dtype=np.float32))

    def make():
        f = ODEFunc(20, CsrOperator.from_arrays(d['indptr'], d['indices'], d['data'], d['shape'], dev), dropout=p,
                    no_control=variant == 'no_control', no_graph=variant == 'no_graph').to(dev)
        f.load_state_dict({'wt.weight': torch.from_numpy(np.asarray(d['W'], dtype=np.float32)),
                           'wt.bias': torch.from_numpy(np.asarray(d['b'], dtype=np.float32))})
        return f
    return make, x0


@pytest.mark.parametrize('p', [0.5, 0.1])
@pytest.mark.parametrize('variant', ['default', 'no_control', 'no_graph'])
@pytest.mark.parametrize('ticks,rtol,atol', [([0., 0.3, 0.6, 0.9, 1.0], 1e-3, 1e-5), (list(np.linspace(0., 5., 80)), 1e-2, 1e-3)])
def test_tape_equals_the_per_operation_path_on_the_reference_size(dev, variant, ticks, rtol, atol, p):
    """400 nodes x 20 hidden: the mask in the narrow-panel launch's epilogue; both time grids of test_gpu_tape.py's p = 0 cases"""
    from ndcn_amd import _lib
    assert _lib.load().ndcn_abi_version() == 29
    make, x0 = _reference_model(dev, variant, p)
    w = torch.randn(len(ticks), *x0.shape, generator=torch.Generator().manual_seed(3))
    a = _solve(dev, 'tape', make, x0, ticks, rtol, atol, w)
    b = _solve(dev, 'per_op', make, x0, ticks, rtol, atol, w)
    _check(a, b)
    if len(ticks) == 80:
        print('most ticks in one accepted step: %d' % _most_ticks_in_a_step(ticks, a[1]))


def _most_ticks_in_a_step(ticks, log):
    return max(sum(1 for tk in ticks if r[0] < tk <= r[0] + r[1]) for r in log if r[0] != 'nfe' and r[2] == 1.0)


def test_more_than_seven_ticks_in_a_step(dev):
    """The dense output of one accepted step in more than one pass of <= 7 ticks.  With a mask per evaluation the steps stay short:
    on the 80-tick grid above the longest step covers 3 to 12 ticks depending on variant and p (measured, MI355X), so this case
    spreads 400 ticks over the same interval at the same tolerances and asserts the property."""
    make, x0 = _reference_model(dev, 'default', 0.5)
    ticks = list(np.linspace(0., 5., 400))
    w = torch.randn(len(ticks), *x0.shape, generator=torch.Generator().manual_seed(3))
    a = _solve(dev, 'tape', make, x0, ticks, 1e-2, 1e-3, w)
    b = _solve(dev, 'per_op', make, x0, ticks, 1e-2, 1e-3, w)
    _check(a, b)
    most = _most_ticks_in_a_step(ticks, a[1])
    print('most ticks in one accepted step: %d' % most)
    assert most > 14, most                                        # (three passes at least)


def _wide_model(dev, side, no_control, p=0.5):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    H = 256
    op = graphs.normalized_laplacian(graphs.grid_8_neighbor(side))
    x0 = torch.rand(side * side, H, generator=torch.Generator().manual_seed(2))

    def make():
        torch.manual_seed(0)
        return ODEFunc(H, graphs.to_device(op, dev), dropout=p, no_control=no_control).to(dev)
    return make, x0


WIDE_TICKS, WIDE_RTOL, WIDE_ATOL = [0., 0.4, 0.9, 1.5], 1e-2, 1e-3


@pytest.mark.parametrize('side,no_control', [(12, False), (12, True), (36, False), (36, True)])
def test_tape_equals_the_per_operation_path_at_the_fused_width(dev, side, no_control):
    """H = 256: the routes without a dropout epilogue - the launch, then ndcn_dropout_combine_f32 (mask and stage sum in one pass).
    Side 12 is inside the ATen-order range of the error norm, side 36 (331 776 elements) past it."""
    make, x0 = _wide_model(dev, side, no_control)
    w = torch.randn(len(WIDE_TICKS), side * side, 256, generator=torch.Generator().manual_seed(1))
    a = _solve(dev, 'tape', make, x0, WIDE_TICKS, WIDE_RTOL, WIDE_ATOL, w)
    b = _solve(dev, 'per_op', make, x0, WIDE_TICKS, WIDE_RTOL, WIDE_ATOL, w)
    _check(a, b)
    assert len([r for r in a[1] if r[0] != 'nfe']) >= 3


REJECT_RTOL, REJECT_ATOL = 1e-3, 1e-4


def test_tape_with_rejected_attempts(dev):
    """The 1500-node Barabasi-Albert graph x 32 of test_gpu_tape.py's rejected-attempts case at rtol 1e-3 / atol 1e-4.  Every evaluation
    has another mask, so the error estimate does not shrink with the step as it does at p = 0 and the step count grows fast with the
    tolerance.  Measured on the per-operation path (MI355X, p = 0.5; the seed moves the counts by one or two): 1e-2 / 1e-3 rejects
    nothing (22 attempts over [0, 2.5]); 1e-3 / 1e-4 rejects its first five attempts (the initial step is too long) and needs 96
    attempts over [0, 2.5], 54 over [0, 1] - so the pair is 1e-3 / 1e-4 and the time grid is that case's without its last tick.  A
    rejected attempt consumes its six evaluation numbers like an accepted one."""
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    n, H = 1500, 32
    op = graphs.normalized_laplacian(graphs.barabasi_albert(n, 4, seed=1))
    ticks = [0., 0.01, 0.02, 0.9, 1.0]
    x0 = 25.0 * torch.rand(n, H, generator=torch.Generator().manual_seed(2))
    w = torch.randn(len(ticks), n, H, generator=torch.Generator().manual_seed(1))

    def make():
        torch.manual_seed(0)
        return ODEFunc(H, graphs.to_device(op, dev), dropout=0.5).to(dev)

    a = _solve(dev, 'tape', make, x0, ticks, REJECT_RTOL, REJECT_ATOL, w)
    b = _solve(dev, 'per_op', make, x0, ticks, REJECT_RTOL, REJECT_ATOL, w)
    rows = [r for r in b[1] if r[0] != 'nfe']
    assert any(r[2] == 0.0 for r in rows) and len(rows) <= 64, (len(rows), sum(r[2] == 0.0 for r in rows))
    _check(a, b)


@pytest.mark.parametrize('shape', ['reference_size', 'fused_width'])
def test_budget_gives_the_same_bits(dev, shape):
    """NDCN_TAPE_BUDGET_MB unset, 0 and a value in between: thin attempts are re-formed with their own evaluation numbers - the same
    masks, hence the same trajectory, log and gradients bit for bit"""
    from ndcn_amd.torchdiffeq._impl import tape
    if shape == 'reference_size':
        make, x0 = _reference_model(dev, 'default', 0.5)
        ticks, rtol, atol, between = [0., 0.3, 0.6, 0.9, 1.0], 1e-3, 1e-5, 1         # 1 MiB: 32 panels of 32 KB - two full attempts
    else:
        make, x0 = _wide_model(dev, 36, False)
        ticks, rtol, atol, between = WIDE_TICKS, WIDE_RTOL, WIDE_ATOL, 20            # 20 MiB: 15 panels of 1.3 MB - one full attempt
    w = torch.randn(len(ticks), *x0.shape, generator=torch.Generator().manual_seed(3))
    full = _solve(dev, 'tape', make, x0, ticks, rtol, atol, w)
    rec_full = dict(tape.last_record)
    attempts = len([r for r in full[1] if r[0] != 'nfe'])
    assert full[3].startswith('_TapeDopri5') and rec_full['thin_attempts'] == 0 and rec_full['full_panels'] == 12 * attempts
    for budget in (0, between):
        thin = _solve(dev, 'tape', make, x0, ticks, rtol, atol, w, budget=budget)
        rec = dict(tape.last_record)
        assert rec['thin_attempts'] == attempts if budget == 0 else 0 < rec['thin_attempts'] < attempts, (budget, rec, attempts)
        assert thin[1] == full[1] and torch.equal(thin[0], full[0])
        assert len(thin[2]) == len(full[2]) == 3
        assert all(torch.equal(x, y) for x, y in zip(thin[2], full[2]))


def test_seeds_eval_mode_and_the_switch(dev):
    """one seed twice: the same bits; another seed: another trajectory; eval() mode: the p = 0 tape; NDCN_TAPE_DROPOUT unset: the
    per-operation graph with one fused node per evaluation, as before the switch existed"""
    make, x0 = _reference_model(dev, 'default', 0.5)
    ticks = [0., 0.3, 0.6, 0.9, 1.0]
    w = torch.randn(len(ticks), *x0.shape, generator=torch.Generator().manual_seed(3))
    a = _solve(dev, 'tape', make, x0, ticks, 1e-3, 1e-5, w, seed=5)
    b = _solve(dev, 'tape', make, x0, ticks, 1e-3, 1e-5, w, seed=5)
    c = _solve(dev, 'tape', make, x0, ticks, 1e-3, 1e-5, w, seed=6)
    assert a[3].startswith('_TapeDopri5')
    assert a[1] == b[1] and torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert not torch.equal(a[0], c[0])
    make0, _ = _reference_model(dev, 'default', 0.0)
    e = _solve(dev, 'tape', make, x0, ticks, 1e-3, 1e-5, w, train=False)
    z = _solve(dev, 'default', make0, x0, ticks, 1e-3, 1e-5, w)
    assert e[3].startswith('_TapeDopri5') and z[3].startswith('_TapeDopri5')
    assert e[1] == z[1] and torch.equal(e[0], z[0]) and all(torch.equal(x, y) for x, y in zip(e[2], z[2]))
    assert not torch.equal(e[0], a[0])
    # the switch unset
    from ndcn_amd import torchdiffeq as ode
    f = make().train()
    y = ode.odeint(f, x0.to(dev).requires_grad_(True), torch.tensor(ticks).to(dev), rtol=1e-3, atol=1e-5, method='dopri5')
    assert '_RhsBackward' in _graph_names(y)


def _graph_names(out):
    names, stack, seen = set(), [out.grad_fn], set()
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        stack.extend(nf for nf, _ in fn.next_functions)
    return names


def test_second_backward_gives_the_same_bits(dev, monkeypatch):
    """retain_graph: the reverse pass runs again over the same record - thin attempts re-formed again with their own numbers"""
    from ndcn_amd import torchdiffeq as ode
    make, x0h = _reference_model(dev, 'default', 0.5)
    for budget in (None, '0'):
        monkeypatch.setenv('NDCN_TAPE_DROPOUT', '1')
        if budget is not None:
            monkeypatch.setenv('NDCN_TAPE_BUDGET_MB', budget)
        f = make().train()
        x0 = x0h.clone().to(dev).requires_grad_(True)
        torch.manual_seed(9)
        y = ode.odeint(f, x0, torch.tensor([0., 0.5, 1.0], device=dev), rtol=1e-3, atol=1e-4, method='dopri5')
        assert type(y.grad_fn).__name__.startswith('_TapeDopri5')
        y.sum().backward(retain_graph=True)
        g1, w1, b1 = x0.grad.clone(), f.wt.weight.grad.clone(), f.wt.bias.grad.clone()
        x0.grad = None
        f.zero_grad(set_to_none=True)
        y.sum().backward()
        assert torch.equal(x0.grad, g1) and torch.equal(f.wt.weight.grad, w1) and torch.equal(f.wt.bias.grad, b1)
        assert float(w1.abs().max()) > 0


def test_the_stream_advances_by_what_the_solve_consumed(dev, monkeypatch):
    """a second evaluation of the same solve scope would continue behind the tape's numbers: 2 + 6 per attempt"""
    from ndcn_amd import dropout as _dropout
    from ndcn_amd.torchdiffeq._impl import tape
    make, x0h = _reference_model(dev, 'default', 0.5)
    monkeypatch.setenv('NDCN_TAPE_DROPOUT', '1')
    f = make().train()
    log = []
    with _dropout.solve_scope() as stream:
        y = tape.solve(f, x0h.clone().to(dev).requires_grad_(True), torch.tensor([0., 0.5, 1.0], device=dev), 1e-3, 1e-4, {}, log)
        assert type(y.grad_fn).__name__.startswith('_TapeDopri5')
        attempts = len([r for r in log if r[0] != 'nfe'])
        assert stream.evaluations == 2 + 6 * attempts == dict(r for r in log if r[0] == 'nfe')['nfe']


def _cora(dev):
    from ndcn_amd import CsrOperator
    import scipy.sparse as sp
    d, g = load_golden('dataset_cora'), load_golden('operators_cora')
    n = int(g['n'])
    feats = sp.csr_matrix((d['feat_data'], d['feat_indices'].astype(np.int64), d['feat_indptr']), shape=tuple(d['feat_shape'])).toarray()
    adj = CsrOperator.from_arrays(g['alpha00_indptr'], g['alpha00_indices'], g['alpha00_data'], (n, n), dev)
    return (adj, torch.from_numpy(feats.astype(np.float32)).to(dev), torch.from_numpy(d['labels'].astype(np.int64)).to(dev),
            torch.from_numpy(d['idx_train'].astype(np.int64)).to(dev))


def test_seeded_dgnn_training_steps_on_the_tape(dev):
    """the dgnn model at its defaults (Cora, hidden 16, dropout 0.5, dopri5 rtol = atol = 0.1) with the switch set: two seeded Adam
    steps repeat bit for bit, the solve is ONE autograd node, and the first loss is the per-operation path's bit for bit (the same
    forward)"""
    import torch.nn as nn
    import torch.nn.functional as F
    from ndcn_amd.neural_dynamics import ODEBlock2, ODEFunc
    adj, feats, labels, idx = _cora(dev)
    t = torch.linspace(0, 2., 5).float().to(dev)

    def run(seed, env, steps=2):
        assert not any(k in os.environ for k in SWITCHES)
        os.environ.update(env)
        try:
            torch.manual_seed(0)
            model = nn.Sequential(nn.Linear(feats.shape[1], 16), nn.Tanh(),
                                  ODEBlock2(ODEFunc(16, adj, dropout=0.5), t, rtol=0.1, atol=0.1, method='dopri5', terminal=True),
                                  nn.Linear(16, int(labels.max()) + 1)).to(dev)
            opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)
            torch.manual_seed(seed)
            model.train()
            losses = []
            for _ in range(steps):
                opt.zero_grad()
                out = model(feats)
                loss = F.cross_entropy(out[idx], labels[idx])
                loss.backward()
                opt.step()
                losses.append(loss.detach().cpu())
            return losses, [p.grad.detach().cpu().clone() for p in model.parameters()], _graph_names(out)
        finally:
            for k in env:
                del os.environ[k]

    la, ga, names = run(17, {'NDCN_TAPE_DROPOUT': '1'})
    lb, gb, _ = run(17, {'NDCN_TAPE_DROPOUT': '1'})
    assert any(nm.startswith('_TapeDopri5') for nm in names) and '_RhsBackward' not in names, sorted(names)
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    assert all(torch.equal(a, b) for a, b in zip(ga, gb))
    assert all(bool(torch.isfinite(g).all()) for g in ga) and float(ga[2].abs().max()) > 0      # (ga[2]: the ODEFunc weight)
    lc, gc, names_c = run(17, {'NDCN_GRAD_TAPE': '0'}, steps=1)
    assert '_RhsBackward' in names_c
    assert torch.equal(la[0], lc[0])
    ld, _, _ = run(18, {'NDCN_TAPE_DROPOUT': '1'}, steps=1)
    assert not torch.equal(la[0], ld[0])
