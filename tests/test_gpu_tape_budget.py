"""The budgeted dopri5 training tape (csrc/tape.hip: ndcn_tape_dopri5_budget_f32; NDCN_TAPE_BUDGET_MB): attempts past the record budget
keep two panels and the reverse pass re-forms the rest by the forward pass's own launches.  The unlimited tape is held to the
per-operation path by test_gpu_tape.py on these inputs; here the budgeted forms are held to the unlimited one BIT FOR BIT
(trajectory, step log with the evaluation count, every gradient), the record counts to the bounds the code states, the peak
memory to "below the unlimited tape's", and the retry after an allocation failure to a plain budget-0 solve."""
import math
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

MB = 1 << 20


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need a ROCm device'
    return torch.device('cuda:0')


def _solve(dev, budget_mb, make_func, x0_host, ticks, rtol, atol, w_host):
    """one training step's solve under NDCN_TAPE_BUDGET_MB = budget_mb (None: unset) -> (trajectory, log, gradients, last_record)"""
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.torchdiffeq._impl import tape
    assert 'NDCN_TAPE_BUDGET_MB' not in os.environ
    if budget_mb is not None:
        os.environ['NDCN_TAPE_BUDGET_MB'] = str(budget_mb)
    try:
        f = make_func()
        x0 = x0_host.clone().to(dev).requires_grad_(True)
        log = []
        y = ode.odeint(f, x0, torch.tensor(ticks).to(dev), rtol=rtol, atol=atol, method='dopri5', step_log=log)
        assert type(y.grad_fn).__name__.startswith('_TapeDopri5')
        rec = dict(tape.last_record)
        (y * w_host.to(dev)).sum().backward()
        grads = [x0.grad.cpu()] + [p.grad.cpu() for p in f.parameters() if p.grad is not None]
        return y.detach().cpu(), log, grads, rec
    finally:
        os.environ.pop('NDCN_TAPE_BUDGET_MB', None)


def _rows(log):
    return [r for r in log if r[0] != 'nfe']


def _same(a, b):
    assert a[1] == b[1], 'step log (or nfe) differs'
    assert torch.equal(a[0], b[0]), 'trajectory differs'
    assert len(a[2]) == len(b[2])
    for name, ga, gb in zip(('g_y0', 'g_W', 'g_b'), a[2], b[2]):
        assert torch.equal(ga, gb), name + ' differs'


def _middle_budget_mb(rec, n_attempts, panel_bytes, n_full=None):
    """the smallest whole-MB budget under which n_full attempts (default: half of them) are certainly recorded in full: each full
    attempt holds `per` panels (the unlimited run's record), the test before an attempt charges at most 18"""
    per = rec['full_panels'] // n_attempts
    assert per * n_attempts == rec['full_panels'] and 12 <= per <= 18
    n_full = max(1, n_attempts // 2) if n_full is None else n_full
    return max(1, math.ceil((per * (n_full - 1) + 18) * panel_bytes / MB))


def _three_budgets(dev, make, x0, ticks, rtol, atol, w, n_full=None):
    """unset / 0 / a middle value -> the three results, after the bit-identity and thin-count assertions"""
    unl = _solve(dev, None, make, x0, ticks, rtol, atol, w)
    A = len(_rows(unl[1]))
    assert A >= 2
    assert unl[3]['thin_attempts'] == 0 and unl[3]['retried'] is False
    assert unl[3]['full_panels'] >= 12 * A and unl[3]['thin_kept_panels'] == 0 and unl[3]['ring_panels'] == 0
    zero = _solve(dev, 0, make, x0, ticks, rtol, atol, w)
    assert zero[3]['thin_attempts'] == A and zero[3]['full_panels'] == 0
    mb = _middle_budget_mb(unl[3], A, x0.numel() * 4 + 16, n_full(unl[1]) if callable(n_full) else n_full)
    mid = _solve(dev, mb, make, x0, ticks, rtol, atol, w)
    print('attempts %d, %d panels each; budget %d MB: %d full panels, %d thin attempts' %
          (A, unl[3]['full_panels'] // A, mb, mid[3]['full_panels'], mid[3]['thin_attempts']))
    assert 0 < mid[3]['thin_attempts'] < A, (mb, mid[3], A)
    assert mid[3]['full_panels'] > 0
    _same(unl, zero)
    _same(unl, mid)
    return unl, zero, mid


# ---------------------------------------------------------------------------------------------------- 1. bit identity

@pytest.mark.parametrize('variant', ['default', 'no_control', 'no_graph'])
@pytest.mark.parametrize('ticks,rtol,atol', [([0., 0.3, 0.6, 0.9, 1.0], 1e-3, 1e-5), (list(np.linspace(0., 5., 80)), 1e-2, 1e-3)])
def test_budgeted_tape_is_bit_identical_on_the_reference_size(dev, variant, ticks, rtol, atol):
    """400 nodes x 20 hidden: narrow-panel kernels (S on the side with keep_s), ATen-order error norms in a launch of their own"""
    from ndcn_amd import CsrOperator
    from ndcn_amd.neural_dynamics import ODEFunc
    d = load_golden('fixed_rk4_equal')
    x0 = torch.from_numpy(np.asarray(d['x0'], dtype=np.float32))
    w = torch.randn(len(ticks), *x0.shape, generator=torch.Generator().manual_seed(3))

    def make():
        f = ODEFunc(20, CsrOperator.from_arrays(d['indptr'], d['indices'], d['data'], d['shape'], dev), no_control=variant == 'no_control',
                    no_graph=variant == 'no_graph').to(dev)
        f.load_state_dict({'wt.weight': torch.from_numpy(np.asarray(d['W'], dtype=np.float32)),
                           'wt.bias': torch.from_numpy(np.asarray(d['b'], dtype=np.float32))})
        return f

    _three_budgets(dev, make, x0, ticks, rtol, atol, w)


@pytest.mark.parametrize('side,no_control', [(12, False), (12, True), (36, False), (36, True)])
def test_budgeted_tape_is_bit_identical_at_the_fused_width(dev, side, no_control):
    """H = 256: the fused MFMA launches with packed weights; side 36 puts the error record into the seventh launch (the re-run's goes
    to a scratch record) and keeps S panels (ring S panels)"""
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    H = 256
    op = graphs.normalized_laplacian(graphs.grid_8_neighbor(side))
    ticks = [0., 0.4, 0.9, 1.5]
    x0 = torch.rand(side * side, H, generator=torch.Generator().manual_seed(2))
    w = torch.randn(4, side * side, H, generator=torch.Generator().manual_seed(1))

    def make():
        torch.manual_seed(0)
        return ODEFunc(H, graphs.to_device(op, dev), no_control=no_control).to(dev)

    unl, zero, _ = _three_budgets(dev, make, x0, ticks, 1e-3, 1e-4, w)
    assert zero[3]['ring_panels'] <= 16
    if side == 36 and not no_control:
        assert unl[3]['full_panels'] > 12 * len(_rows(unl[1])), 'the case must keep S panels'
        assert zero[3]['ring_panels'] > 10


@pytest.fixture(scope='module')
def power_law(dev):
    """the rejected-attempts case of test_gpu_tape.py, solved once under the three budgets; the middle budget keeps in full as many
    attempts as stand before the LAST rejected one (at most half of all), so that one is thin"""
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    n, H = 1500, 32
    op = graphs.normalized_laplacian(graphs.barabasi_albert(n, 4, seed=1))
    ticks = [0., 0.01, 0.02, 0.9, 1.0, 2.5]
    x0 = 25.0 * torch.rand(n, H, generator=torch.Generator().manual_seed(2))
    w = torch.randn(len(ticks), n, H, generator=torch.Generator().manual_seed(1))

    def make():
        torch.manual_seed(0)
        return ODEFunc(H, graphs.to_device(op, dev)).to(dev)

    def n_full(log):
        rej = [i for i, r in enumerate(_rows(log)) if r[2] == 0.0]
        assert rej and rej[-1] >= 1, 'the case must reject an attempt behind the first'
        return min(rej[-1], len(_rows(log)) // 2)

    return _three_budgets(dev, make, x0, ticks, 1e-5, 1e-7, w, n_full)


def test_budgeted_tape_with_rejected_thin_attempts(power_law):
    unl, zero, mid = power_law
    rows = _rows(unl[1])
    rej = [i for i, r in enumerate(rows) if r[2] == 0.0]
    assert rej, 'a rejection must occur'
    # thin attempts are the last ones (once thin, always thin): attempt i is thin iff i >= A - thin_attempts
    assert rej[-1] >= len(rows) - zero[3]['thin_attempts']
    assert rej[-1] >= len(rows) - mid[3]['thin_attempts'], (rej, mid[3])
    # a rejected thin attempt followed by an accepted one: the pair of panels is handed on, not kept twice
    assert any(rows[i + 1][2] == 1.0 for i in rej if i + 1 < len(rows))


# ---------------------------------------------------------------------------------------------------- 4. record counts

def test_record_counts(power_law):
    """the bounds the code states: budget 0 holds no full panel, two per accepted attempt + one spare pair, a ring of <= 10 + 6;
    unlimited holds >= 12 per attempt"""
    unl, zero, mid = power_law
    rows = _rows(unl[1])
    A, accepted = len(rows), sum(1 for r in rows if r[2] == 1.0)
    assert A >= 8
    assert zero[3]['full_panels'] == 0
    assert zero[3]['thin_kept_panels'] <= 2 * accepted + 2
    assert 10 <= zero[3]['ring_panels'] <= 16
    assert zero[3]['thin_attempts'] == A
    assert unl[3]['full_panels'] >= 12 * A
    thin_acc = sum(1 for r in rows[A - mid[3]['thin_attempts']:] if r[2] == 1.0)
    assert mid[3]['thin_kept_panels'] <= 2 * thin_acc + 2 and mid[3]['ring_panels'] <= 16
    assert mid[3]['full_panels'] >= 12 * (A - mid[3]['thin_attempts'])


# ---------------------------------------------------------------------------------------------------- 2. reverse pass twice

def test_second_backward_through_a_thin_tape(dev, monkeypatch):
    """the retain_graph case of test_gpu_tape.py with every attempt thin: the ring belongs to the forward record, so the pass runs
    again (and row by row) with the same result; once the graph is released, autograd's own error"""
    from ndcn_amd import graphs
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.neural_dynamics import ODEFunc
    from ndcn_amd.torchdiffeq._impl import tape
    op = graphs.normalized_laplacian(graphs.grid_8_neighbor(10))
    torch.manual_seed(0)
    f = ODEFunc(16, graphs.to_device(op, dev)).to(dev)
    x0h = torch.rand(100, 16, generator=torch.Generator().manual_seed(4))
    t = torch.tensor([0., 0.5, 1.0], device=dev)
    # the unlimited tape's gradient
    x0 = x0h.to(dev).requires_grad_(True)
    ode.odeint(f, x0, t, rtol=1e-3, atol=1e-4, method='dopri5').sum().backward()
    g0, w0 = x0.grad.clone(), f.wt.weight.grad.clone()
    f.zero_grad(set_to_none=True)

    monkeypatch.setenv('NDCN_TAPE_BUDGET_MB', '0')
    x0 = x0h.to(dev).requires_grad_(True)
    y = ode.odeint(f, x0, t, rtol=1e-3, atol=1e-4, method='dopri5')
    assert type(y.grad_fn).__name__.startswith('_TapeDopri5')
    assert tape.last_record['thin_attempts'] >= 1 and tape.last_record['full_panels'] == 0
    y.sum().backward(retain_graph=True)
    g1, w1 = x0.grad.clone(), f.wt.weight.grad.clone()
    assert torch.equal(g1, g0) and torch.equal(w1, w0)
    x0.grad = None
    f.zero_grad(set_to_none=True)
    rows = [torch.autograd.grad(y[2, i].sum(), x0, retain_graph=True)[0] for i in range(2)]
    assert not torch.equal(rows[0], rows[1])
    y.sum().backward()
    assert torch.equal(x0.grad, g1) and torch.equal(f.wt.weight.grad, w1)
    with pytest.raises(RuntimeError, match='second time'):
        y.sum().backward()


# ---------------------------------------------------------------------------------------------------- 3. > 24 dense groups in a step

def test_thin_tape_with_more_ticks_in_a_step_than_one_read_back_carries(dev):
    """600 ticks over few accepted steps: the dense output of a thin step is evaluated while the ring holds its derivatives, its
    reverse pass reads the re-formed ones batch after batch"""
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    side, H = 10, 16
    op = graphs.normalized_laplacian(graphs.grid_8_neighbor(side))
    ticks = list(np.linspace(0., 2., 600))
    x0 = torch.rand(side * side, H, generator=torch.Generator().manual_seed(2))
    w = torch.randn(len(ticks), side * side, H, generator=torch.Generator().manual_seed(1))

    def make():
        torch.manual_seed(0)
        return ODEFunc(H, graphs.to_device(op, dev)).to(dev)

    unl = _solve(dev, None, make, x0, ticks, 1e-2, 1e-3, w)
    zero = _solve(dev, 0, make, x0, ticks, 1e-2, 1e-3, w)
    steps = _rows(unl[1])
    assert len(ticks) / max(len(steps), 1) > 7 * 24, (len(steps), 'the case must put > 24 groups into one step')
    assert zero[3]['thin_attempts'] == len(steps) and unl[3]['thin_attempts'] == 0
    _same(unl, zero)


# ---------------------------------------------------------------------------------------------------- 5. peak memory

def test_peak_memory_of_a_training_step(dev):
    """370 x 370 lattice x 64 (35 MB panels), >= 8 attempts: the peak over forward + backward with every attempt thin is strictly
    below the unlimited tape's.  On an MI355X: 19 attempts, 2831 MB (40 kept + 10 ring panels) against 8892 MB (228 panels), ratio 0.318
    (printed by the test; DESIGN.md section 0.1 has the row; no ratio is asserted)."""
    from ndcn_amd import graphs
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.neural_dynamics import ODEFunc
    from ndcn_amd.torchdiffeq._impl import tape
    side, H = 370, 64
    op = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(side)), dev)
    torch.manual_seed(0)
    f = ODEFunc(H, op).to(dev)
    x0h = torch.rand(side * side, H, generator=torch.Generator().manual_seed(2))
    t = torch.tensor([0., 1.0, 2.0], device=dev)
    G = torch.randn(3, side * side, H, generator=torch.Generator().manual_seed(1)).to(dev)
    panel = x0h.numel() * 4
    peaks, recs, logs = {}, {}, {}
    try:
        for budget in (None, '0'):
            if budget is not None:
                os.environ['NDCN_TAPE_BUDGET_MB'] = budget
            f.zero_grad(set_to_none=True)
            x0 = x0h.to(dev).requires_grad_(True)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            log = []
            y = ode.odeint(f, x0, t, rtol=1e-6, atol=1e-8, method='dopri5', step_log=log)
            recs[budget] = dict(tape.last_record)
            (y * G).sum().backward()
            torch.cuda.synchronize()
            peaks[budget] = torch.cuda.max_memory_allocated(dev) - base
            logs[budget] = log
            del y, x0
    finally:
        os.environ.pop('NDCN_TAPE_BUDGET_MB', None)
    A = len(_rows(logs[None]))
    print('peak memory over one step, %d attempts of %.1f MB panels: budget 0 %.1f MB (%d kept + %d ring panels), unlimited %.1f MB '
          '(%d panels), ratio %.3f' % (A, panel / MB, peaks['0'] / MB, recs['0']['thin_kept_panels'], recs['0']['ring_panels'],
                                       peaks[None] / MB, recs[None]['full_panels'], peaks['0'] / peaks[None]))
    assert logs[None] == logs['0'] and A >= 8
    assert recs['0']['full_panels'] == 0 and recs[None]['thin_attempts'] == 0
    assert peaks['0'] < peaks[None]


# ---------------------------------------------------------------------------------------------------- 6. the retry

def _retry_case(dev):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import ODEFunc
    side, H = 36, 256                               # 1.3 MB panels: every panel is an allocator call of its own
    op = graphs.normalized_laplacian(graphs.grid_8_neighbor(side))
    ticks = [0., 0.4, 0.9, 1.5]
    x0 = torch.rand(side * side, H, generator=torch.Generator().manual_seed(2))
    w = torch.randn(4, side * side, H, generator=torch.Generator().manual_seed(1))

    def make():
        torch.manual_seed(0)
        return ODEFunc(H, graphs.to_device(op, dev)).to(dev)
    return make, x0, ticks, w


def test_allocation_failure_under_an_unlimited_budget_retries_with_thin_attempts(dev, monkeypatch):
    """an injected torch.cuda.OutOfMemoryError at the third allocator call of the first solve (no memory is exhausted): one warning,
    one more solve with budget 0, whose results and log are those of a plain budget-0 solve"""
    from ndcn_amd.torchdiffeq._impl import tape
    make, x0, ticks, w = _retry_case(dev)
    plain_zero = _solve(dev, 0, make, x0, ticks, 1e-3, 1e-4, w)
    plain = tape.Tape._alloc
    state = {'first': None, 'calls': 0}

    def failing(self, ctx, nbytes):
        if state['first'] is None:
            state['first'] = self
        if state['first'] is self:
            state['calls'] += 1
            if state['calls'] == 3:
                raise torch.cuda.OutOfMemoryError('injected: the third allocation of the first solve')
        return plain(self, ctx, nbytes)

    monkeypatch.setattr(tape.Tape, '_alloc', failing)
    monkeypatch.setattr(tape, '_retry_warned', False)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        got = _solve(dev, None, make, x0, ticks, 1e-3, 1e-4, w)
        assert state['calls'] == 3
        state.update(first=None, calls=0)
        again = _solve(dev, None, make, x0, ticks, 1e-3, 1e-4, w)          # the warning is given once per process
        assert state['calls'] == 3
    named = [c for c in caught if 'NDCN_TAPE_BUDGET_MB' in str(c.message)]
    assert len(named) == 1 and issubclass(named[0].category, RuntimeWarning)
    for res in (got, again):
        assert res[3]['retried'] is True and res[3]['full_panels'] == 0 and res[3]['thin_attempts'] == len(_rows(res[1]))
        _same(plain_zero, res)                      # (the log: one solve's rows)
    assert plain_zero[3]['retried'] is False


def test_allocation_failure_in_both_runs_propagates(dev, monkeypatch):
    from ndcn_amd.torchdiffeq._impl import tape
    make, x0, ticks, w = _retry_case(dev)
    plain = tape.Tape._alloc
    tapes = []                                      # (kept alive: one entry per solve)

    def failing(self, ctx, nbytes):
        if not any(self is t for t in tapes):
            tapes.append(self)
            self.calls_seen = 0
        self.calls_seen += 1
        if self.calls_seen == 3:
            raise torch.cuda.OutOfMemoryError('injected: the third allocation of every solve')
        return plain(self, ctx, nbytes)

    monkeypatch.setattr(tape.Tape, '_alloc', failing)
    monkeypatch.setattr(tape, '_retry_warned', True)
    with pytest.raises(torch.cuda.OutOfMemoryError, match='injected'):
        _solve(dev, None, make, x0, ticks, 1e-3, 1e-4, w)
    assert [t.calls_seen for t in tapes] == [3, 3]
    # a budget that is set is not overridden: no second run
    del tapes[:]
    with pytest.raises(torch.cuda.OutOfMemoryError, match='injected'):
        _solve(dev, 64, make, x0, ticks, 1e-3, 1e-4, w)
    assert [t.calls_seen for t in tapes] == [3]
