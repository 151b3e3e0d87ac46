"""TemporalGCN on the device (csrc/tgcn.hip, neural_dynamics.TemporalGCN, the drivers' lstm_gnn / gru_gnn / rnn_gnn baselines): the
four kernels one by one against the float64 restatement tests/_tgcn.py at their size edges, determinism, refusals, the module's fused
form against its composed form and against the reference's fixtures (tests/golden/tgcn_*.npz), the routing, and the drivers.

Bounds: outputs within 1e-5 of each tensor's maximum (what the reference's float32 run meets against its own double run,
tools/gen_golden.py gen_tgcn), gradients within 2e-4 of each tensor's maximum (the project's gradient bound)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _tgcn
from conftest import load_golden

pytestmark = pytest.mark.gpu
TYPES = ('lstm', 'gru', 'rnn')
OUT_TOL, GRAD_TOL = 1e-5, 2e-4
NS = (1, 63, 64, 65, 130)
SHAPES = ((1, 1), (5, 10), (8, 16))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def ticks():
    """1, 2 and the edges of both chunk lengths (forward and reverse)"""
    from ndcn_amd import hip
    out = {1, 2}
    for c in (hip.tgcn_chunk(), hip.tgcn_chunk(reverse=True)):
        out |= {c - 1, c, c + 1}
    return sorted(t for t in out if t >= 1)


def err(got, want):
    """max |got - want| over max |want| (0 / 0 = 0)"""
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = float(np.abs(want).max())
    d = float(np.abs(got - want).max())
    return 0.0 if d == 0.0 else d / scale


def D(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def ring(N, rng, dev):
    """a ring with random weights (self, left, right) as a device operator"""
    from ndcn_amd.csr import CsrOperator
    i = np.arange(N)
    rows = np.concatenate([i, i, i])
    cols = np.concatenate([i, (i - 1) % N, (i + 1) % N])
    vals = rng.uniform(0.2, 1.0, 3 * N)
    m = sp.coo_matrix((vals, (rows, cols)), shape=(N, N)).tocsr().astype(np.float32)   # duplicates (N <= 2) are summed
    m.sort_indices()
    return CsrOperator.from_scipy(m, device=dev)


def proj_inputs(N, T, Hg, M, seed):
    rng = np.random.RandomState(seed)
    f = np.float32
    return dict(X=rng.uniform(0.0, 2.0, (N, T)).astype(f), w=rng.normal(0, 1, Hg).astype(f), b=rng.normal(0, 0.5, Hg).astype(f),
                W_ih=(rng.normal(0, 1, (M, N * Hg)) / np.sqrt(N * Hg)).astype(f), b_ih=rng.normal(0, 0.3, M).astype(f),
                GGI=rng.normal(0, 1, (T, M)).astype(f)), rng


def clear_of_the_kink(S, r, w, b):
    """a property of the INPUTS: no Z = s w + r b other than an exact zero lies within float32 rounding of the relu's kink, where the
    float32 and the float64 mask may differ"""
    Z = S[:, None, :].astype(np.float64) * w[None, :, None] + (r[:, None].astype(np.float64) * b[None, :])[:, :, None]
    a = np.abs(Z[np.isfinite(Z)])
    return bool(((a == 0) | (a > 1e-6)).all())


@pytest.mark.parametrize('rnn_type', TYPES)
@pytest.mark.parametrize('Hg,Hr', SHAPES)
def test_proj_and_its_reverse_against_float64(dev, Hg, Hr, rnn_type):
    from ndcn_amd import hip
    M = _tgcn.GATES[rnn_type] * Hr
    worst = [0.0, 0.0]
    for N in NS:
        for T in ticks():
            for draw in range(8):                        # the inputs are drawn again until they are clear of the kink
                p, rng = proj_inputs(N, T, Hg, M, 1000 * N + T + 1000000 * draw)
                A = ring(N, rng, dev)
                S = hip.spmm(A, D(p['X'], dev))
                r = hip.spmm(A, torch.ones(N, device=dev))
                Sn, rn = S.cpu().numpy(), r.cpu().numpy()
                if clear_of_the_kink(Sn, rn, p['w'], p['b']):
                    break
            assert clear_of_the_kink(Sn, rn, p['w'], p['b']), (N, T)
            GI = hip.tgcn_proj(S, r, D(p['w'], dev), D(p['b'], dev), D(p['W_ih'], dev), D(p['b_ih'], dev))
            e = err(GI, _tgcn.proj(Sn, rn, p['w'], p['b'], p['W_ih'], p['b_ih']))
            worst[0] = max(worst[0], e)
            assert e <= OUT_TOL, (N, T, e)
            got = hip.tgcn_proj_bwd(S, r, D(p['w'], dev), D(p['b'], dev), D(p['W_ih'], dev), D(p['GGI'], dev))
            want = _tgcn.proj_bwd(Sn, rn, p['w'], p['b'], p['W_ih'], p['GGI'])
            for name, g, wnt in zip(('g_Wih', 'g_w', 'g_b', 'g_bih'), got, want):
                e = err(g, wnt)
                worst[1] = max(worst[1], e)
                assert e <= GRAD_TOL, (N, T, name, e)
    print('tgcn proj Hg %d M %d: worst output error %.3e, worst gradient error %.3e of maximum' % (Hg, M, worst[0], worst[1]))


def cell_inputs(rnn_type, T, Hr, seed):
    rng = np.random.RandomState(seed)
    f = np.float32
    M = _tgcn.GATES[rnn_type] * Hr
    return dict(GI=rng.normal(0, 1, (T, M)).astype(f), W_hh=(rng.normal(0, 0.5, (M, Hr)) / np.sqrt(Hr)).astype(f),
                b_hh=rng.normal(0, 0.3, M).astype(f), h0=rng.uniform(-0.5, 0.5, Hr).astype(f), c0=rng.uniform(-0.5, 0.5, Hr).astype(f),
                gH=rng.normal(0, 1, (T, Hr)).astype(f))


@pytest.mark.parametrize('rnn_type', TYPES)
@pytest.mark.parametrize('Hg,Hr', SHAPES)
def test_cell_and_its_reverse_against_float64(dev, Hg, Hr, rnn_type):
    from ndcn_amd import hip
    lstm = rnn_type == 'lstm'
    worst = [0.0, 0.0]
    for T in ticks():
        for with_state in (False, True):
            p = cell_inputs(rnn_type, T, Hr, 77 * T + Hr)
            h0, c0 = (p['h0'], p['c0'] if lstm else None) if with_state else (None, None)
            dv = lambda a: None if a is None else D(a, dev)
            H, gates, c_rec, hT, cT = hip.tgcn_cell(rnn_type, D(p['GI'], dev), D(p['W_hh'], dev), D(p['b_hh'], dev), h0=dv(h0), c0=dv(c0))
            wH, whT, wcT = _tgcn.cell(rnn_type, p['GI'], p['W_hh'], p['b_hh'], h0, c0)
            outs = [('H', H, wH), ('hT', hT, whT)] + ([('cT', cT, wcT)] if lstm else [])
            for name, g, wnt in outs:
                e = err(g, wnt)
                worst[0] = max(worst[0], e)
                assert e <= OUT_TOL, (T, with_state, name, e)
            assert torch.equal(hT, H[-1]) and tuple(gates.shape) == (T, 4 * Hr) and (c_rec is not None) == lstm
            got = hip.tgcn_cell_bwd(rnn_type, D(p['gH'], dev), gates, c_rec, H, D(p['W_hh'], dev), h0=dv(h0), c0=dv(c0))
            want = _tgcn.cell_bwd(rnn_type, p['GI'], p['W_hh'], p['b_hh'], p['gH'], h0, c0)
            names = ('GGI', 'g_Whh', 'g_bhh', 'g_h0') + (('g_c0',) if lstm else ())
            for name, g, wnt in zip(names, got, want):
                e = err(g, wnt)
                worst[1] = max(worst[1], e)
                assert e <= GRAD_TOL, (T, with_state, name, e)
            assert (got[4] is not None) == lstm
    print('tgcn cell %s Hr %d: worst output error %.3e, worst gradient error %.3e of maximum' % (rnn_type, Hr, worst[0], worst[1]))


def test_planted_zero_is_masked_and_nan_reaches_GI(dev):
    from ndcn_amd import hip
    N, T, Hg, M = 65, 33, 5, 40
    p, rng = proj_inputs(N, T, Hg, M, 5)
    S = rng.uniform(0.25, 2.0, (N, T)).astype(np.float32)
    r = rng.uniform(0.5, 1.5, N).astype(np.float32)
    w, b = p['w'].copy(), p['b'].copy()
    w[2] = b[2] = 0.0                                    # Z[:, 2, :] = 0 exactly
    w[0], b[0] = 0.5, -1.0
    S[3, 5], r[3] = 2.0, 1.0                             # Z[3, 0, 5] = fma(2, 0.5, -1) = 0 exactly
    assert clear_of_the_kink(S, r, w, b)
    dv = lambda a: D(a, dev)
    GI = hip.tgcn_proj(dv(S), dv(r), dv(w), dv(b), dv(p['W_ih']), dv(p['b_ih']))
    assert err(GI, _tgcn.proj(S, r, w, b, p['W_ih'], p['b_ih'])) <= OUT_TOL
    g_Wih, g_w, g_b, g_bih = hip.tgcn_proj_bwd(dv(S), dv(r), dv(w), dv(b), dv(p['W_ih']), dv(p['GGI']))
    for g, wnt in zip((g_Wih, g_w, g_b, g_bih), _tgcn.proj_bwd(S, r, w, b, p['W_ih'], p['GGI'])):
        assert err(g, wnt) <= GRAD_TOL
    assert float(g_w[2]) == 0.0 and float(g_b[2]) == 0.0 and not g_Wih[:, 2::Hg].any()        # masked in value and in gradient
    # the single planted zero: with one tick only, that element's v and gradient are exactly 0
    S1 = np.ascontiguousarray(S[:, 5:6])
    gW1, gw1, _, _ = hip.tgcn_proj_bwd(dv(S1), dv(r), dv(w), dv(b), dv(p['W_ih']), dv(p['GGI'][:1]))
    assert not gW1[:, 3 * Hg].any()
    want = _tgcn.proj_bwd(S1, r, w, b, p['W_ih'], p['GGI'][:1])
    assert err(gw1, want[1]) <= GRAD_TOL
    # a NaN in one input element reaches every gate of its tick, and only that tick
    S[7, 4] = np.nan
    GI = hip.tgcn_proj(dv(S), dv(r), dv(w), dv(b), dv(p['W_ih']), dv(p['b_ih'])).cpu().numpy()
    assert np.isnan(GI[4]).all() and np.isfinite(np.delete(GI, 4, axis=0)).all()
    want = _tgcn.proj(S, r, w, b, p['W_ih'], p['b_ih'])
    assert err(np.delete(GI, 4, axis=0), np.delete(want, 4, axis=0)) <= OUT_TOL


def test_proj_and_its_reverse_are_deterministic(dev):
    from ndcn_amd import hip
    N, T, Hg, M = 130, 33, 5, 40
    p, rng = proj_inputs(N, T, Hg, M, 9)
    S, r = D(rng.uniform(0, 2, (N, T)), dev), D(rng.uniform(0.5, 1.5, N), dev)
    args = (S, r, D(p['w'], dev), D(p['b'], dev), D(p['W_ih'], dev))
    a, b = hip.tgcn_proj(*args, D(p['b_ih'], dev)), hip.tgcn_proj(*args, D(p['b_ih'], dev))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ga, gb = hip.tgcn_proj_bwd(*args, D(p['GGI'], dev)), hip.tgcn_proj_bwd(*args, D(p['GGI'], dev))
    for x, y in zip(ga, gb):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_kernels_refuse_bad_arguments_before_any_launch(dev):
    from ndcn_amd import _lib, hip
    lib = _lib.load()
    P, st = _lib.ptr, _lib.stream_ptr
    # G * Hr = 68
    GI, W_hh, b_hh = torch.zeros(3, 68, device=dev), torch.zeros(68, 17, device=dev), torch.zeros(68, device=dev)
    with pytest.raises(_lib.NdcnHipError) as e:
        hip.tgcn_cell('lstm', GI, W_hh, b_hh)
    assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.NdcnHipError) as e:
        hip.tgcn_cell_bwd('lstm', torch.zeros(3, 17, device=dev), torch.zeros(3, 68, device=dev), torch.zeros(3, 17, device=dev),
                          torch.zeros(3, 17, device=dev), W_hh)
    assert e.value.code == _lib.EINVAL
    N, T, Hg = 10, 3, 5
    S, r, w, b = torch.ones(N, T, device=dev), torch.ones(N, device=dev), torch.ones(Hg, device=dev), torch.ones(Hg, device=dev)
    with pytest.raises(_lib.NdcnHipError) as e:
        hip.tgcn_proj(S, r, w, b, torch.zeros(68, N * Hg, device=dev), torch.zeros(68, device=dev))
    assert e.value.code == _lib.EINVAL
    # a null panel; g_Wih aliased to W_ih: refused, and the outputs keep their sentinel
    M = 40
    W_ih, b_ih = torch.full((M, N * Hg), 0.25, device=dev), torch.zeros(M, device=dev)
    GI = torch.full((T, M), 7.0, device=dev)
    ws = torch.empty(max(int(lib.ndcn_tgcn_proj_ws_bytes(N, T, M)), 4), dtype=torch.uint8, device=dev)
    assert lib.ndcn_tgcn_proj_f32(None, P(r), P(w), P(b), P(W_ih), P(b_ih), P(GI), P(ws), N, T, Hg, M, st()) == _lib.EINVAL
    GGI = torch.ones(T, M, device=dev)
    g_w, g_b, g_bih = (torch.full((n,), 7.0, device=dev) for n in (Hg, Hg, M))
    ws2 = torch.empty(max(int(lib.ndcn_tgcn_proj_bwd_ws_bytes(N)), 4), dtype=torch.uint8, device=dev)
    assert lib.ndcn_tgcn_proj_bwd_f32(P(S), P(r), P(w), P(b), P(W_ih), P(GGI), P(W_ih), P(g_w), P(g_b), P(g_bih), P(ws2), N, T, Hg, M,
                                      st()) == _lib.EINVAL
    assert lib.ndcn_tgcn_proj_bwd_f32(P(S), None, P(w), P(b), P(W_ih), P(GGI), P(GI), P(g_w), P(g_b), P(g_bih), P(ws2), N, T, Hg, M,
                                      st()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((GI == 7.0).all()) and bool((W_ih == 0.25).all()) and all(bool((x == 7.0).all()) for x in (g_w, g_b, g_bih))


# ------------------------------------------------------------------------------------------------ the module
def set_params(m, d):
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(torch.from_numpy(d[k]))


def fixture_case(rnn_type, dev):
    from ndcn_amd.neural_dynamics import TemporalGCN
    d = load_golden('tgcn_' + rnn_type)
    m = TemporalGCN(1, 5, 36, 10, D(d['A'], dev), dropout=0.0, rnn_type=rnn_type).to(dev)
    set_params(m, d)
    return m, D(d['X'], dev), D(d['target'], dev), d


def lattice_case(rnn_type, dev):
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import TemporalGCN
    A = graphs.grid_8_neighbor(40)
    OM = graphs.to_device(graphs.make_operator(A, 'kipf'), dev)
    torch.manual_seed(3)
    m = TemporalGCN(1, 5, 1600, 10, OM, dropout=0.0, rnn_type=rnn_type).to(dev)
    X = torch.rand(1600, 12, device=dev) * 2
    return m, X, torch.rand(1600, 12, device=dev) * 2, None


def run(m, X, target, fused, future):
    from ndcn_amd import hip
    hip.set_tgcn_fused(1 if fused else 0)
    try:
        m.zero_grad()
        if future:
            with torch.no_grad():
                out = m(X, future=future)
            grads = None
        else:
            out = m(X)
            torch.nn.functional.l1_loss(out, target).backward()
            grads = {k: p.grad.clone() for k, p in m.named_parameters()}
        assert m.last_route == ('fused' if fused else 'composed')
        return out.detach(), grads
    finally:
        hip.set_tgcn_fused(-1)


@pytest.mark.parametrize('case', ['fixture', 'lattice'])
@pytest.mark.parametrize('rnn_type', TYPES)
def test_module_fused_against_composed(dev, rnn_type, case):
    m, X, target, _ = (fixture_case if case == 'fixture' else lattice_case)(rnn_type, dev)
    T = X.shape[1]
    out_c, g_c = run(m, X, target, False, 0)
    out_f, g_f = run(m, X, target, True, 0)
    assert tuple(out_f.shape) == (X.shape[0], T) and err(out_f, out_c.cpu().numpy()) <= OUT_TOL
    assert set(g_f) == set(g_c) == set(_tgcn.PARAMS)
    worst = 0.0
    for k in _tgcn.PARAMS:
        e = err(g_f[k], g_c[k].cpu().numpy())
        worst = max(worst, e)
        assert e <= GRAD_TOL, (k, e)
    out_c3, _ = run(m, X, target, False, 3)
    out_f3, _ = run(m, X, target, True, 3)
    assert tuple(out_f3.shape) == (X.shape[0], T + 3)
    e3 = err(out_f3, out_c3.cpu().numpy())
    print('tgcn module %s %s: future 0 %.3e, future 3 %.3e, gradients %.3e of maximum' % (rnn_type, case, err(out_f, out_c.cpu().numpy()), e3, worst))
    assert e3 <= OUT_TOL
    assert torch.equal(out_f3[:, :T], out_f)              # the teacher-forced part does not depend on the rollout


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
@pytest.mark.parametrize('rnn_type', TYPES)
def test_module_against_the_reference(dev, rnn_type, fused):
    m, X, target, d = fixture_case(rnn_type, dev)
    out0, grads = run(m, X, target, fused, 0)
    out3, _ = run(m, X, target, fused, 3)
    l1 = lambda a, b: float(np.abs(a.cpu().numpy().astype(np.float64) - b).mean())
    assert l1(out0, d['out_future0']) < 1e-4 and l1(out3, d['out_future3']) < 1e-4          # the README's parity bound
    for k in _tgcn.PARAMS:
        assert err(grads[k], d['grad.' + k]) <= GRAD_TOL, k


def test_routing(dev):
    from ndcn_amd.neural_dynamics import TemporalGCN
    m, X, target, d = fixture_case('gru', dev)
    ok = lambda out, n: tuple(out.shape) == (36, n) and bool(torch.isfinite(out).all())
    assert ok(m(X), 8) and m.last_route == 'fused' and m.route_counts == {'fused': 1, 'composed': 0}
    with torch.no_grad():
        assert ok(m(X, future=2), 10) and m.last_route == 'fused'
    assert ok(m(X, future=2), 10) and m.last_route == 'composed'              # a gradient through the fed-back ticks
    assert ok(m(X.clone().requires_grad_()), 8) and m.last_route == 'composed'
    m.eval()
    assert ok(m(X), 8) and m.last_route == 'fused'
    p = TemporalGCN(1, 5, 36, 10, m.A, dropout=0.5, rnn_type='gru').to(dev)
    assert ok(p(X), 8) and p.last_route == 'composed'                          # active dropout in train()
    p.eval()
    assert ok(p(X), 8) and p.last_route == 'fused'
    two = TemporalGCN(2, 5, 36, 10, m.A, dropout=0.0, rnn_type='gru').to(dev)
    two.eval()
    # input width 2 never takes the fused form; forward hands the convolution one column per tick (neural_dynamics.py:210-212), so
    # the composed loop then ends where the reference's does: in the Linear(2, Hg) that is given an N x 1 panel
    assert not two._fusable(X, 0)
    with torch.no_grad(), pytest.raises((AssertionError, RuntimeError)):
        two(X)
    assert two.last_route == 'composed' and two.route_counts == {'fused': 0, 'composed': 1}
    h = m.linear.register_forward_hook(lambda *a: None)
    assert ok(m(X), 8) and m.last_route == 'composed'
    h.remove()
    assert ok(m(X), 8) and m.last_route == 'fused'


@pytest.mark.parametrize('baseline', ['lstm_gnn', 'gru_gnn', 'rnn_gnn'])
def test_driver_trains_the_discrete_baselines(dev, baseline, capsys):
    from ndcn_amd.drivers import dynamics
    argv = ['--network', 'grid', '--sampled_time', 'equal', '--baseline', baseline, '--n', '100', '--test_freq', '10', '--gpu', '0']
    first = dynamics.main('heat', argv + ['--niters', '1'])                    # same seed, same draws: the loss of the first iteration
    res = dynamics.main('heat', argv + ['--niters', '20'])
    text = capsys.readouterr().out
    assert 'Graph Operator Choose: Kipf in GCN' in text and 'Choose model:' + baseline in text and 'Iter 0020| Train Loss' in text
    assert all(np.isfinite(res[k]) for k in ('loss', 'rel', 'train_loss')) and set(res) == {'loss', 'rel', 'train_loss', 'params'}
    assert res['params'] == _tgcn.param_count(100, 5, 10, dynamics.RNN_BASELINES[baseline])
    assert res['train_loss'] < first['train_loss']
