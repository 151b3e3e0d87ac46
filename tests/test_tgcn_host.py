"""TemporalGCN without a GPU: the module's constructor, state_dict and parameter count against the reference's (through the fixtures
tests/golden/tgcn_*.npz, tools/gen_golden.py gen_tgcn), the float64 restatement tests/_tgcn.py against the same fixtures, the driver's
refusal of irregular sampling with a discrete baseline, and the declarations of the new calls."""
import inspect
import re

import numpy as np
import pytest
import torch

import _tgcn
from conftest import ROOT, load_golden

TYPES = ('lstm', 'gru', 'rnn')
TOL = 1e-5             # of each tensor's maximum: what gen_tgcn asserts between the reference in float32 and in double


def within(got, want, tol):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) <= tol * float(np.abs(want).max())


@pytest.mark.parametrize('rnn_type', TYPES)
def test_module_has_the_reference_constructor_and_state_dict(rnn_type):
    from ndcn_amd.neural_dynamics import TemporalGCN, GraphConvolution, _HipLinear
    assert list(inspect.signature(TemporalGCN.__init__).parameters) == [
        'self', 'input_size_gnn', 'hidden_size_gnn', 'input_n_graph', 'hidden_size_rnn', 'A', 'dropout', 'rnn_type']
    assert inspect.signature(TemporalGCN.__init__).parameters['dropout'].default == 0.5
    assert inspect.signature(TemporalGCN.__init__).parameters['rnn_type'].default == 'lstm'
    d = load_golden('tgcn_' + rnn_type)
    A = torch.eye(36)
    m = TemporalGCN(1, 5, 36, 10, A, dropout=0.25, rnn_type=rnn_type)
    assert (m.input_size_gnn, m.hidden_size_gnn, m.input_size_rnn, m.hidden_size_rnn, m.output_size) == (1, 5, 180, 10, 36)
    assert m.dropout == 0.25 and m.rnn_type == rnn_type and m.A is A and isinstance(m.dropout_layer, torch.nn.Dropout)
    assert type(m.gc) is GraphConvolution and type(m.linear) is _HipLinear
    assert type(m.rnn) is {'lstm': torch.nn.LSTMCell, 'gru': torch.nn.GRUCell, 'rnn': torch.nn.RNNCell}[rnn_type]
    sd = m.state_dict()
    assert list(sd) == list(_tgcn.PARAMS) == [k for k, _ in m.named_parameters()]
    for k, v in sd.items():
        assert tuple(v.shape) == d[k].shape, k
    assert sum(p.numel() for p in m.parameters()) == _tgcn.param_count(36, 5, 10, rnn_type)


def test_parameter_count_is_the_closed_form_at_the_driver_default():
    from ndcn_amd.neural_dynamics import TemporalGCN
    assert _tgcn.param_count(400, 5, 10, 'lstm') == 84890
    for rnn_type in TYPES:
        m = TemporalGCN(1, 5, 400, 10, None, dropout=0, rnn_type=rnn_type)
        assert sum(p.numel() for p in m.parameters()) == _tgcn.param_count(400, 5, 10, rnn_type)


def test_seeded_initial_draws_follow_the_construction_order():
    """gc, rnn, linear: the order the reference constructs (and therefore draws) in - the same torch classes hold the parameters"""
    from ndcn_amd.neural_dynamics import TemporalGCN
    torch.manual_seed(5)
    m = TemporalGCN(1, 5, 12, 10, None, rnn_type='gru')
    torch.manual_seed(5)
    fc = torch.nn.Linear(1, 5)
    rnn = torch.nn.GRUCell(60, 10)
    lin = torch.nn.Linear(10, 12)
    want = list(fc.parameters()) + list(rnn.parameters()) + list(lin.parameters())
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), want))


@pytest.mark.parametrize('rnn_type', TYPES)
def test_restatement_matches_the_reference(rnn_type):
    d = load_golden('tgcn_' + rnn_type)
    assert within(_tgcn.forward(rnn_type, d['A'], d['X'], d, 0), d['out_future0'], TOL)
    assert within(_tgcn.forward(rnn_type, d['A'], d['X'], d, 3), d['out_future3'], TOL)
    _, grads = _tgcn.loss_and_grads(rnn_type, d['A'], d['X'], d, d['target'])
    for k in _tgcn.PARAMS:
        assert grads[k].shape == d['grad.' + k].shape and within(grads[k], d['grad.' + k], TOL), k


@pytest.mark.parametrize('rnn_type', TYPES)
def test_restated_pieces_compose_to_the_model(rnn_type):
    """proj / cell (what the GPU tests hold the kernels to, one by one) chained = the model of the fixtures"""
    d = load_golden('tgcn_' + rnn_type)
    A, X = d['A'].astype(np.float64), d['X'].astype(np.float64)
    GI = _tgcn.proj(A @ X, A.sum(1), d['gc.fc.weight'], d['gc.fc.bias'], d['rnn.weight_ih'], d['rnn.bias_ih'])
    H, _, _ = _tgcn.cell(rnn_type, GI, d['rnn.weight_hh'], d['rnn.bias_hh'])
    out = (H @ d['linear.weight'].astype(np.float64).T + d['linear.bias']).T
    assert within(out, d['out_future0'], TOL)
    assert _tgcn.proj_min_abs_z(A @ X, A.sum(1), d['gc.fc.weight'], d['gc.fc.bias']) >= 1e-4


@pytest.mark.parametrize('baseline', ['lstm_gnn', 'gru_gnn', 'rnn_gnn'])
def test_driver_refuses_irregular_sampling_with_a_discrete_baseline(baseline, capsys):
    from ndcn_amd.drivers import dynamics
    with pytest.raises(SystemExit) as e:
        dynamics.main('heat', ['--network', 'grid', '--sampled_time', 'irregular', '--baseline', baseline, '--n', '16'])
    assert e.value.code == 2
    assert 'loss2 is never set' in capsys.readouterr().err


def test_calls_are_declared_and_bound():
    from ndcn_amd import _lib, hip
    header = open(ROOT + '/include/ndcn_hip.h').read()
    for name in ('ndcn_tgcn_chunk', 'ndcn_tgcn_proj_ws_bytes', 'ndcn_tgcn_proj_f32', 'ndcn_tgcn_proj_bwd_ws_bytes', 'ndcn_tgcn_proj_bwd_f32',
                 'ndcn_tgcn_cell_f32', 'ndcn_tgcn_cell_bwd_f32'):
        assert name in _lib.SIGNATURES and re.search(r'NDCN_API[^;]*\b%s\(' % name, header), name
    lib = _lib.load()
    assert lib.ndcn_tgcn_chunk(0) >= 80 and lib.ndcn_tgcn_chunk(1) >= 1          # the drivers' 79 / 80 ticks: one pass over W_ih
    assert lib.ndcn_tgcn_proj_ws_bytes(0, 8, 40) == 0
    prev = hip.set_tgcn_fused(0)
    try:
        assert hip.tgcn_fused_on() == 0 and hip.set_tgcn_fused(1) == 0 and hip.tgcn_fused_on() == 1
    finally:
        hip.set_tgcn_fused(-1)
    assert prev in (0, 1)
