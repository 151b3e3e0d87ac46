"""tests/_small_solve.py - the float32 restatement of the one-launch fixed-grid solve that the GPU tests compare csrc/solve_small.hip
with bit for bit - pinned on the CPU: against the reference's own fixed-grid trajectories and against the float64 oracle on one
operator of every class the GPU tests run."""
import numpy as np
import pytest
import torch

import _small_solve as ss
from conftest import load_golden
from oracle import ndcn_oracle as orc

# the bounds of test_gpu_small_solve.py::test_one_launch_solve_against_the_reference_fixtures
MEAN_BOUND, MAX_BOUND = 1e-5, 2e-4


@pytest.mark.parametrize('name', ['fixed_euler_equal', 'fixed_euler_irregular', 'fixed_midpoint_equal', 'fixed_midpoint_irregular',
                                  'fixed_rk4_equal', 'fixed_rk4_irregular'])
def test_restatement_against_the_reference_fixtures(name):
    """the reference's trajectories (400-node grid, H = 20, 100 ticks) within the bounds the device solve is held to"""
    d = load_golden(name)
    y = ss.solve((d['indptr'], d['indices'], d['data']), d['W'], d['b'], d['x0'], d['t'], name.split('_')[1])
    err = np.abs(y.astype(np.float64) - d['traj'])
    print('%s: mean %.3e max %.3e' % (name, err.mean(), err.max()))
    assert err.mean() < MEAN_BOUND and err.max() < MAX_BOUND


def _operators():
    return {
        'random': (lambda: ss.driver_operator('random'), 20),                         # rows of 25..59 entries
        'power_law': (lambda: ss.driver_operator('power_law'), 20),                   # a hub of 73 entries
        'small_world': (lambda: ss.driver_operator('small_world'), 16),
        'community': (lambda: ss.driver_operator('community'), 20),
        'band18': (lambda: ss.band(300, 18), 16),
        'band19_empty_rows': (lambda: ss.without_nodes(ss.band(300, 19), [0, 7, 150, 299]), 16),
        'band_values': (lambda: ss.band(300, 9, 'values'), 16),
        'band_upper': (lambda: ss.band(300, 9, 'upper'), 16),
        'ring5_h33': (lambda: ss.ring(5), 33),
        'ring1': (lambda: ss.ring(1), 20),
    }


# (the variants are run on the operator the GPU tests run them on)
CASES = [(name, 'default') for name in sorted(_operators())] + [('random', 'no_graph'), ('random', 'no_control')]


@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('name,variant', CASES)
def test_restatement_against_the_float64_oracle(name, variant, method):
    """oracle.ndcn_oracle.odeint in float64 over 5 irregular ticks; states and weights of order 1, so the fixtures' ABSOLUTE bounds (set
    for their states of up to 25) hold with room: the float32 solve differs from the float64 one by rounding alone.  The variants run on
    the operators the GPU tests run them on."""
    make, H = _operators()[name]
    m = make()
    n = m.shape[0]
    rng = np.random.default_rng(3)
    W = (rng.uniform(-1, 1, (H, H)) / np.sqrt(H)).astype(np.float32)
    b = rng.uniform(-0.3, 0.3, H).astype(np.float32)
    y0 = rng.uniform(0, 1, (n, H)).astype(np.float32)
    t = np.array([0.0, 0.13, 0.5, 0.55, 1.0], np.float32)
    kw = dict(no_graph=variant == 'no_graph', no_control=variant == 'no_control')
    y = ss.solve((m.indptr, m.indices, m.data), W, b, y0, t, method, **kw)
    A = orc.coo_from_csr(m.indptr, m.indices, m.data, m.shape).double()
    fo = orc.OracleODEFunc(A, torch.from_numpy(W).double(), torch.from_numpy(b).double(), **kw)
    ref = orc.odeint(fo, torch.from_numpy(y0).double(), torch.from_numpy(t).double(), method=method).numpy()
    assert y.dtype == np.float32 and np.isfinite(y).all()
    err = np.abs(y.astype(np.float64) - ref)
    print('%s %s %s: mean %.3e max %.3e' % (name, method, variant, err.mean(), err.max()))
    assert err.mean() < MEAN_BOUND and err.max() < MAX_BOUND


def test_step_size_emission_and_nan_passing():
    """the pieces no fixture holds: a tick strictly inside a step is y + ((y - y) / dt) * dt - the state for finite values, NaN for an
    infinite one, +0 for -0 - and a coincident tick the state itself; relu_nan passes a NaN and keeps -0; an empty row sums to +0"""
    m = ss.without_nodes(ss.ring(6), [2])
    op = (m.indptr, m.indices, m.data)
    H = 4
    W = np.eye(H, dtype=np.float32)
    y0 = np.ones((6, H), np.float32)
    y0[4, 1] = np.nan
    t = np.array([0.0, 0.05, 0.1, 0.25], np.float32)
    y = ss.solve(op, W, None, y0, t, 'euler', step_size=0.1)
    fine = ss.solve(op, W, None, y0, np.array([0.0, 0.1, 0.2, 0.25], np.float32), 'euler')
    assert ss.same_bits(y[1], fine[1]) and ss.same_bits(y[2], fine[1]) and ss.same_bits(y[3], fine[3])
    # the NaN reaches rows 3, 4, 5 (4 and its neighbours in the ring) after one step - every column: the Linear's chain multiplies it
    # by each weight, zeros included - and row 2 (no entries) never changes
    assert np.array_equal(np.argwhere(np.isnan(fine[1])), [[r, o] for r in (3, 4, 5) for o in range(H)])
    assert ss.same_bits(fine[3][2], y0[2])
    assert np.signbit(ss.relu_nan(np.array([-0.0], np.float32)))[0] and np.isnan(ss.relu_nan(np.array([np.nan], np.float32)))[0]
    assert ss.same_bits(ss.rhs(op, y0, W, None)[2], np.zeros(H, np.float32))
