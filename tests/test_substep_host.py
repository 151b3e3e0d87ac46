"""CPU tests of the fixed-grid `step_size` option (FixedGridODESolver, solvers.py:39-108): the host plan every path shares
(core.fixed_plan: grid, step sizes, tick placement) against tables and trajectories the reference itself wrote
(tests/golden/substep_*.npz, tools/gen_golden.py gen_substep), core.integrate_fixed driven with the oracle-backed ops double, and the
argument behaviour of odeint.  (The kernels are tested on the GPU in test_gpu_substep.py.)"""
import glob
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from oracle import ndcn_oracle as orc
from ndcn_amd.torchdiffeq._impl import core
from _oracle_ops import OracleOps

torch.set_num_threads(1)
f32 = np.float32


def T(a):
    return torch.from_numpy(np.asarray(a))


def trajectory_fixtures():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'substep_*.npz')))
    return [n for n in names if n not in ('substep_grids', 'substep_adjoint_rk4')]


class Ops(OracleOps):
    """the oracle-backed ops double plus the one op the option adds, as the reference writes it (solvers.py:107-108 with y0 = y1)"""

    @staticmethod
    def tick_emit(y, dt, tms, outs=None):
        dt = torch.tensor(float(dt), dtype=y.dtype)
        return [y + ((y - y) / dt) * torch.tensor(float(tm), dtype=y.dtype) for tm in tms]


def test_fixture_set_is_complete():
    names = trajectory_fixtures()
    for method in ('euler', 'midpoint', 'rk4'):
        for case in ('multiples', 'irregular', 'clamped'):
            assert 'substep_%s_%s' % (method, case) in names
    assert 'substep_rk4_decreasing' in names and 'substep_euler_nocontrol' in names
    assert os.path.exists(os.path.join(GOLDEN, 'substep_adjoint_rk4.npz')) and os.path.exists(os.path.join(GOLDEN, 'substep_grids.npz'))


def test_grid_equals_the_reference_table():
    """(t0, t1, h) -> the reference's grid length, its last three points, and whether its assertion (solvers.py:83) fired"""
    d = load_golden('substep_grids')
    table = d['table']
    assert len(table) >= 300
    for t0, t1, h, n, fired, a, b, c in table:
        t32 = np.array([t0, t1], dtype=f32)
        if fired:
            with pytest.raises(AssertionError):
                core.fixed_plan(t32, h)
            continue
        plan = core.fixed_plan(t32, h)
        assert len(plan.grid) == int(n) and plan.grid.dtype == f32
        last = np.array([np.nan] * 3 + plan.grid.tolist(), dtype=np.float64)[-3:]
        assert np.array_equal(last, np.array([a, b, c]), equal_nan=True), (t0, t1, h)
        assert np.array_equal(plan.dts, plan.grid[1:] - plan.grid[:-1])


def increasing(t):
    t = np.asarray(t, dtype=f32)
    return -t if (t[1:] < t[:-1]).all() else t


@pytest.mark.parametrize('name', trajectory_fixtures())
def test_tick_placement(name):
    """the grid bit for bit, and per tick the row of the reference's own explicit-grid solve it is equal to"""
    d = load_golden(name)
    plan = core.fixed_plan(increasing(d['t']), float(d['h']))
    assert np.array_equal(plan.grid, d['grid'])              # (a decreasing t: the reference's grid on the negated times)
    assert np.array_equal(plan.tick_step[1:] + 1, d['rows'][1:]) and d['rows'][0] == 0
    assert plan.n_emitted == len(d['t'])
    for i, em in enumerate(plan.emits):
        for j, same, tm in em:
            assert same == bool(plan.t[j] == plan.grid[i + 1] or plan.t[j] == plan.grid[i]) and tm == f32(plan.t[j] - plan.grid[i])
    if 'irregular' in name:
        assert max(len(e) for e in plan.emits) >= 2 and min(len(e) for e in plan.emits) == 0
        assert not plan.tick_coincident[1:].all()
    if 'clamped' in name:
        assert plan.dts[-1] < plan.dts[0]


def test_default_plan_is_the_time_vector():
    t = np.array([0., .3, .35, 2.], dtype=f32)
    plan = core.fixed_plan(t)
    assert plan.default and np.array_equal(plan.grid, t)
    assert [[(j, s) for j, s, _ in e] for e in plan.emits] == [[(1, True)], [(2, True)], [(3, True)]]


@pytest.mark.parametrize('name', trajectory_fixtures())
def test_integrate_fixed_reproduces_the_reference(name):
    d = load_golden(name)
    A = orc.coo_from_csr(d['indptr'], d['indices'], d['data'], d['shape'])
    func = orc.OracleODEFunc(A, T(d['W']), T(d['b']), no_control=bool(d['no_control']))
    tensor_input, f, y, tt = core.check_inputs(func, T(d['x0']), T(d['t']))
    plan = core.fixed_plan(tt.numpy(), float(d['h']))
    sol = core.integrate_fixed(Ops, f, y, tt, name.split('_')[1], plan=plan)
    got = torch.stack([s[0] for s in sol]).numpy()
    print('%s: max |difference| to the reference %.3e' % (name, np.abs(got - d['traj']).max()))
    assert np.array_equal(got, d['traj'])


def test_tuple_state_and_several_ticks_in_one_step():
    """a tuple state through the generic path: each tick is the state at the end of the first step that reaches it"""
    f = lambda t, y: (-y[0], 0.5 * y[1])
    y0 = (torch.tensor([1.0, -0.0]), torch.tensor([[2.0]]))
    t = torch.tensor([0., .13, .5, .55, .57, 1.0])
    plan = core.fixed_plan(t.numpy(), 0.1)
    fine = core.integrate_fixed(Ops, f, y0, T(plan.grid), 'rk4')
    sol = core.integrate_fixed(Ops, f, y0, t, 'rk4', plan=plan)
    assert len(sol) == len(t)
    for j in range(1, len(t)):
        for a, b in zip(sol[j], fine[plan.tick_step[j] + 1]):
            assert torch.equal(a, b)


def test_argument_behaviour():
    from ndcn_amd import _lib
    from ndcn_amd import torchdiffeq as ode
    f = lambda t, y: -y
    y0, t = torch.ones(3), torch.tensor([0., 1.])
    with pytest.raises(ValueError, match='step_size and grid_constructor are exclusive arguments.'):
        ode.odeint(f, y0, t, method='euler', options={'grid_constructor': lambda f, y, t: t})
    with pytest.raises(ValueError, match='step_size and grid_constructor are exclusive arguments.'):
        ode.odeint(f, y0, t, method='rk4', options={'step_size': 0.1, 'grid_constructor': lambda f, y, t: t})
    with pytest.raises(NotImplementedError):
        ode.odeint(f, y0, t.clone().requires_grad_(True), method='midpoint', options={'step_size': 0.1})
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        with pytest.raises(_lib.NdcnHipError):               # (host tensors are refused - after the options were looked at)
            ode.odeint(f, y0, t, method='rk4', options={'step_size': 0.5, 'first_step': 0.1})
    msgs = [str(x.message) for x in w if 'Unexpected arguments' in str(x.message)]
    assert msgs == ["RK4: Unexpected arguments {'first_step': 0.1}"]
    with pytest.raises(_lib.NdcnHipError):                   # the option itself is accepted: the refusal is the host tensor's
        ode.odeint(f, y0, t, method='euler', options={'step_size': 0.25})
