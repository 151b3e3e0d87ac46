"""The device-resident solver on the one-launch kernels for hidden widths 16..128 (csrc/rhs_mid.hip, csrc/rhs_abl.hip) - the launch kinds
'mid' / 'abl' of csrc/solver.hip under hip.set_solver_mid - against the same solve with the switch off.  The kernels write the composed
launches' bits and the error record is the composed step's own call, so every comparison is torch.equal on raw words plus equal step
logs and nfe.  Shapes: n_rows * H just above 2^18 (below it the solver is 'small' or one launch), where a replayed dopri5 step reads its
coefficients from device memory (c_dev, rhs_mid_epi.h) - the replayed-against-eager equality is the check of that path - and one state
above 2^20 elements, where the eager step keeps its partial sums in the launches (y_aux) and the error record leaves ATen's order.
No public call hands c_dev to the kernels outside the solver: the host-oracle checks of tests/test_gpu_rhs_mid.py cover the by-value
epilogue, the replayed cases here the device-memory one."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (rows, H, operator): whole 64-row tiles and a ragged last tile at H = 16; every width class of the kernels (P = 32, 64, 96, 128)
SHAPES = [(16448, 16, 'lattice'), (16451, 16, 'power'), (13171, 20, 'empty'), (4099, 64, 'power'), (2755, 96, 'lattice'), (2051, 128, 'empty')]
BIG = (16451, 64, 'lattice')                                 # 1 052 864 elements: beyond the ATen-order bound of the error record (2^20)
RTOL, ATOL = 1e-3, 1e-5
# several ticks inside one step, several steps between two ticks
TICKS = [0., .002, .004, .006, .008, 1.5, 3.]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need a ROCm device'
    return torch.device('cuda:0')


_OPS = {}


def operator(n, kind, dev):
    """lattice: the leading n x n block of an 8-neighbour grid; power: preferential attachment, whose hub rows are hundreds of entries
    long (the gather takes four at a time); empty: the lattice with the stored entries of one row inside a tile, and of the last row,
    removed"""
    import scipy.sparse as sp
    from ndcn_amd import graphs
    key = (n, kind)
    if key not in _OPS:
        if kind == 'power':
            A = graphs.barabasi_albert(n, 5, seed=3)
            assert int(np.diff(A.indptr).max()) > 64
            op = graphs.normalized_laplacian(A).tocsr()
        else:
            side = int(np.ceil(np.sqrt(n)))
            op = graphs.normalized_laplacian(graphs.grid_8_neighbor(side)).tocsr()[:n, :n].tocsr()
            if kind == 'empty':
                keep = np.ones(n, dtype=np.float32)
                keep[[77, n - 1]] = 0
                op = (sp.diags(keep) @ op).tocsr()
                op.eliminate_zeros()
                assert op.indptr[78] == op.indptr[77] and op.indptr[n] == op.indptr[n - 1]
        op.sort_indices()
        _OPS[key] = graphs.to_device(op, dev)
    return _OPS[key]


@contextlib.contextmanager
def switch(mode):
    from ndcn_amd import hip
    prev = hip.set_solver_mid(mode)
    try:
        yield
    finally:
        hip.set_solver_mid(prev)


W_SCALE = 3.0                                                # livelier dynamics: the controller rejects now and then


def func(n, H, kind, dev, **abl):
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(H)
    f = ODEFunc(H, operator(n, kind, dev), **abl).to(dev)
    with torch.no_grad():
        f.wt.weight.mul_(W_SCALE)
    return f


def state(n, H, dev):
    return torch.rand(n, H, generator=torch.Generator().manual_seed(n + H)).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


def rhs_path():
    from ndcn_amd import _lib
    return int(_lib.load().ndcn_debug_last_rhs_path())


def odd_panels(n_panels, shape, dev):
    """n_panels contiguous panels that start 4 bytes past a 16-byte boundary"""
    numel = shape[0] * shape[1]
    flat = torch.zeros(n_panels * numel + 4, device=dev)
    view = flat[1:1 + n_panels * numel].view((n_panels,) + tuple(shape))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def solver_run(f, x0, method, use_graph, ticks=TICKS, rtol=RTOL, atol=ATOL, shard=None, odd=False, borrow=False):
    """one solve through DeviceSolver: (trajectory, step log, nfe, kind, path bits).  odd: the caller's panels - the initial state and
    the ticks - are not 16-byte aligned; borrow: dopri5 reads the initial state where the caller keeps it"""
    from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver
    s = DeviceSolver(f, x0.shape[0], method, rtol, atol, use_graph=use_graph, shard=shard)
    try:
        out = torch.empty((len(ticks) - 1,) + tuple(x0.shape), device=x0.device)
        if odd:
            out = odd_panels(len(ticks) - 1, x0.shape, x0.device)
            y0 = odd_panels(1, x0.shape, x0.device)[0]
            y0.copy_(x0)
            x0 = y0
        if borrow:
            s.begin(x0, ticks[0], borrow=True)
        else:
            s.begin(x0, ticks[0])
        s.advance_many(ticks[1:], out)
        torch.cuda.synchronize()
        return out, s.steplog(), int(s.stats()['nfe']), s.rhs_kind(), rhs_path()
    finally:
        s.close()


def same_solve(a, b):
    assert a[1] == b[1], 'step logs differ'
    assert a[2] == b[2], 'nfe differs: %d, %d' % (a[2], b[2])
    assert torch.equal(bits(a[0]), bits(b[0])), 'trajectories differ'


# ------------------------------------------------------------------------------------------------------------------ 1. the kind
def test_kind_follows_the_switch_only_where_no_kind_stood(dev):
    from ndcn_amd import graphs, truth
    from ndcn_amd.neural_dynamics import ODEFunc
    from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver

    def kind(f, n, method='dopri5', use_graph=True):
        s = DeviceSolver(f, n, method, RTOL, ATOL, use_graph=use_graph)
        try:
            return s.rhs_kind()
        finally:
            s.close()

    want = {0: 'composed', 1: 'mid', 2: 'mid'}
    for n, H, op in SHAPES + [BIG]:
        for mode in (0, 1, 2):
            with switch(mode):
                got = kind(func(n, H, op, dev), n)
            assert got == ('composed' if mode == 1 and H > 96 else want[mode]), (n, H, mode, got)
    for abl, H in ((dict(no_control=True), 20), (dict(no_control=True), 64), (dict(no_graph=True), 20), (dict(no_graph=True), 64),
                   (dict(no_graph=True), 128), (dict(no_control=True), 128)):
        for mode in (0, 1, 2):
            for method in ('dopri5', 'rk4', 'euler'):
                with switch(mode):
                    got = kind(func(4099, H, 'power', dev, **abl), 4099, method)
                off = mode == 0 or (mode == 1 and H == 128)
                assert got == ('composed' if off else 'abl'), (abl, H, mode, method, got)
    with switch(2):                                          # midpoint has no epilogue form: it keeps its replayed composed step
        assert kind(func(4099, 64, 'power', dev), 4099, 'midpoint') == 'composed'
    # every solve that has a kind without the switch keeps it
    lat = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(32)), dev)
    small = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(20)), dev)
    heat = truth.HeatDiffusion(graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(20)), dev)).to(dev)
    cases = [('H = 256', lambda: ODEFunc(256, lat).to(dev), 1024, 'dopri5'),
             ('H = 256 no_control, lattice', lambda: ODEFunc(256, lat, no_control=True).to(dev), 1024, 'dopri5'),
             ('H = 256 no_control, power law', lambda: ODEFunc(256, operator(4099, 'power', dev), no_control=True).to(dev), 4099, 'rk4'),
             ('narrow panel', lambda: ODEFunc(64, small).to(dev), 400, 'dopri5'),
             ('truth dynamics', lambda: heat, 400, 'dopri5')]
    seen = set()
    for label, make, n, method in cases:
        kinds = []
        for mode in (0, 1, 2):
            with switch(mode):
                kinds.append(kind(make(), n, method))
        assert kinds[0] == kinds[1] == kinds[2] and kinds[0] not in ('mid', 'abl', 'composed'), (label, kinds)
        seen.add(kinds[0])
    assert {'small', 'dyn'} <= seen and seen & {'mfma', 'fused1'} and seen & {'rec', 'wide'}, seen


def test_a_shard_keeps_its_kind_and_its_bits(dev):
    """a single-rank shard (the lattice as ONE shard whose first two lattice rows travel through the exchange) at a width of the new
    kinds, with graph and control and with no_graph: 'composed' under every mode - a shard dispatches each launch through ndcn_rhs_rk_f32 -
    and the mode-2 dopri5 solve is the mode-0 one"""
    import torch.distributed as dist
    from ndcn_amd import graphs, sharding
    from ndcn_amd.neural_dynamics import ODEFunc
    mine = not dist.is_initialized()
    if mine:
        dist.init_process_group('nccl', init_method='tcp://127.0.0.1:29653', rank=0, world_size=1, device_id=dev)
    try:
        side, H = 32, 64
        n = side * side
        L = graphs.normalized_laplacian(graphs.grid_8_neighbor(side))
        A = graphs.to_device(L, dev)
        x0 = state(n, H, dev)
        for abl in ({}, {'no_graph': True}):
            torch.manual_seed(H)
            f = ODEFunc(H, A, **abl).to(dev)
            plan = sharding.HaloPlan(L, [0, n], 0, dev, self_halo=2 * side)
            shard = sharding.DeviceShard(plan, n)
            try:
                runs = {}
                for mode in (0, 1, 2):
                    with switch(mode):
                        runs[mode] = solver_run(f, x0, 'dopri5', False, ticks=[0., .1, .5, 1.], rtol=.01, atol=.001, shard=shard)
                    assert runs[mode][3] == 'composed', (abl, mode, runs[mode][3])
                assert len(runs[0][1]) >= 2
                same_solve(runs[1], runs[0])
                same_solve(runs[2], runs[0])
            finally:
                shard.close()
    finally:
        if mine:
            dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------------------ 2. dopri5
@pytest.mark.parametrize('n,H,op', SHAPES + [BIG])
def test_dopri5_on_equals_off_replayed_and_eager(dev, n, H, op):
    from ndcn_amd import _lib
    f, x0 = func(n, H, op, dev), state(n, H, dev)
    runs = {}
    for mode in (0, 2):
        for graph in (True, False):
            with switch(mode):
                runs[mode, graph] = solver_run(f, x0, 'dopri5', graph)
    off = runs[0, True]
    accepted = sum(1 for r in off[1] if r[2] == 1.0)
    print('off arm: %d attempts, %d accepted, nfe %d' % (len(off[1]), accepted, off[2]))
    assert accepted >= 3 and len(off[1]) - accepted >= 1, 'the off arm must accept three steps and reject one: %r' % (off[1],)
    assert off[3] == 'composed' and runs[2, True][3] == 'mid' and runs[2, False][3] == 'mid'
    assert off[4] & _lib.PATH_MID == 0 and runs[2, True][4] & _lib.PATH_MID and runs[2, False][4] & _lib.PATH_MID
    same_solve(runs[0, False], off)
    same_solve(runs[2, True], off)                           # replayed: coefficients from device memory
    same_solve(runs[2, False], off)                          # eager: by value
    assert bool(torch.isfinite(off[0]).all())


# ------------------------------------------------------------------------------------------------------------------ 3. fixed grids
@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('n,H,op', [SHAPES[1], SHAPES[2], SHAPES[3], SHAPES[5]])
def test_fixed_grid_on_equals_off(dev, method, n, H, op):
    """(midpoint keeps its kind under the switch - it has no epilogue form - so its cases run the same launches in both arms: they pin
    that the switch leaves it alone, nothing more)"""
    from ndcn_amd import torchdiffeq as ode
    f, x0 = func(n, H, op, dev), state(n, H, dev)
    t = torch.tensor([0., .05, .1, .3, .35]).to(dev)
    res = {}
    for mode in (0, 2):
        with switch(mode), torch.no_grad():
            y = ode.odeint(f, x0, t, method=method)
            g = ode.odeint(f, x0, torch.tensor([0., .03, .13, .31]).to(dev), method=method, options={'step_size': 0.1})   # ticks strictly inside steps
            torch.cuda.synchronize()
            res[mode] = (y, g)
    assert torch.equal(bits(res[0][0]), bits(res[2][0])), 'grid of t'
    assert torch.equal(bits(res[0][1]), bits(res[2][1])), 'step_size grid'
    assert bool(torch.isfinite(res[0][0]).all()) and bool(torch.isfinite(res[0][1]).all())


# ------------------------------------------------------------------------------------------------------------------ 4. the decoder
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('n,H,op', [SHAPES[0], SHAPES[2], SHAPES[3]])
def test_readout_on_equals_off_and_the_decoded_hidden_solve(dev, n, H, op, C):
    from ndcn_amd import hip
    from ndcn_amd import torchdiffeq as ode
    f, x0 = func(n, H, op, dev), state(n, H, dev)
    g = torch.Generator().manual_seed(C)
    Wd, bd = torch.randn(C, H, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    t = torch.tensor(TICKS).to(dev)
    for method in ('dopri5', 'rk4'):
        res = {}
        for mode in (0, 2):
            with switch(mode), torch.no_grad():
                log = []
                kw = dict(rtol=RTOL, atol=ATOL, step_log=log) if method == 'dopri5' else {}
                d = ode.odeint(f, x0, t, method=method, readout=(Wd, bd), **kw)
                hid = ode.odeint(f, x0, t, method=method, **{k: v for k, v in kw.items() if k != 'step_log'})
                torch.cuda.synchronize()
                res[mode] = (d, log, hid)
        assert res[0][1] == res[2][1] and (method != 'dopri5' or len(res[0][1]) > 1)
        assert torch.equal(bits(res[0][0]), bits(res[2][0])), method
        assert torch.equal(bits(res[2][0]), bits(hip.linear(res[2][2], Wd, bd))), method


# ------------------------------------------------------------------------------------------------------------------ 5. the ablations
@pytest.mark.parametrize('abl', ['no_control', 'no_graph'])
@pytest.mark.parametrize('n,H,op', [SHAPES[2], SHAPES[3]])
def test_ablations_on_equal_off(dev, abl, n, H, op):
    from ndcn_amd import _lib
    f, x0 = func(n, H, op, dev, **{abl: True}), state(n, H, dev)
    runs = {}
    for mode in (0, 1):
        with switch(mode):
            for graph in (True, False):
                runs[mode, 'dopri5', graph] = solver_run(f, x0, 'dopri5', graph, ticks=[0., .002, .004, 1., 2.])
            runs[mode, 'rk4'] = solver_run(f, x0, 'rk4', True, ticks=[0., .05, .1, .3])
    off = runs[0, 'dopri5', True]
    assert off[3] == 'composed' and len(off[1]) >= 3
    for graph in (True, False):
        on = runs[1, 'dopri5', graph]
        assert on[3] == 'abl' and on[4] & _lib.PATH_ABL and not off[4] & _lib.PATH_ABL
        same_solve(on, off)
    same_solve(runs[0, 'dopri5', False], off)
    assert runs[1, 'rk4'][3] == 'abl' and runs[0, 'rk4'][3] == 'composed'
    same_solve(runs[1, 'rk4'], runs[0, 'rk4'])


# ------------------------------------------------------------------------------------------------------------------ panels off the 16-byte grid
@pytest.mark.parametrize('abl', [{}, {'no_control': True}])
def test_unaligned_caller_panels_take_the_dispatch_with_the_same_bits(dev, abl):
    """the kernels move 16 bytes per lane; the solver's own panels are aligned, a caller's need not be.  An initial state that dopri5
    reads in place and fixed-grid ticks written where the caller wants them, both 4 bytes off: those launches go through
    ndcn_rhs_rk_f32's dispatch, and the solve is the aligned one's and the switched-off one's"""
    n, H, op = SHAPES[3]
    f, x0 = func(n, H, op, dev, **abl), state(n, H, dev)
    for method, ticks, borrow in (('dopri5', [0., .002, .004, .5, 1.], True), ('rk4', [0., .05, .1, .3], False), ('euler', [0., .05, .1, .3], False)):
        with switch(0):
            off = solver_run(f, x0, method, False, ticks=ticks, odd=True, borrow=borrow)
        with switch(2):
            on = solver_run(f, x0, method, False, ticks=ticks, odd=True, borrow=borrow)
            aligned = solver_run(f, x0, method, False, ticks=ticks, borrow=borrow)
        assert off[3] == 'composed' and on[3] == aligned[3] == ('abl' if abl else 'mid')
        same_solve(on, off)
        same_solve(on, aligned)


# ------------------------------------------------------------------------------------------------------------------ 7. the kept solvers
def test_kept_solver_is_not_shared_across_the_switch(dev):
    from ndcn_amd import _lib
    from ndcn_amd import torchdiffeq as ode
    import importlib
    oi = importlib.import_module('ndcn_amd.torchdiffeq._impl.odeint')         # (the package's attribute of that name is the function)
    n, H, op = SHAPES[3]
    f, x0 = func(n, H, op, dev), state(n, H, dev)
    t = torch.tensor(TICKS).to(dev)
    got = []
    for mode in (0, 2, 0):
        with switch(mode), torch.no_grad():
            log = []
            y = ode.odeint(f, x0, t, rtol=RTOL, atol=ATOL, method='dopri5', step_log=log)
            torch.cuda.synchronize()
            kept = list(oi._SOLVERS.values())[-1][1]            # the solver this solve was handed (most recently used)
            got.append((y, log, rhs_path(), kept.rhs_kind()))
    assert [g[3] for g in got] == ['composed', 'mid', 'composed']
    assert got[0][2] & _lib.PATH_MID == 0 and got[1][2] & _lib.PATH_MID and got[2][2] & _lib.PATH_MID == 0, [hex(g[2]) for g in got]
    assert got[0][1] == got[1][1] == got[2][1]
    assert torch.equal(bits(got[0][0]), bits(got[1][0])) and torch.equal(bits(got[0][0]), bits(got[2][0]))


# ------------------------------------------------------------------------------------------------------------------ 8. non-finite state
def test_nan_in_the_initial_state_raises_as_without_the_switch(dev):
    from ndcn_amd import torchdiffeq as ode
    n, H, op = SHAPES[2]
    f, x0 = func(n, H, op, dev), state(n, H, dev)
    x0[n // 2, 3] = float('nan')
    t = torch.tensor(TICKS).to(dev)
    said = []
    for mode in (0, 2):
        with switch(mode), torch.no_grad(), pytest.raises(AssertionError) as err:
            ode.odeint(f, x0, t, rtol=RTOL, atol=ATOL, method='dopri5')
        said.append(str(err.value))
    assert said[0] == said[1] and said[0], said              # (the initial step's norms are NaN: the refusal names the step size)
