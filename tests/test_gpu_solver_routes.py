"""Which launch the device-resident solver (csrc/solver.hip) evaluates the right-hand side with, one case per route it decides on in
ndcn_solver_create / ndcn_solver_begin: the path report of the last launch (ndcn_debug_last_rhs_path, exact value), the solver's
counters (attempts, accepted steps, evaluations) and the trajectory against the generic per-operation path - the same function as a
closure, stepped from Python over the stand-alone kernels.  Bits where the suite establishes bits (the RK4 stage algebra in the H = 256
epilogue: test_fused_epilogue_solver_equals_generic_path; the truth dynamics: test_gpu_truth_solver.py), else that test's tolerance,
1e-5 of the trajectory's maximum.

Every case starts from a path report of 0 (a composed launch on two nodes): a solve whose launches report nothing leaves 0 behind.
The solver is driven as odeint drives it: the first tick borrowed, all others in one ndcn_solver_advance_many call, one captured
graph per step where the state is launch-bound and the route has a replayable form."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# route -> (ndcn_debug_last_rhs_path, attempts, accepted, evaluations)
FUSED2, FUSED3, HALO, REC, WIDE, SMALL, EXACT32, DYN = 1, 2, 8, 32, 64, 128, 256, 2048
EXPECT = {
    'mfma_rec_plan-dopri5': (FUSED3, 2, 2, 14),
    'mfma_rec_plan-rk4': (FUSED3, 6, 6, 24),
    'mfma_no_plan-dopri5': (FUSED2, 2, 2, 14),
    'mfma_exact32-dopri5': (EXACT32, 2, 2, 14),
    'rec-dopri5': (REC, 2, 2, 14),
    'rec-rk4': (REC, 4, 4, 16),
    'wide-dopri5': (WIDE, 2, 2, 14),
    'wide-rk4': (WIDE, 4, 4, 16),
    'small-dopri5': (SMALL, 2, 2, 14),
    'composed-rk4': (0, 4, 4, 16),
    'dyn-dopri5': (DYN, 7, 7, 44),
    'dyn-rk4': (DYN, 4, 4, 16),
    'sharded-dopri5': (FUSED3 | HALO, 2, 2, 14),
    'fused1-dopri5': (0, 2, 2, 14),
}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def rhs_path():
    from ndcn_amd import _lib
    return int(_lib.load().ndcn_debug_last_rhs_path())


def clear_path(dev):
    """relu(A X) with a stage sum on two nodes composes (no epilogue route at H = 4) and reports 0"""
    from ndcn_amd import CsrOperator, hip
    A = CsrOperator.from_arrays([0, 1, 2], [0, 1], [1.0, 1.0], (2, 2), dev)
    X = torch.ones(2, 4, device=dev)
    hip.rhs_rk(A, X, None, None, 'combine', X, [], [0.5], no_control=True)
    assert rhs_path() == 0


def lattice(side, dev):
    from ndcn_amd import graphs
    return graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(side)), dev)


def gnp(n, dev):
    from ndcn_amd import graphs
    return graphs.to_device(graphs.normalized_laplacian(graphs.make_graph('random', n, seed=0)), dev)


def odefunc(H, A, dev, seed=3, **kw):
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(seed)
    return ODEFunc(H, A, **kw).to(dev).eval()


def solve(f, x0, t, method, shard=None):
    """(trajectory, (attempts, accepted, evaluations), path report) of one solve on the device-resident solver"""
    from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver, GRAPH_MAX_ELEMS
    n = x0.shape[0]
    clear_path(x0.device)
    s = DeviceSolver(f, n, method, .01, .001, use_graph=shard is None and x0.numel() <= GRAPH_MAX_ELEMS, shard=shard)
    try:
        out = torch.empty((len(t),) + tuple(x0.shape), dtype=torch.float32, device=x0.device)
        out[0].copy_(x0)
        with torch.no_grad():
            s.begin(out[0], t[0], borrow=shard is None)
            s.advance_many(t[1:], out[1:])
        torch.cuda.synchronize()
        st = s.stats()
        return out, (int(st['steps']), int(st['accepted']), int(st['nfe'])), rhs_path()
    finally:
        s.close()


def generic(f, x0, t, method):
    """the same function as a closure: odeint steps from Python over the stand-alone kernels"""
    from ndcn_amd import torchdiffeq as ode
    with torch.no_grad():
        return ode.odeint(lambda tt, y: f(tt, y), x0, torch.tensor(t, dtype=torch.float64, device=x0.device), rtol=.01, atol=.001,
                          method=method)


def check(case, got, want_traj, bits):
    y, counters, path = got
    print('%s: path %d, attempts / accepted / evaluations %s, max |solver - generic| %.3e of max %.3e'
          % (case, path, counters, float((y - want_traj).abs().max()), float(want_traj.abs().max())), flush=True)
    assert (path,) + counters == EXPECT[case]
    if case.endswith('dopri5'):
        assert counters[2] == 2 + 6 * counters[0]                     # f0, the initial step's f1, six per attempt
    else:
        assert counters[0] == counters[1] and counters[2] == 4 * counters[0]
    assert bool(torch.isfinite(y).all())
    if bits:
        assert torch.equal(y, want_traj)
    else:
        assert float((y - want_traj).abs().max()) <= 1e-5 * float(want_traj.abs().max())


T_DOPRI5 = [0., 0.4, 1.0]
T_RK4 = [0., 0.25, 0.5, 0.75, 1.0]


@pytest.mark.parametrize('method', ['dopri5', 'rk4'])
def test_mfma_on_the_record_plan(dev, method):
    """32 x 32 lattice, H = 256: rhs_fused3 with every stage sum in its epilogue"""
    A = lattice(32, dev)
    f = odefunc(256, A, dev)
    x0 = torch.rand(1024, 256, generator=torch.Generator().manual_seed(4)).to(dev)
    t = T_DOPRI5 if method == 'dopri5' else T_RK4 + [1.25, 1.5]
    got = solve(f, x0, t, method)
    assert A.rec is not None
    check('mfma_rec_plan-' + method, got, generic(f, x0, t, method), bits=method == 'rk4')


def test_mfma_without_a_record_plan(dev):
    """500-node G(n,p), H = 256: no locality to plan on - rhs_fused2"""
    A = gnp(500, dev)
    f = odefunc(256, A, dev)
    x0 = torch.rand(500, 256, generator=torch.Generator().manual_seed(4)).to(dev)
    got = solve(f, x0, T_DOPRI5, 'dopri5')
    assert A.rec is None
    check('mfma_no_plan-dopri5', got, generic(f, x0, T_DOPRI5, 'dopri5'), bits=False)


def test_mfma_weights_beyond_the_split_guarantee(dev):
    """the lattice with a weight row spanning 2^24 (test_gpu_split_range._wide_range_weights): the solver learns the range guard's
    verdict when it packs and steps on the fp32 matrix cores"""
    from ndcn_amd import _lib
    from ndcn_amd.ops import invalidate_packed_weights
    A = lattice(32, dev)
    f = odefunc(256, A, dev, seed=0)
    W, b = f.wt.weight.detach().cpu().clone(), f.wt.bias.detach().cpu().clone()
    W[17, :] *= 2.0 ** -24 * 16.0
    W[17, 33] = 1.0
    b[17] = 0.0
    W = W / max(1.0, float(torch.linalg.matrix_norm(W, 2)))
    f.load_state_dict({'wt.weight': W.contiguous(), 'wt.bias': b})
    x0 = torch.rand(1024, 256, generator=torch.Generator().manual_seed(8))
    x0[:, 33] = 0.0
    x0 = x0.to(dev)
    prev = _lib.load().ndcn_set_range_guard(1)
    invalidate_packed_weights()
    try:
        check('mfma_exact32-dopri5', solve(f, x0, T_DOPRI5, 'dopri5'), generic(f, x0, T_DOPRI5, 'dopri5'), bits=False)
    finally:
        _lib.load().ndcn_set_range_guard(prev)
        invalidate_packed_weights()


@pytest.mark.parametrize('method', ['dopri5', 'rk4'])
@pytest.mark.parametrize('route', ['rec', 'wide'])
def test_no_control_in_the_spmm_epilogue(dev, route, method):
    """relu(A X) at H = 256: the group-record SpMM on the lattice, the row SpMM on a graph without a record plan"""
    A = lattice(32, dev) if route == 'rec' else gnp(500, dev)
    n = A.shape[0]
    f = odefunc(256, A, dev, no_control=True)
    x0 = torch.rand(n, 256, generator=torch.Generator().manual_seed(4)).to(dev)
    t = T_DOPRI5 if method == 'dopri5' else T_RK4
    got = solve(f, x0, t, method)
    assert (A.rec is not None) == (route == 'rec')
    check('%s-%s' % (route, method), got, generic(f, x0, t, method), bits=False)


@pytest.mark.parametrize('method', ['dopri5', 'rk4'])
def test_narrow_panels(dev, method):
    """20 x 20 lattice, H = 64: dopri5 steps on rhs_small with the stage sums in its epilogue; rk4 composes its stages, the launch
    behind ndcn_rhs_f32 picks the kernel and reports nothing"""
    A = lattice(20, dev)
    f = odefunc(64, A, dev)
    x0 = torch.rand(400, 64, generator=torch.Generator().manual_seed(4)).to(dev)
    t = T_DOPRI5 if method == 'dopri5' else T_RK4
    check(('small-' if method == 'dopri5' else 'composed-') + method, solve(f, x0, t, method), generic(f, x0, t, method), bits=False)


@pytest.mark.parametrize('method', ['dopri5', 'rk4'])
def test_truth_dynamics(dev, method):
    """heat diffusion of the reference's driver (truth_heat_coo): the module inside the solver against a closure over the SpMM"""
    from ndcn_amd import CsrOperator, HeatDiffusion, hip, torchdiffeq as ode
    d = load_golden('truth_heat_coo')
    n = int(d['x0'].shape[0])
    L = CsrOperator.from_arrays(d['L_indptr'], d['L_indices'], d['L_data'], (n, n), dev)
    x0 = torch.from_numpy(d['x0']).to(dev)
    t = T_DOPRI5 if method == 'dopri5' else T_RK4
    with torch.no_grad():
        want = ode.odeint(lambda tt, x: hip.spmm(L, x, alpha=-1.0), x0, torch.tensor(t, dtype=torch.float64, device=dev), rtol=.01,
                          atol=.001, method=method)
    check('dyn-' + method, solve(HeatDiffusion(L, 1), x0, t, method), want, bits=True)


def test_single_rank_shard(dev):
    """the lattice as ONE shard whose first two lattice rows travel through the exchange (self-halo): every launch goes through
    ndcn_rhs_rk_f32, the last one of a step is a boundary block's"""
    import torch.distributed as dist
    from ndcn_amd import graphs, sharding
    if not dist.is_initialized():
        dist.init_process_group('nccl', init_method='tcp://127.0.0.1:29647', rank=0, world_size=1, device_id=dev)
    try:
        side = 32
        L = graphs.normalized_laplacian(graphs.grid_8_neighbor(side))
        f = odefunc(256, graphs.to_device(L, dev), dev)
        x0 = torch.rand(side * side, 256, generator=torch.Generator().manual_seed(4)).to(dev)
        plan = sharding.HaloPlan(L, [0, side * side], 0, dev, self_halo=2 * side)
        assert plan.n_halo == 2 * side and plan.ranges is not None
        shard = sharding.DeviceShard(plan, side * side)
        try:
            check('sharded-dopri5', solve(f, x0, T_DOPRI5, 'dopri5', shard=shard), generic(f, x0, T_DOPRI5, 'dopri5'), bits=False)
        finally:
            shard.close()
    finally:
        dist.destroy_process_group()


def fused1_child():
    """(in a process started with NDCN_RHS_FUSED2=0) the lattice at H = 256 on the first-generation kernel: packed weights, composed stages"""
    dev = torch.device('cuda:0')
    A = lattice(32, dev)
    f = odefunc(256, A, dev)
    x0 = torch.rand(1024, 256, generator=torch.Generator().manual_seed(4)).to(dev)
    check('fused1-dopri5', solve(f, x0, T_DOPRI5, 'dopri5'), generic(f, x0, T_DOPRI5, 'dopri5'), bits=False)
    return 'ok'


def test_first_generation_kernel_in_a_fresh_process(dev):
    """NDCN_RHS_FUSED2 is read once per process: a child with the switch off"""
    code = ('import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_solver_routes as T; '
            'print("RESULT " + json.dumps(T.fused1_child()), flush=True)' % (os.path.dirname(HERE), HERE))
    p = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, NDCN_RHS_FUSED2='0'), capture_output=True, text=True,
                       timeout=300, cwd=os.path.dirname(HERE))
    print(p.stdout[-2000:], flush=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    assert [l for l in p.stdout.splitlines() if l.startswith('RESULT ')][-1] == 'RESULT ' + json.dumps('ok')
