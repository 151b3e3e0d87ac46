"""dopri5 dense output riding in the step's launches (rhs_fused3.hip: rhs_fused3_dense_kernel; solver.hip: enqueue_attempt) against
the schedule without it, bit for bit: every tick, the step log and the evaluation count.  The kill switch NDCN_DENSE_MID (the
midpoint sum M in k6's panel, no k6 for steps that cover no tick) is read once per process: each configuration runs in a fresh
child process of its own."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import hashlib, sys, torch
sys.path.insert(0, ROOT)
from ndcn_amd import _lib, graphs
from ndcn_amd.neural_dynamics import ODEFunc
from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver

dev = torch.device('cuda:0')
lib = _lib.load()
lib.ndcn_set_aten_norm_max(1 << 12)            # every panel here takes the large-panel (fused error record) path
res = {}


def solver(f, n, rtol, atol):
    return DeviceSolver(f, n, 'dopri5', rtol, atol)


def fused_rhs_bytes():
    # bytes the fused right-hand-side launches were accounted since the last call (ndcn_prof_*: the launcher counts the
    # panels of the variant it picks - 1 P less for <COMBINE, 4> without K)
    nk = lib.ndcn_prof_kinds()
    buf = (_lib.ctypes.c_double * (4 * nk))()
    lib.ndcn_prof_read(buf, nk)
    i = _lib.PROF_KINDS.index('rhs_fused')
    return buf[4 * i + 2], buf[4 * i]


def record(name, s, outs):
    torch.cuda.synchronize()
    # the outputs by digest of their bytes (bit-identical or not; the panels themselves would be gigabytes)
    res[name] = {'log': s.steplog(), 'nfe': s.stats()['nfe'],
                 'outs': [hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest() for o in outs]}


side = SIDE
A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(side)), dev)
torch.manual_seed(0)
f = ODEFunc(256, A).to(dev).eval()
n = side * side
x0 = torch.rand(n, 256, generator=torch.Generator().manual_seed(0)).to(dev)

# one tick per solve, as the bench (borrowed initial state, restarts); the profiler's account of the fused launches on the side
s = solver(f, n, .01, .001)
lib.ndcn_prof_enable(1)
fused_rhs_bytes()                              # drain
outs = []
for rep in range(4):
    s.begin(x0, 0.0, borrow=True)
    o = torch.empty_like(x0)
    assert s.advance(5.0, o)
    outs.append(o)
record('one_tick', s, outs)
res['fused_bytes'], res['fused_launches'] = fused_rhs_bytes()
lib.ndcn_prof_enable(0)
if FULL:
    ticks = [0.1, 0.6, 0.7, 5.0]
    s.begin(x0, 0.0, borrow=True)
    many = torch.empty((len(ticks), n, 256), device=dev)
    s.advance_many(ticks, many)
    record('many', s, [many])
    del many
    s.begin(x0, 0.0)
    outs = []
    for t in ticks:
        o = torch.empty_like(x0)
        assert s.advance(t, o)
        outs.append(o)
    record('tick_by_tick', s, outs)
else:
    # several ticks in one step, one call; then tick by tick (the second tick of a step takes the stored fit)
    ticks = [0.05, 0.1, 0.15, 0.6, 0.61, 2.0, 2.5, 5.0]
    s.begin(x0, 0.0)
    many = torch.empty((len(ticks), n, 256), device=dev)
    s.advance_many(ticks, many)
    record('many', s, [many])
    s.begin(x0, 0.0)
    outs = []
    for t in ticks:
        o = torch.empty_like(x0)
        assert s.advance(t, o)
        outs.append(o)
    record('tick_by_tick', s, outs)
    # a tick exactly at the end of an accepted step (x = 1)
    s.begin(x0, 0.0)
    assert s.advance(5.0, None)
    acc = [r for r in s.steplog() if r[2] == 1.0]
    t_end = acc[1][0] + acc[1][1]
    s.begin(x0, 0.0)
    o = torch.empty_like(x0)
    assert s.advance(t_end, o)
    record('tick_at_t1', s, [o])
    # a step budget that stops short of the tick, then a tick inside the last accepted step, then the tick
    s.begin(x0, 0.0)
    o1 = torch.empty_like(x0)
    assert not s.advance(5.0, o1, step_budget=2)
    last = s.steplog()[-1]
    o2, o3 = torch.zeros_like(x0), torch.zeros_like(x0)
    if last[2] == 1.0:                         # (the budget ended on an accepted step: sample inside it)
        assert s.advance(last[0] + 0.5 * last[1], o2)
    assert s.advance(5.0, o3)
    record('budget', s, [o2, o3])
    s.close()
    # attempts that cover a tick and are rejected: a controller without its safety margin aims at the tolerance itself: about half of its attempts are rejected
    ticks = [0.5 * (i + 1) for i in range(60)]
    s = DeviceSolver(f, n, 'dopri5', .01, .001, max_num_steps=2000, safety=1.)
    s.begin(x0, 0.0, borrow=True)
    many = torch.empty((len(ticks), n, 256), device=dev)
    s.advance_many(ticks, many)
    record('rejected', s, [many])
    s.begin(x0, 0.0)
    outs = []
    for t in ticks:
        o = torch.empty_like(x0)
        assert s.advance(t, o)
        outs.append(o)
    record('rejected_tick_by_tick', s, outs)
s.close()
torch.save(res, OUT)
print('ok')
'''


def run_child(tmp_path, tag, mid, side, full):
    out = str(tmp_path / ('%s.pt' % tag))
    code = CHILD.replace('ROOT', repr(ROOT)).replace('SIDE', str(side)).replace('FULL', str(full)).replace('OUT', repr(out))
    env = dict(os.environ, NDCN_DENSE_MID=mid, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'ok' in r.stdout, r.stderr[-3000:]
    return torch.load(out)


def compare(ref, got, n_rows):
    assert ref.keys() == got.keys()
    # the switch took effect: same launches, and the <COMBINE, 4> launch of every attempt that covers no tick (4 solves to t = 5)
    # went without its K panel
    no_tick = sum(1 for r in ref['one_tick']['log'] if r[0] + r[1] < 5.0)
    assert no_tick >= 1
    assert got['fused_launches'] == ref['fused_launches']
    assert ref['fused_bytes'] - got['fused_bytes'] == 4 * no_tick * n_rows * 256 * 4.0, (ref['fused_bytes'], got['fused_bytes'])
    # restarts of the same solve: the same bits every time
    assert len(set(got['one_tick']['outs'])) == 1
    for k in ref:
        if k.startswith('fused_'):
            continue
        assert ref[k]['log'] == got[k]['log'], k
        assert ref[k]['nfe'] == got[k]['nfe'], k
        assert len(ref[k]['outs']) == len(got[k]['outs'])
        for a, b in zip(ref[k]['outs'], got[k]['outs']):
            assert a == b, k


@pytest.mark.gpu
def test_dense_output_in_the_step_launches_is_bit_identical_128(tmp_path):
    """128^2 lattice, H = 256: one tick per solve, several ticks in one step, a tick at t1, a step budget that stops before the
    tick, rejected attempts that cover a tick, borrowed initial states - switch off / on."""
    ref = run_child(tmp_path, 'off', '0', 128, False)
    rej = ref['rejected']['log']
    ticks = [0.5 * (i + 1) for i in range(60)]
    # the case exists: an attempt that covers a tick is rejected
    assert any(r[2] == 0.0 and any(r[0] < t <= r[0] + r[1] for t in ticks) for r in rej), rej
    assert len([r for r in ref['many']['log'] if r[2] == 1.0]) < 8          # ticks share steps
    compare(ref, run_child(tmp_path, 'on', '1', 128, False), 128 * 128)


@pytest.mark.gpu
def test_dense_output_in_the_step_launches_is_bit_identical_M(tmp_path):
    """The bench's size (1000^2 lattice, H = 256, non-temporal epilogue stores): one tick per solve, and ticks inside the steps
    (the stored fit / the multi-tick kernel on {M, k7}) - switch off / on."""
    ref = run_child(tmp_path, 'off', '0', 1000, True)
    compare(ref, run_child(tmp_path, 'on', '1', 1000, True), 1000 * 1000)
