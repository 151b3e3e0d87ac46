"""Un-differentiated solves of ODEFunc at hidden widths 16..128 through the device-resident solver with its one-launch kinds
(hip.set_solver_mid 1 / 2: 'mid' / 'abl', csrc/rhs_mid.hip / csrc/rhs_abl.hip) against the composed solve (0): ms per attempted dopri5
step and per rk4 grid step.  One DeviceSolver per arm is built ONCE, with graph replay wherever odeint would ask for it (the library
declines where the kind has no replayable form), and warmed up - creation, graph capture and instantiation are outside every figure; a
timed solve is begin (not timed: the copy of y0, f0 and the initial-step probe, common to all arms) and then advance_many over the time
vector between two synchronises on a host clock, divided by the attempts of the step log (dopri5, tolerances tight enough for tens of
attempts) or the grid steps (rk4).  The timed blocks alternate their order (0 1 2, 2 1 0, ...); the figure is the median (min .. max)
over the blocks.  The arms' solutions and step logs are compared word for word, and each row names the kind its solver reports.  On a
library without the switch (an earlier commit's tree) only arm 0 exists: --arms 0 there gives the composed solve to hold against this
tree's arm 0.  Prints one JSON line per row, a table, and the ratios to the first arm.

    python tools/bench_solver_mid.py [--cases lattice316:16,...,pubmed:64] [--ablations lattice316:20,lattice316:64,lattice316:128]
                                     [--methods dopri5,rk4] [--arms 0,1,2] [--blocks 7] [--warmup 2] [--rtol 1e-4] [--atol 1e-6]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ndcn_amd import graphs, hip                                # noqa: E402
from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver, GRAPH_MAX_ELEMS   # noqa: E402
from ndcn_amd.neural_dynamics import ODEFunc                    # noqa: E402


def operator(name):
    if name == 'pubmed':
        g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'operators_pubmed.npz')))
        return sp.csr_matrix((g['alpha00_data'], g['alpha00_indices'], g['alpha00_indptr']), shape=(int(g['n']), int(g['n'])))
    assert name.startswith('lattice'), name
    return graphs.normalized_laplacian(graphs.grid_8_neighbor(int(name[len('lattice'):])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='lattice316:16,lattice316:20,lattice316:32,lattice316:64,lattice316:96,lattice316:128,pubmed:16,pubmed:64')
    ap.add_argument('--ablations', default='lattice316:20,lattice316:64,lattice316:128')
    ap.add_argument('--methods', default='dopri5,rk4')
    ap.add_argument('--arms', default='0,1,2')
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rk4-steps', type=int, default=20)
    ap.add_argument('--rtol', type=float, default=1e-4)
    ap.add_argument('--atol', type=float, default=1e-6)
    args = ap.parse_args()
    assert args.blocks >= 5, 'at least 5 repetitions'
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda:0')
    has_switch = hasattr(hip, 'set_solver_mid')              # (an older library: the composed arm only)
    arms = [int(a) for a in args.arms.split(',')]
    assert has_switch or arms == [0], 'this library has no solver switch: --arms 0'
    todo = [(c, {}) for c in args.cases.split(',') if c]
    for c in args.ablations.split(','):
        if c:
            todo += [(c, {'no_control': True}), (c, {'no_graph': True})]
    rows = []
    ops = {}
    for case, abl in todo:
        name, H = case.split(':')
        H = int(H)
        if name not in ops:
            ops[name] = graphs.to_device(operator(name), dev)
        A = ops[name]
        n = A.shape[0]
        torch.manual_seed(0)
        f = ODEFunc(H, A, **abl).to(dev)
        x0 = torch.rand(n, H, generator=torch.Generator().manual_seed(1)).to(dev)
        for method in args.methods.split(','):
            ticks = (torch.linspace(0., 2., 5) if method == 'dopri5' else torch.linspace(0., 0.5, args.rk4_steps + 1)).tolist()
            use_graph = x0.numel() <= GRAPH_MAX_ELEMS          # odeint's rule
            solvers, kinds, outs, logs = {}, {}, {}, {}
            out = torch.empty((len(ticks) - 1, n, H), device=dev)

            def solve(arm, keep=False):
                sv = solvers[arm]
                sv.begin(x0, ticks[0])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sv.advance_many(ticks[1:], out)
                torch.cuda.synchronize()
                ms = 1e3 * (time.perf_counter() - t0)
                log = sv.steplog()
                steps = len(log) if method == 'dopri5' else args.rk4_steps
                if keep:
                    outs[arm], logs[arm] = out.clone(), log
                return ms / steps
            times = {a: [] for a in arms}
            try:
                for a in arms:
                    if has_switch:
                        hip.set_solver_mid(a)
                    solvers[a] = DeviceSolver(f, n, method, args.rtol, args.atol, use_graph=use_graph)
                    kinds[a] = solvers[a].rhs_kind() if hasattr(solvers[a], 'rhs_kind') else 'n/a'
                    for _ in range(args.warmup):
                        solve(a)
                for r in range(args.blocks):
                    for a in (arms if r % 2 == 0 else arms[::-1]):
                        times[a].append(solve(a))
                for a in arms:
                    solve(a, keep=True)
            finally:
                if has_switch:
                    hip.set_solver_mid(-1)
                for sv in solvers.values():
                    sv.close()
            same = all(logs[a] == logs[arms[0]] and torch.equal(outs[a].view(torch.int32), outs[arms[0]].view(torch.int32)) for a in arms)
            for a in arms:
                rows.append({'case': name, 'rows': n, 'H': H, 'variant': '+'.join(sorted(abl)) or 'graph+control', 'method': method,
                             'solver_mid': a, 'kind': kinds[a], 'graph_asked': bool(use_graph), 'steps': len(logs[a]) if method == 'dopri5' else args.rk4_steps,
                             'ms_per_step': statistics.median(times[a]), 'min': min(times[a]), 'max': max(times[a]), 'same_words': same})
            del outs, logs, out
        del f
        torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r), flush=True)
    print('\n| case | H | variant | method | NDCN_SOLVER_MID | kind | steps | ms / step (median of %d, min .. max) | x of arm 0 | spread |' % args.blocks)
    print('|---|---|---|---|---|---|---|---|---|---|')
    base = {}
    for r in rows:
        key = (r['case'], r['H'], r['variant'], r['method'])
        if r['solver_mid'] == arms[0]:
            base[key] = r
        b = base[key]
        spread = max((r['max'] - r['min']) / r['ms_per_step'], (b['max'] - b['min']) / b['ms_per_step'])
        print('| %s (%d rows) | %d | %s | %s | %d | %s | %d | %.4f (%.4f .. %.4f) | %.3f | %.1f %% |'
              % (r['case'], r['rows'], r['H'], r['variant'], r['method'], r['solver_mid'], r['kind'], r['steps'], r['ms_per_step'], r['min'],
                 r['max'], r['ms_per_step'] / b['ms_per_step'], 100 * spread))
    print('same words and step logs in every arm: %s' % all(r['same_words'] for r in rows))


if __name__ == '__main__':
    main()
