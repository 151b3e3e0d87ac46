#!/usr/bin/env python3
"""The drivers' ground-truth solve (drivers/dynamics.py: dopri5 at odeint's default tolerances on an N x 1 state), timed two ways in
one process, alternating: the modules of ndcn_amd.truth - the solve runs inside the device solver, its right-hand-side launches
carrying the Runge-Kutta algebra (ndcn_dyn_rk_f32) - against a closure over the stand-alone operation, which steps from Python
through core.integrate_dopri5 (the path every truth solve took before the modules existed; it stays in the tree).

One JSON line per (dynamics, case): wall ms as the median of --reps timed solves after --warmup untimed ones (a host clock around a
solve that ends in a device synchronise), attempts, evaluations, ms per attempt, whether the two trajectories are the same bits, and
the truth_dynamics line of the library's launch profile for one module solve with eager launches (a replayed graph records no
per-launch events).  Cases: the README size (400-node grid), a 10^5-node random graph, 10^6-node grid and power-law graphs; 100 ticks
over T = 5 - T is halved for a case until one closure solve fits --solve_seconds, and the T used is reported.

    python tools/bench_truth.py --out profiles/truth_solve.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {'readme': ('grid', 400), 'random_1e5': ('random', 100000), 'grid_1e6': ('grid', 1000000), 'power_law_1e6': ('power_law', 1000000)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--cases', default=','.join(CASES))
    p.add_argument('--kinds', default='heat,gene,mutualistic')
    p.add_argument('--T', type=float, default=5.0)
    p.add_argument('--ticks', type=int, default=100)
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--solve_seconds', type=float, default=4.0, help='halve T until one closure solve takes no longer than this')
    p.add_argument('--out', default=None, help='append the JSON lines to this file too')
    a = p.parse_args()
    assert a.reps >= 5 and a.warmup >= 2
    from ndcn_amd import graphs, _lib
    from ndcn_amd import torchdiffeq as ode
    from ndcn_amd.drivers.dynamics import truth_rhs
    from ndcn_amd.ops import hip
    from ndcn_amd.torchdiffeq._impl.odeint import DeviceSolver
    from tools._prof import breakdown
    assert torch.cuda.is_available(), 'bench_truth.py measures on a ROCm device'
    dev = torch.device('cuda:0')
    closures = {'heat': lambda A, L: (lambda t, x: hip.spmm(L, x, alpha=-1.0)),
                'gene': lambda A, L: (lambda t, x: hip.gene_rhs(A, x, b=1.0, f=1.0, h=2.0)),
                'mutualistic': lambda A, L: (lambda t, x: hip.mutual_rhs(A, x))}
    for case in a.cases.split(','):
        net, n = CASES[case]
        G = graphs.make_graph(net, n, seed=0, layout=None if net == 'grid' else 'community')
        n = G.shape[0]
        A_op, L_op = graphs.to_device(G, dev), graphs.to_device(graphs.laplacian(G), dev)
        x0 = torch.from_numpy(graphs.x0_blocks(int(np.ceil(np.sqrt(n))))[:n]).to(dev)
        for kind in a.kinds.split(','):
            mod, clo = truth_rhs(kind, A_op, L_op), closures[kind](A_op, L_op)
            T = a.T
            with torch.no_grad():
                while True:
                    t = torch.linspace(0., T, a.ticks).to(dev)
                    ms, _ = timed(lambda: ode.odeint(clo, x0, t, method='dopri5'))
                    if ms <= 1e3 * a.solve_seconds or T < 1e-3:
                        break
                    T /= 2
                logs = {'module': [], 'closure': []}
                runs = {'module': lambda: ode.odeint(mod, x0, t, method='dopri5', step_log=logs['module']),
                        'closure': lambda: ode.odeint(clo, x0, t, method='dopri5', step_log=logs['closure'])}
                times = {'module': [], 'closure': []}
                last = {}
                for i in range(a.warmup + a.reps):
                    for who in ('module', 'closure'):
                        del logs[who][:]
                        ms, last[who] = timed(runs[who])
                        if i >= a.warmup:
                            times[who].append(ms)

                def eager():
                    s = DeviceSolver(mod, n, 'dopri5', use_graph=False)
                    out = torch.empty((a.ticks, n, 1), dtype=torch.float32, device=dev)
                    out[0].copy_(x0)
                    s.begin(out[0], 0.0, borrow=True)
                    s.advance_many(t.double().tolist()[1:], out[1:])
                    torch.cuda.synchronize()
                    s.close()
                bd, _ = breakdown(eager)
            row = {'dynamics': kind, 'case': case, 'network': net, 'n': int(n), 'nnz': int(G.nnz), 'T': T, 'ticks': a.ticks,
                   'same_bits': bool(torch.equal(last['module'], last['closure'])), 'reps': a.reps}
            for who in ('module', 'closure'):
                attempts = len(logs[who]) - 1
                med = statistics.median(times[who])
                row[who] = {'wall_ms_median': round(med, 3), 'wall_ms_min': round(min(times[who]), 3), 'wall_ms_max': round(max(times[who]), 3),
                            'attempts': attempts, 'nfe': int(dict([logs[who][-1]])['nfe']), 'ms_per_attempt': round(med / max(attempts, 1), 4)}
            row['closure_over_module'] = round(row['closure']['wall_ms_median'] / row['module']['wall_ms_median'], 2)
            row['prof_truth_dynamics_eager'] = bd.get('truth_dynamics')
            row['last_rhs_path_has_dyn'] = bool(int(_lib.load().ndcn_debug_last_rhs_path()) & _lib.PATH_DYN)
            line = json.dumps(row)
            print(line, flush=True)
            if a.out:
                with open(a.out, 'a') as fh:
                    fh.write(line + '\n')
        del A_op, L_op, x0


if __name__ == '__main__':
    main()
