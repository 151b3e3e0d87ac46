"""ms per grid step of method='fixed_adams' - the library solve (a plain ODEFunc) and the generic branch (the same function behind a
lambda) - next to method='rk4' and method='explicit_adams', same process, on the S x S lattice (default 316) at H = 20, 64, 256 over 64
grid steps of a step_size grid (two ticks: no trajectory is stored), with the corrector iterations per step that the solve ran.  Every
variant is warmed up once; the timed rounds alternate the order of the variants (A B C D, D C B A, ...); the figure is the median over
the rounds of a host clock around a solve that ends in a synchronise.  Prints one JSON line per row and a table.

    python tools/bench_fixed_adams.py [--side 316] [--steps 64] [--rounds 5] [--widths 20,64,256] [--rtol 0.01] [--atol 0.001]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ndcn_amd import graphs                                     # noqa: E402
from ndcn_amd.neural_dynamics import ODEFunc                    # noqa: E402
from ndcn_amd.torchdiffeq import odeint                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=316)
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--widths', default='20,64,256')
    ap.add_argument('--dt', type=float, default=1.0 / 512)
    ap.add_argument('--rtol', type=float, default=0.01)          # the drivers' tolerances
    ap.add_argument('--atol', type=float, default=0.001)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda:0')
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(args.side)), dev)
    n = args.side * args.side
    t = torch.tensor([0., args.steps * args.dt]).to(dev)
    rows = []
    for H in [int(v) for v in args.widths.split(',')]:
        torch.manual_seed(0)
        f = ODEFunc(H, A).to(dev).eval()
        wrapped = lambda tt, y: f(tt, y)
        x0 = torch.rand(n, H, device=dev)
        variants = [('rk4', f, 'rk4'), ('explicit_adams', f, 'explicit_adams'), ('fixed_adams library solve', f, 'fixed_adams'),
                    ('fixed_adams generic branch', wrapped, 'fixed_adams')]
        times = {v[0]: [] for v in variants}
        info = {}

        def run(name, func, method):
            log = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad(), contextlib.redirect_stderr(io.StringIO()):
                y = odeint(func, x0, t, rtol=args.rtol, atol=args.atol, method=method, options={'step_size': args.dt},
                           step_log=log if method == 'fixed_adams' else None)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / args.steps
            its = [e[0] for e in log if e[0] != 'nfe']
            info[name] = (bool(torch.isfinite(y[-1]).all()), sum(its) / max(1, len(its) - 2) if its else None,
                          sum(1 for e in log if e[0] != 'nfe' and not e[1]))
            return ms
        for v in variants:                                       # warm-up: code objects, plans, the allocator's blocks
            run(*v)
        for r in range(args.rounds):
            for v in (variants if r % 2 == 0 else variants[::-1]):
                times[v[0]].append(run(*v))
        for name, _, _ in variants:
            rows.append({'H': H, 'rows': n, 'steps': args.steps, 'variant': name, 'ms_per_step': statistics.median(times[name]),
                         'min': min(times[name]), 'max': max(times[name]), 'finite': info[name][0],
                         'iterations_per_corrected_step': info[name][1], 'steps_not_converged': info[name][2]})
    for r in rows:
        print(json.dumps(r), flush=True)
    print('\n| H | variant | ms / grid step (median of %d, min .. max) | iterations per corrected step | finite |' % args.rounds)
    print('|---|---|---|---|---|')
    for r in rows:
        it = '-' if r['iterations_per_corrected_step'] is None else '%.2f' % r['iterations_per_corrected_step']
        print('| %d | %s | %.3f (%.3f .. %.3f) | %s | %s |' % (r['H'], r['variant'], r['ms_per_step'], r['min'], r['max'], it, r['finite']))


if __name__ == '__main__':
    main()
