"""ms per grid step of method='explicit_adams' (default order and max_order=4) next to method='rk4', same process, on the S x S lattice
(default 316) at H = 20, 64, 256 over 64 grid steps of a step_size grid (two ticks: no trajectory is stored), and the ndcn_ab_step_f32
launch alone at n = 3 and 11 with its achieved GB/s.  Every variant is warmed up once; the timed rounds alternate the order of the
variants (A B C, C B A, ...); the figure is the median over the rounds of a host clock around a solve that ends in a synchronise.
Prints a table and one JSON line per row.

    python tools/bench_explicit_adams.py [--side 316] [--steps 64] [--rounds 5] [--widths 20,64,256]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ndcn_amd import graphs, hip                                # noqa: E402
from ndcn_amd.neural_dynamics import ODEFunc                    # noqa: E402
from ndcn_amd.torchdiffeq import odeint                         # noqa: E402
from ndcn_amd.torchdiffeq._impl import core                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=316)
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--widths', default='20,64,256')
    ap.add_argument('--dt', type=float, default=1.0 / 512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda:0')
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(args.side)), dev)
    n = args.side * args.side
    t = torch.tensor([0., args.steps * args.dt]).to(dev)
    variants = [('rk4', 'rk4', {'step_size': args.dt}),
                ('explicit_adams', 'explicit_adams', {'step_size': args.dt}),
                ('explicit_adams max_order=4', 'explicit_adams', {'step_size': args.dt, 'max_order': 4})]
    rows = []
    for H in [int(v) for v in args.widths.split(',')]:
        torch.manual_seed(0)
        f = ODEFunc(H, A).to(dev).eval()
        x0 = torch.rand(n, H, device=dev)
        times = {name: [] for name, _, _ in variants}
        finite = {}

        def run(name, method, opts):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                y = odeint(f, x0, t, method=method, options=dict(opts))
            torch.cuda.synchronize()
            finite[name] = bool(torch.isfinite(y[-1]).all())
            return 1e3 * (time.perf_counter() - t0) / args.steps
        for v in variants:                                       # warm-up: code objects, plans, the allocator's blocks
            run(*v)
        for r in range(args.rounds):
            for v in (variants if r % 2 == 0 else variants[::-1]):
                times[v[0]].append(run(*v))
        for name, _, _ in variants:
            rows.append({'kind': 'solve', 'H': H, 'rows': n, 'steps': args.steps, 'variant': name, 'ms_per_step': statistics.median(times[name]),
                         'min': min(times[name]), 'max': max(times[name]), 'finite': finite[name]})
    # the step launch alone, on the widest panel of the list
    H = max(int(v) for v in args.widths.split(','))
    numel = n * H
    y = torch.rand(numel, device=dev)
    out = torch.empty_like(y)
    fs = [torch.rand(numel, device=dev) for _ in range(11)]
    for k in (3, 11):
        a = core.ab_weights(k)
        for _ in range(3):
            hip.ab_step(y, fs[:k], a, 0.01, out=out)
        reps, per = 20, []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                hip.ab_step(y, fs[:k], a, 0.01, out=out)
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) / reps)
        ms = statistics.median(per)
        rows.append({'kind': 'ab_step', 'n': k, 'numel': numel, 'ms': ms, 'GB_per_s': 4.0 * numel * (k + 2) / (ms * 1e-3) / 1e9})
    for r in rows:
        print(json.dumps(r), flush=True)
    print('\n| H | variant | ms / grid step (median of %d, min .. max) | finite |' % args.rounds)
    print('|---|---|---|---|')
    for r in rows:
        if r['kind'] == 'solve':
            print('| %d | %s | %.3f (%.3f .. %.3f) | %s |' % (r['H'], r['variant'], r['ms_per_step'], r['min'], r['max'], r['finite']))
    for r in rows:
        if r['kind'] == 'ab_step':
            print('ab_step n=%d over %d elements: %.3f ms, %.0f GB/s of its %d panel passes' % (r['n'], r['numel'], r['ms'], r['GB_per_s'], r['n'] + 2))


if __name__ == '__main__':
    main()
