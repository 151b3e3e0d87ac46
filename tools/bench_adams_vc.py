"""method='adams' with the three-pass step (csrc/adams_vc.hip) against the per-operation calls, in one process.

    python tools/bench_adams_vc.py [--sizes 316x20,316x64,316x256,1000x256] [--pairs 3] [--out FILE]

Per size: odeint(ODEFunc(H) on the S x S 8-neighbour lattice, x0, 5 ticks on [0, 1], method='adams', rtol=1e-3, atol=1e-4) under
torch.no_grad(), one warm-up solve per mode, then `pairs` pairs with hip.set_adams_fused(0) and (1) alternating.  Each solve is timed
by the host clock around work that ends in a device synchronise.  One JSON line per size: milliseconds per attempted step (median
and every sample), attempted steps, the order histogram of the step log, peak device memory per mode, and whether the two
trajectories are the same bits.  A size that does not fit the device is reported as not run.  Needs a ROCm device."""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def solve(f, x0, t, mode):
    from ndcn_amd import hip, torchdiffeq as ode
    hip.set_adams_fused(mode)
    log = []
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    with torch.no_grad():
        y = ode.odeint(f, x0, t, method='adams', rtol=1e-3, atol=1e-4, step_log=log)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    steps = [r for r in log if r[0] != 'nfe']
    return y, steps, wall, torch.cuda.max_memory_allocated()


def run_size(S, H, pairs, dev):
    from ndcn_amd import graphs, hip
    from ndcn_amd.neural_dynamics import ODEFunc
    torch.manual_seed(0)
    f = ODEFunc(H, graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(S)), dev)).to(dev).eval()
    x0 = torch.rand(S * S, H, generator=torch.Generator().manual_seed(1)).to(dev)
    t = torch.linspace(0., 1., 5).to(dev)
    rec = {'lattice': '%dx%d' % (S, S), 'H': H, 'elements': S * S * H, 'above_aten_bound': bool(hip.adams_fusable(x0))}
    try:
        ys = {m: solve(f, x0, t, m)[0] for m in (0, 1)}                    # warm-up, and the results to compare
        rec['same_bits'] = bool(torch.equal(ys[0], ys[1]))
        del ys
        ms, peak = {0: [], 1: []}, {0: 0, 1: 0}
        for _ in range(pairs):
            for m in (0, 1):
                _, steps, wall, mem = solve(f, x0, t, m)
                ms[m].append(1e3 * wall / len(steps))
                peak[m] = max(peak[m], mem)
        rec['attempted_steps'] = len(steps)
        rec['orders'] = dict(sorted(collections.Counter(int(r[2]) for r in steps).items()))
        for m, name in ((0, 'composed'), (1, 'fused')):
            rec['ms_per_step_' + name] = round(statistics.median(ms[m]), 4)
            rec['samples_' + name] = [round(v, 4) for v in ms[m]]
            rec['peak_MB_' + name] = round(peak[m] / 2 ** 20, 1)
        rec['fused_over_composed'] = round(rec['ms_per_step_fused'] / rec['ms_per_step_composed'], 3)
    except torch.cuda.OutOfMemoryError:
        rec['not_run'] = 'out of device memory'
    finally:
        hip.set_adams_fused(-1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='316x20,316x64,316x256,1000x256')
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_adams_vc needs a ROCm device'
    dev = torch.device('cuda:0')
    lines = []
    for s in a.sizes.split(','):
        S, H = (int(v) for v in s.split('x'))
        lines.append(json.dumps(run_size(S, H, a.pairs, dev)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
