"""Inference of NDCN(1, H, method='explicit_adams' | 'fixed_adams') under no_grad over `--ticks` ticks (every grid step a tick), with the
decoder inside the library's solve (NDCN_ADAMS_READOUT on, the default) against decode-after (hip.set_adams_readout(0): the solve
stores the (T, N, H) trajectory and one Linear runs over it - the only path before the switch existed): ms per grid step and peak
memory, alternating in one process on one model.  Both variants are warmed up; the timed blocks alternate their order (on off, off on,
...); the figure is the median (min .. max) over the blocks of a host clock around a forward that ends in a synchronise; peak =
max_memory_allocated of one forward above what was allocated before it.  The outputs of the two variants are compared word for word.
Prints one JSON line per row, a table, and the on / off ratios.

    python tools/bench_adams_readout.py [--cases lattice316:20,lattice316:64,lattice316:256,pubmed:16] [--methods explicit_adams,fixed_adams]
                                        [--ticks 100] [--blocks 5] [--warmup 2] [--t1 0.2]
"""
import argparse
import contextlib
import io
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
from ndcn_amd import _lib, graphs, hip                          # noqa: E402
from ndcn_amd.neural_dynamics import NDCN                       # noqa: E402


def operator(name):
    if name == 'pubmed':
        g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'operators_pubmed.npz')))
        return sp.csr_matrix((g['alpha00_data'], g['alpha00_indices'], g['alpha00_indptr']), shape=(int(g['n']), int(g['n'])))
    assert name.startswith('lattice'), name
    return graphs.normalized_laplacian(graphs.grid_8_neighbor(int(name[len('lattice'):])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='lattice316:20,lattice316:64,lattice316:256,pubmed:16')
    ap.add_argument('--methods', default='explicit_adams,fixed_adams')
    ap.add_argument('--ticks', type=int, default=100)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--t1', type=float, default=0.2)
    args = ap.parse_args()
    assert args.blocks >= 5, 'at least 5 repetitions'
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda:0')
    lib = _lib.load()
    rows = []
    for case in args.cases.split(','):
        name, H = case.split(':')
        H = int(H)
        A = graphs.to_device(operator(name), dev)
        n = A.shape[0]
        for method in args.methods.split(','):
            torch.manual_seed(0)
            model = NDCN(input_size=1, hidden_size=H, A=A, num_classes=1, rtol=.01, atol=.001, method=method).to(dev).eval()
            x0 = torch.rand(n, 1, device=dev)
            t = torch.linspace(0., args.t1, args.ticks).to(dev)
            route, outs = {}, {}

            def forward(on, keep=False):
                hip.set_adams_readout(on)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.no_grad(), contextlib.redirect_stderr(io.StringIO()):
                    out = model(t, x0)
                torch.cuda.synchronize()
                ms = 1e3 * (time.perf_counter() - t0) / (args.ticks - 1)
                route[on] = int(lib.ndcn_last_readout_path())
                if keep:
                    outs[on] = out
                return ms
            variants = (1, 0)
            times = {v: [] for v in variants}
            peak = {}
            try:
                for v in variants:
                    for _ in range(args.warmup):
                        forward(v)
                for r in range(args.blocks):
                    for v in (variants if r % 2 == 0 else variants[::-1]):
                        times[v].append(forward(v))
                for v in variants:
                    torch.cuda.empty_cache()
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated(dev)
                    torch.cuda.reset_peak_memory_stats(dev)
                    forward(v)
                    peak[v] = (torch.cuda.max_memory_allocated(dev) - base) / 2.0 ** 20
                for v in variants:
                    forward(v, keep=True)
            finally:
                hip.set_adams_readout(-1)
            a, b = outs[1], outs[0]
            nan = torch.isnan(b)
            same = bool(torch.equal(torch.isnan(a), nan) and torch.equal(a.view(torch.int32)[~nan], b.view(torch.int32)[~nan]))
            for v in variants:
                rows.append({'case': name, 'rows': n, 'H': H, 'method': method, 'ticks': args.ticks, 'readout_in_solve': v,
                             'route_bits': route[v], 'ms_per_grid_step': statistics.median(times[v]), 'min': min(times[v]),
                             'max': max(times[v]), 'peak_MiB': peak[v], 'same_words': same, 'finite': bool(torch.isfinite(b).all())})
            del model, outs, a, b
            torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r), flush=True)
    print('\n| case | H | method | decoder in the solve | route bits | ms / grid step (median of %d, min .. max) | peak MiB |' % args.blocks)
    print('|---|---|---|---|---|---|---|')
    for r in rows:
        print('| %s (%d rows) | %d | %s | %s | %d | %.4f (%.4f .. %.4f) | %.1f |'
              % (r['case'], r['rows'], r['H'], r['method'], 'on' if r['readout_in_solve'] else 'off', r['route_bits'],
                 r['ms_per_grid_step'], r['min'], r['max'], r['peak_MiB']))
    for a, b in zip(rows[0::2], rows[1::2]):
        spread = max((a['max'] - a['min']) / a['ms_per_grid_step'], (b['max'] - b['min']) / b['ms_per_grid_step'])
        print('%s H = %d %s: on / off = %.3f x time (spread of the blocks %.1f %%), %.3f x memory, same words: %s'
              % (a['case'], a['H'], a['method'], a['ms_per_grid_step'] / b['ms_per_grid_step'], 100 * spread,
                 a['peak_MiB'] / b['peak_MiB'], a['same_words']))


if __name__ == '__main__':
    main()
