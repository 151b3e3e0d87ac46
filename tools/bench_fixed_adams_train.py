"""One Adam step of NDCN(1, H, method='fixed_adams') over 100 ticks - forward, l1 loss, backward, optimizer step - with
NDCN_ADAMS_TRAIN unset (the per-operation graph: what the commit before the node ran, and still the default) and = 1 (one autograd node
per solve: ndcn_fixed_adams_train_f32 forward, the predictor-corrector reverse sweep backward), in one process on one model.  Per case: both variants
are warmed up, then timed in blocks that alternate their order (A B, B A, ...); the figure is the median over the blocks of a host
clock around a step that ends in a synchronise, with min and max beside it; torch.cuda.max_memory_allocated of one step of each
(the peak counter reset before it).  Then the gather kernel ndcn_abm_adjoint_f32 against the two ndcn_ab_adjoint_f32 calls that
would form the same sum (the P half, then the D half onto it - another rounding order, the same panels read) at n = 3 and n = 11 pairs
on panels of the lattice cases: device time per call from events around a run of calls, median over the blocks.  Prints one JSON line
per row and a table.

    python tools/bench_fixed_adams_train.py [--cases lattice316:20,lattice316:64,lattice316:256,pubmed:16] [--ticks 100] [--blocks 5]
                                            [--warmup 2] [--rtol 0.01] [--atol 0.001] [--gather 316x20,316x256]
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
from ndcn_amd.neural_dynamics import NDCN                       # noqa: E402

SWITCH = 'NDCN_ADAMS_TRAIN'


def operator(name):
    if name == 'pubmed':
        g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'operators_pubmed.npz')))
        return sp.csr_matrix((g['alpha00_data'], g['alpha00_indices'], g['alpha00_indptr']), shape=(int(g['n']), int(g['n'])))
    assert name.startswith('lattice'), name
    return graphs.normalized_laplacian(graphs.grid_8_neighbor(int(name[len('lattice'):])))


def gather_rows(spec, blocks, calls=20):
    """the paired gather against two single gathers on panels of side x side rows by H -> rows of the table"""
    dev = torch.device('cuda:0')
    side, H = (int(v) for v in spec.split('x'))
    numel = side * side * H
    rows = []
    for n in (3, 11):
        gen = torch.Generator(device=dev).manual_seed(n)
        ps = [torch.randn(numel, device=dev, generator=gen) for _ in range(n)]
        ds = [torch.randn(numel, device=dev, generator=gen) for _ in range(n)]
        cs = [0.01 * (q + 1) for q in range(n)]
        out = torch.empty(numel, device=dev)
        forms = {'ndcn_abm_adjoint_f32': lambda: hip.abm_adjoint(ps, cs, ds, cs, out=out),
                 '2 x ndcn_ab_adjoint_f32': lambda: hip.ab_adjoint(ds, cs, base=hip.ab_adjoint(ps, cs, out=out), out=out)}
        us = {k: [] for k in forms}
        for k, fn in forms.items():
            fn()
        for r in range(blocks):
            for k in (list(forms) if r % 2 == 0 else list(forms)[::-1]):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    forms[k]()
                b.record()
                b.synchronize()
                us[k].append(1e3 * a.elapsed_time(b) / calls)
        for k in forms:
            rows.append({'gather': k, 'panel': spec, 'elements': numel, 'pairs': n, 'us_per_gradient': statistics.median(us[k]),
                         'min': min(us[k]), 'max': max(us[k])})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='lattice316:20,lattice316:64,lattice316:256,pubmed:16')
    ap.add_argument('--ticks', type=int, default=100)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--t1', type=float, default=0.2)
    ap.add_argument('--rtol', type=float, default=0.01)           # the drivers' tolerances
    ap.add_argument('--atol', type=float, default=0.001)
    ap.add_argument('--gather', default='316x20,316x256')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda:0')
    rows = []
    for case in [c for c in args.cases.split(',') if c]:
        name, H = case.split(':')
        H = int(H)
        L = operator(name)
        n = L.shape[0]
        torch.manual_seed(0)
        model = NDCN(input_size=1, hidden_size=H, A=graphs.to_device(L, dev), num_classes=1, rtol=args.rtol, atol=args.atol,
                     method='fixed_adams').to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        x0 = torch.rand(n, 1, device=dev)
        t = torch.linspace(0., args.t1, args.ticks).to(dev)
        target = torch.rand(args.ticks, n, 1, device=dev)
        nodes, losses = {}, {}

        def step(value):
            os.environ.pop(SWITCH, None)
            if value is not None:
                os.environ[SWITCH] = value
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            opt.zero_grad(set_to_none=True)
            out = model(t, x0)
            nodes[value] = type(out.grad_fn).__name__
            loss = torch.nn.functional.l1_loss(out, target)
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            losses[value] = float(loss)
            return 1e3 * (time.perf_counter() - t0)
        variants = (None, '1')
        times = {v: [] for v in variants}
        peak = {}
        try:
            for v in variants:
                for _ in range(args.warmup):
                    step(v)
            for r in range(args.blocks):
                for v in (variants if r % 2 == 0 else variants[::-1]):
                    times[v].append(step(v))
            for v in variants:
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats(dev)
                step(v)
                peak[v] = torch.cuda.max_memory_allocated(dev) / 2.0 ** 20
        finally:
            os.environ.pop(SWITCH, None)
        for v in variants:
            rows.append({'case': name, 'rows': n, 'H': H, 'ticks': args.ticks, SWITCH: v or 'unset', 'node': nodes[v],
                         'ms_per_step': statistics.median(times[v]), 'min': min(times[v]), 'max': max(times[v]), 'peak_MiB': peak[v],
                         'loss': losses[v]})
        del model, opt
        torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r), flush=True)
    print('\n| case | H | %s | ms / Adam step (median of %d, min .. max) | peak MiB | node |' % (SWITCH, args.blocks))
    print('|---|---|---|---|---|---|')
    for r in rows:
        print('| %s (%d rows) | %d | %s | %.2f (%.2f .. %.2f) | %.0f | %s |'
              % (r['case'], r['rows'], r['H'], r[SWITCH], r['ms_per_step'], r['min'], r['max'], r['peak_MiB'], r['node']))
    for a, b in zip(rows[0::2], rows[1::2]):
        print('%s H = %d: on / off = %.3f x time, %.3f x memory' % (a['case'], a['H'], b['ms_per_step'] / a['ms_per_step'], b['peak_MiB'] / a['peak_MiB']))
    grows = [r for spec in args.gather.split(',') if spec for r in gather_rows(spec, args.blocks)]
    for r in grows:
        print(json.dumps(r), flush=True)
    print('\n| panel | pairs | form | us per gathered gradient (median of %d, min .. max) |' % args.blocks)
    print('|---|---|---|---|')
    for r in grows:
        print('| %s (%d elements) | %d | %s | %.1f (%.1f .. %.1f) |' % (r['panel'], r['elements'], r['pairs'], r['gather'], r['us_per_gradient'], r['min'], r['max']))


if __name__ == '__main__':
    main()
