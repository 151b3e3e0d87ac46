"""TemporalGCN (the drivers' lstm_gnn / gru_gnn / rnn_gnn baselines) with NDCN_TGCN_FUSED on and off, in one process on one model per
case: one Adam step over 79 teacher-forced ticks - forward, l1 loss, backward, optimizer step - and one evaluation (80 input ticks,
future = 20, no gradient), at Hg = 5, Hr = 10 with the Kipf operator, as the drivers run them.  Per case both variants are warmed up,
then timed in blocks that alternate their order (A B, B A, ...); the figure is the median over the blocks of a host clock around a
call that ends in a synchronise, with min and max beside it; torch.cuda.max_memory_allocated of one call of each (the peak counter
reset before it).  Prints one JSON line per row and a table.

    python tools/bench_tgcn.py [--sides 20,316,1000] [--types lstm,gru,rnn] [--blocks 5] [--warmup 2] [--composed_max_side 1000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ndcn_amd import graphs, hip                                # noqa: E402
from ndcn_amd.neural_dynamics import TemporalGCN                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sides', default='20,316,1000')              # N = 400 (the driver default), the 316 x 316 and the 10^6-node lattice
    ap.add_argument('--types', default='lstm,gru,rnn')
    ap.add_argument('--ticks', type=int, default=80)
    ap.add_argument('--future', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--composed_max_side', type=int, default=1000, help='lattices beyond this side are timed fused only')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda:0')
    rows = []
    for side in [int(s) for s in args.sides.split(',') if s]:
        OM = graphs.to_device(graphs.make_operator(graphs.grid_8_neighbor(side), 'kipf'), dev)
        n = side * side
        for rnn_type in [t for t in args.types.split(',') if t]:
            torch.manual_seed(0)
            model = TemporalGCN(1, 5, n, 10, OM, dropout=0.0, rnn_type=rnn_type).to(dev).train()
            opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-3)
            y = torch.rand(n, args.ticks, device=dev)
            routes = {}

            def train(fused):
                hip.set_tgcn_fused(fused)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                opt.zero_grad(set_to_none=True)
                out = model(y[:, :-1])
                torch.nn.functional.l1_loss(out, y[:, 1:]).backward()
                opt.step()
                torch.cuda.synchronize()
                routes['train', fused] = model.last_route
                return 1e3 * (time.perf_counter() - t0)

            def evaluate(fused):
                hip.set_tgcn_fused(fused)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.no_grad():
                    model(y, future=args.future)
                torch.cuda.synchronize()
                routes['eval', fused] = model.last_route
                return 1e3 * (time.perf_counter() - t0)

            variants = (1, 0) if side <= args.composed_max_side else (1,)
            try:
                for what, fn in (('train', train), ('eval', evaluate)):
                    times = {v: [] for v in variants}
                    peak = {}
                    for v in variants:
                        for _ in range(args.warmup):
                            fn(v)
                    for r in range(args.blocks):
                        for v in (variants if r % 2 == 0 else variants[::-1]):
                            times[v].append(fn(v))
                    for v in variants:
                        torch.cuda.empty_cache()
                        torch.cuda.reset_peak_memory_stats(dev)
                        fn(v)
                        peak[v] = torch.cuda.max_memory_allocated(dev) / 2.0 ** 20
                    for v in variants:
                        rows.append({'nodes': n, 'rnn_type': rnn_type, 'what': what, 'NDCN_TGCN_FUSED': v, 'route': routes[what, v],
                                     'ms': statistics.median(times[v]), 'min': min(times[v]), 'max': max(times[v]), 'peak_MiB': peak[v]})
                        print(json.dumps(rows[-1]), flush=True)
            finally:
                hip.set_tgcn_fused(-1)
            del model, opt
            torch.cuda.empty_cache()
    print('\n| nodes | cell | call | NDCN_TGCN_FUSED | ms (median of %d, min .. max) | peak MiB | route |' % args.blocks)
    print('|---|---|---|---|---|---|---|')
    for r in rows:
        print('| %d | %s | %s | %d | %.2f (%.2f .. %.2f) | %.0f | %s |'
              % (r['nodes'], r['rnn_type'], r['what'], r['NDCN_TGCN_FUSED'], r['ms'], r['min'], r['max'], r['peak_MiB'], r['route']))
    by = {(r['nodes'], r['rnn_type'], r['what'], r['NDCN_TGCN_FUSED']): r for r in rows}
    for (n, t, w, v), r in by.items():
        if v == 1 and (n, t, w, 0) in by:
            c = by[n, t, w, 0]
            print('%d %s %s: fused / composed = %.3f x time, %.3f x memory' % (n, t, w, r['ms'] / c['ms'], r['peak_MiB'] / c['peak_MiB']))


if __name__ == '__main__':
    main()
