#!/usr/bin/env python3
"""What thin attempts cost in time (measurement aid, not the judged bench line): one Adam step through dopri5 on the 100k-node grid
with H = 256 - the case of tools/bench_train.py / profiles/r06g_train_step.jsonl - with every attempted step of the training tape
re-formed in the reverse pass (NDCN_TAPE_BUDGET_MB=0) against the unlimited record, alternating in one process; the median of
--reps timed steps after --warmup untimed ones per form.  Every timed repetition is the same Adam step (parameters and optimizer
moments put back outside the timed region).  Prints one JSON line."""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=316)
    ap.add_argument('--hidden', type=int, default=256)
    ap.add_argument('--ticks', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    from ndcn_amd import graphs
    from ndcn_amd.neural_dynamics import NDCN
    from ndcn_amd.torchdiffeq._impl import tape
    dev = torch.device('cuda:0')
    side, H = args.side, args.hidden
    n = side * side
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(side)), dev)
    torch.manual_seed(0)
    model = NDCN(input_size=1, hidden_size=H, A=A, num_classes=1, rtol=.01, atol=.001, method='dopri5').to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=1e-3)
    x0 = torch.from_numpy(graphs.x0_blocks(side)[:n]).to(dev)
    t = torch.linspace(0., 5., args.ticks).to(dev)
    target = torch.rand(n, args.ticks, device=dev)

    def step():
        opt.zero_grad()
        loss = F.l1_loss(model(t, x0).squeeze().t(), target)
        loss.backward()
        opt.step()

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    frozen = (copy.deepcopy(model.state_dict()), copy.deepcopy(opt.state_dict()))

    def rewind():
        model.load_state_dict(frozen[0])
        opt.load_state_dict(copy.deepcopy(frozen[1]))
        torch.cuda.synchronize()

    forms = {'unlimited': None, 'budget_0': '0'}
    times = {k: [] for k in forms}
    peaks, records = {}, {}
    for r in range(args.warmup + args.reps):
        for name, value in forms.items():
            os.environ.pop('NDCN_TAPE_BUDGET_MB', None)
            if value is not None:
                os.environ['NDCN_TAPE_BUDGET_MB'] = value
            rewind()
            torch.cuda.reset_peak_memory_stats(dev)
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append(time.perf_counter() - t0)
            peaks[name] = torch.cuda.max_memory_allocated(dev)
            records[name] = dict(tape.last_record)
    os.environ.pop('NDCN_TAPE_BUDGET_MB', None)
    med = {k: 1e3 * float(np.median(v)) for k, v in times.items()}
    print(json.dumps({'case': '%d-node grid, H=%d, dopri5, %d ticks: one Adam step' % (n, H, args.ticks), 'reps': args.reps,
                      'warmup': args.warmup, 'ms_unlimited': round(med['unlimited'], 3), 'ms_budget_0': round(med['budget_0'], 3),
                      'budget_0_over_unlimited': round(med['budget_0'] / med['unlimited'], 3),
                      'all_ms': {k: [round(1e3 * x, 3) for x in v] for k, v in times.items()},
                      'peak_MB': {k: round(v / 2 ** 20, 1) for k, v in peaks.items()}, 'record': records}), flush=True)


if __name__ == '__main__':
    main()
