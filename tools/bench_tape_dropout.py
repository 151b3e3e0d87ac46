#!/usr/bin/env python3
"""What the dopri5 training tape is worth under an active dropout (measurement aid, not the judged bench line).

epochs   one training epoch of tools/bench_dgnn.py's model (--dgnn-defaults --dropout P [--hidden H --no-control]) with
         NDCN_TAPE_DROPOUT unset (the per-operation graph) and = 1 (ndcn_tape_dopri5_drop_f32), alternating in one process on one
         model; the median of --reps timed epochs after --warmup untimed ones per form (train part and eval part as bench_dgnn
         splits them).
kernel   ndcn_dropout_combine_f32 against ndcn_dropout_apply_f32 + ndcn_rk_combine_f32 at --rows x --hidden with --n-prev earlier
         stages, and a device-to-device copy of one panel on the same lease: microseconds (device events, median of --reps after
         --warmup) and the fraction of the copy's bytes per second each form reaches on the bytes it has to move.
Prints one JSON line per part."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch


def epochs(a, dev):
    import bench_dgnn as bd
    bd.HID, bd.T_END, bd.TICKS, bd.WD, bd.NO_CONTROL = 16, 2.0, 5, 5e-4, False
    if a.hidden is not None:
        bd.HID = a.hidden
    bd.NO_CONTROL = bool(a.no_control)
    bd.DROPOUT = a.dropout
    case = bd.load_case('cora')
    model, opt, x, y, itr, iva = bd.build_hip(case, dev)
    forms = {'per_operation': None, 'tape': '1'}
    tr = {k: [] for k in forms}
    ev = {k: [] for k in forms}
    nodes = {}
    for r in range(a.warmup + a.reps):
        for name, value in forms.items():
            os.environ.pop('NDCN_TAPE_DROPOUT', None)
            if value is not None:
                os.environ['NDCN_TAPE_DROPOUT'] = value
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, _, t1 = bd.epoch_hip(model, opt, x, y, itr, iva)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if r >= a.warmup:
                tr[name].append(t1 - t0)
                ev[name].append(t2 - t1)
    os.environ.pop('NDCN_TAPE_DROPOUT', None)
    med = {k: 1e3 * float(np.median(v)) for k, v in tr.items()}
    print(json.dumps({'part': 'epochs', 'case': 'dgnn differential_gcn, cora', 'hidden': bd.HID, 'no_control': bd.NO_CONTROL,
                      'dropout': a.dropout, 'reps': a.reps, 'warmup': a.warmup, 'train_ms_per_operation': round(med['per_operation'], 3),
                      'train_ms_tape': round(med['tape'], 3), 'tape_over_per_operation': round(med['tape'] / med['per_operation'], 3),
                      'eval_ms': {k: round(1e3 * float(np.median(v)), 3) for k, v in ev.items()},
                      'all_train_ms': {k: [round(1e3 * s, 3) for s in v] for k, v in tr.items()}}), flush=True)


def kernel(a, dev):
    from ndcn_amd import hip
    n, H, m = a.rows, a.hidden or 256, a.n_prev
    g = torch.Generator().manual_seed(0)
    K0 = torch.rand(n, H, generator=g).to(dev)
    K, y0, out, dst = torch.empty_like(K0), torch.rand(n, H, generator=g).to(dev), torch.empty_like(K0), torch.empty_like(K0)
    ks = [torch.rand(n, H, generator=g).to(dev) for _ in range(m)]
    cs = [0.1 * (j + 1) for j in range(m + 1)]
    desc = (0.5, 7, 3)
    forms = {'copy': lambda: dst.copy_(K0), 'one_pass': lambda: hip.dropout_combine(K, desc, ks, cs, y0=y0, out=out),
             'apply_then_combine': lambda: (hip.dropout_apply(K, desc), hip.combine(y0, ks + [K], cs))}
    us = {k: [] for k in forms}
    for r in range(a.warmup + a.reps):
        for name, fn in forms.items():
            K.copy_(K0)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                us[name].append(1e3 * e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in us.items()}
    panel = 4.0 * n * H
    moved = {'copy': 2 * panel, 'one_pass': (m + 2 + 2) * panel, 'apply_then_combine': (2 + m + 2 + 1) * panel}
    rate = {k: moved[k] / (med[k] * 1e-6) for k in forms}
    print(json.dumps({'part': 'kernel', 'rows': n, 'hidden': H, 'n_prev': m, 'reps': a.reps, 'warmup': a.warmup,
                      'us': {k: round(v, 2) for k, v in med.items()}, 'panels_moved': {k: moved[k] / panel for k in forms},
                      'TB_per_s': {k: round(v / 1e12, 3) for k, v in rate.items()},
                      'fraction_of_copy_rate': {k: round(rate[k] / rate['copy'], 3) for k in forms},
                      'one_pass_over_two_kernels': round(med['one_pass'] / med['apply_then_combine'], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('part', choices=['epochs', 'kernel'])
    ap.add_argument('--dropout', type=float, default=0.5)
    ap.add_argument('--hidden', type=int, default=None)
    ap.add_argument('--no-control', action='store_true')
    ap.add_argument('--rows', type=int, default=100000)
    ap.add_argument('--n-prev', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    (epochs if a.part == 'epochs' else kernel)(a, dev)


if __name__ == '__main__':
    main()
