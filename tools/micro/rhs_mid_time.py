"""Timing aid: the one-launch right-hand side for hidden widths 16..128 (csrc/rhs_mid.hip, ndcn_set_rhs_mid) against the composed path
(mode 0) in ONE process, the two alternating round by round: launch times of PLAIN and of COMBINE with 5 earlier stages, whole dopri5
solves (rtol 0.01, atol 0.001, two ticks), and a mode-2 sweep over n against the narrow-panel kernel (rhs_small.hip) to place the
crossover.  Prints one JSON line per measurement (median, min and max over the rounds, in ms) and, with --out FILE, writes them there too.

--dropout P times the dropout launches instead (ndcn_rhs_drop_f32 / ndcn_rhs_rk_drop_f32: plain, COMBINE with 0 and with 5 earlier stages,
RK4 stage 3) in mode 2 with ndcn_set_rhs_mid_drop off and on, alternating in the same way: off is the composed form (SpMM, MFMA Linear,
dropout_combine / dropout_apply + stage kernel) above 2^18 elements, on the factor in the one launch's epilogue.  The rows carry
"dropout": P and "drop_switch": 0 / 1.

    python tools/micro/rhs_mid_time.py [--rounds 7] [--iters 30] [--out profiles/NAME.jsonl] [--quick] [--dropout P]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import scipy.sparse as sp
import torch

from ndcn_amd import _lib, graphs, hip
from ndcn_amd import torchdiffeq as ode
from ndcn_amd.neural_dynamics import ODEFunc

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CS = [0.11, 0.07, 0.23, 0.05, -0.31, -0.19]


def lattice(side):
    return graphs.normalized_laplacian(graphs.grid_8_neighbor(side))


def pubmed():
    g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'operators_pubmed.npz')))
    return sp.csr_matrix((g['alpha00_data'], g['alpha00_indices'], g['alpha00_indptr']), shape=(int(g['n']), int(g['n'])))


def timed(fn, iters):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / iters


def alternate(fns, modes, rounds, iters, switch=None):
    """fns: name -> callable; per round every mode in turn, every callable inside it.  Returns {(name, mode): [ms per round]}, paths.
    switch: the setter the modes go to (default hip.set_rhs_mid)"""
    switch = switch or hip.set_rhs_mid
    out, paths = {}, {}
    for mode in modes:                                         # warm every shape in every mode
        prev = switch(mode)
        try:
            for name, fn in fns.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                paths[(name, mode)] = int(_lib.load().ndcn_debug_last_rhs_path())
        finally:
            switch(prev)
    for _ in range(rounds):
        for mode in modes:
            prev = switch(mode)
            try:
                for name, fn in fns.items():
                    out.setdefault((name, mode), []).append(timed(fn, iters))
            finally:
                switch(prev)
    return out, paths


def report(rows, what, graph, n, H, res, paths, sink, dropout=None):
    for (name, mode), ms in sorted(res.items()):
        row = {'what': what, 'launch': name, 'graph': graph, 'n': n, 'H': H, 'mode': mode, 'path': paths.get((name, mode)),
               'ms_median': round(statistics.median(ms), 5), 'ms_min': round(min(ms), 5), 'ms_max': round(max(ms), 5), 'rounds': len(ms)}
        if dropout is not None:                                # the modes alternated were the dropout switch's, inside mode 2
            row.update({'mode': 2, 'dropout': dropout, 'drop_switch': mode})
        rows.append(row)
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + '\n')
            sink.flush()


def launches(m, H, dev, dropout=None):
    A = graphs.to_device(m, dev)
    n = m.shape[0]
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand(n, H, generator=g, device=dev) - 0.3
    W = (torch.rand(H, H, generator=g, device=dev) - 0.5) / 8
    b = (torch.rand(H, generator=g, device=dev) - 0.5) / 8
    y0 = torch.randn(n, H, generator=g, device=dev)
    ks = [torch.randn(n, H, generator=g, device=dev) for _ in range(5)]
    K, yn = torch.empty_like(X), torch.empty_like(X)
    if dropout is not None:
        d = lambda e: (dropout, 1234567, e)
        return {'plain': lambda: hip.rhs(A, X, W, b, out=K, dropout=d(0)),
                'combine0': lambda: hip.rhs_rk(A, X, W, b, 'combine', y0, [], CS[5:], out_K=K, out_y=yn, dropout=d(1)),
                'combine5': lambda: hip.rhs_rk(A, X, W, b, 'combine', y0, ks, CS, out_K=K, out_y=yn, dropout=d(2)),
                'rk4_stage3': lambda: hip.rhs_rk(A, X, W, b, 'rk4', y0, ks[:3], [0.37], out_K=K, out_y=yn, dropout=d(3))}
    return {'plain': lambda: hip.rhs(A, X, W, b, out=K),
            'combine5': lambda: hip.rhs_rk(A, X, W, b, 'combine', y0, ks, CS, out_K=K, out_y=yn)}


def solve(m, H, dev):
    A = graphs.to_device(m, dev)
    torch.manual_seed(0)
    f = ODEFunc(H, A).to(dev)
    x0 = torch.rand(m.shape[0], H, generator=torch.Generator().manual_seed(1)).to(dev)
    t = torch.tensor([0., 1.]).to(dev)

    def run():
        with torch.no_grad():
            ode.odeint(f, x0, t, rtol=0.01, atol=0.001, method='dopri5')
    return {'dopri5_solve': run}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--iters', type=int, default=30)
    p.add_argument('--out', default=None)
    p.add_argument('--quick', action='store_true', help='one width and a 64 x 64 lattice: a rehearsal of every code path')
    p.add_argument('--dropout', type=float, default=None, metavar='P',
                   help='time the dropout launches with probability P: ndcn_set_rhs_mid_drop off against on, in mode 2')
    a = p.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the device'
    dev = torch.device('cuda:0')
    sink = open(a.out, 'w') if a.out else None
    rows = []
    side = 64 if a.quick else 316
    widths = (64,) if a.quick else (16, 20, 32, 64, 128)
    if a.dropout is not None:
        cases = [('lattice %d x %d' % (side, side), lattice(side), (64,) if a.quick else (16, 20, 32, 64, 96, 128))]
        if not a.quick:
            cases.append(('pubmed', pubmed(), (16, 64)))
        prev = hip.set_rhs_mid(2)
        try:
            for graph, m, hs in cases:
                for H in hs:
                    res, paths = alternate(launches(m, H, dev, a.dropout), (0, 1), a.rounds, a.iters, switch=hip.set_rhs_mid_drop)
                    report(rows, 'dropout launch', graph, m.shape[0], H, res, paths, sink, dropout=a.dropout)
        finally:
            hip.set_rhs_mid(prev)
        if sink:
            sink.close()
        return
    cases = [('lattice %d x %d' % (side, side), lattice(side), widths)]
    if not a.quick:
        cases.append(('pubmed', pubmed(), (64,)))
    for graph, m, hs in cases:
        for H in hs:
            res, paths = alternate(launches(m, H, dev), (0, 1), a.rounds, a.iters)
            report(rows, 'launch', graph, m.shape[0], H, res, paths, sink)
            res, paths = alternate(solve(m, H, dev), (0, 1), a.rounds, max(1, a.iters // 10))
            report(rows, 'solve', graph, m.shape[0], H, res, paths, sink)
    # the crossover against the narrow-panel kernel: mode 0 below n H = 2^18 is rhs_small.hip, mode 2 this kernel
    for H in ((64,) if a.quick else (20, 64, 128)):
        for n_side in ((16, 32) if a.quick else (16, 23, 32, 45, 64, 90)):
            if n_side * n_side * H > 1 << 18:
                continue
            m = lattice(n_side)
            res, paths = alternate(launches(m, H, dev), (0, 2), a.rounds, a.iters)
            report(rows, 'crossover', 'lattice %d x %d' % (n_side, n_side), m.shape[0], H, res, paths, sink)
    if sink:
        sink.close()


if __name__ == '__main__':
    main()
