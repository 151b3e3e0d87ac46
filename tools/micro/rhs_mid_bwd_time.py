"""Timing aid: the one-launch reverse of the right-hand side for hidden widths 16..128 (csrc/rhs_mid_bwd.hip, ndcn_set_rhs_mid_bwd) against
the composed launches (mode 0) in ONE process, the two alternating round by round: ndcn_rhs_vjp_f32 with the S panel re-formed and with
it supplied, and one Adam step of NDCN(1, H) through rk4 and through dopri5.  Prints one JSON line per measurement (median, min and max
over the rounds, in ms) and, with --out FILE, writes them there too.

    python tools/micro/rhs_mid_bwd_time.py [--rounds 7] [--iters 30] [--out profiles/NAME.jsonl] [--quick]"""
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
from ndcn_amd.neural_dynamics import NDCN

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def alternate(fns, modes, rounds, iters):
    """fns: name -> callable; per round every mode in turn, every callable inside it.  Returns {(name, mode): [ms per round]}, routes"""
    out, routes = {}, {}
    for mode in modes:                                         # warm every shape in every mode
        prev = hip.set_rhs_mid_bwd(mode)
        try:
            for name, fn in fns.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                routes[(name, mode)] = int(_lib.load().ndcn_debug_last_rhs_vjp_path())
        finally:
            hip.set_rhs_mid_bwd(prev)
    for _ in range(rounds):
        for mode in modes:
            prev = hip.set_rhs_mid_bwd(mode)
            try:
                for name, fn in fns.items():
                    out.setdefault((name, mode), []).append(timed(fn, iters))
            finally:
                hip.set_rhs_mid_bwd(prev)
    return out, routes


def report(what, graph, n, H, res, routes, sink):
    for (name, mode), ms in sorted(res.items()):
        row = {'what': what, 'call': name, 'graph': graph, 'n': n, 'H': H, 'mode': mode, 'route': routes.get((name, mode)),
               'ms_median': round(statistics.median(ms), 5), 'ms_min': round(min(ms), 5), 'ms_max': round(max(ms), 5), 'rounds': len(ms)}
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + '\n')
            sink.flush()


def calls(m, H, dev):
    """ndcn_rhs_vjp_f32 as a reverse pass issues it: gX wanted, gW / gb accumulated"""
    A = graphs.to_device(m, dev)
    n = m.shape[0]
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand(n, H, generator=g, device=dev) - 0.3
    W = (torch.rand(H, H, generator=g, device=dev) - 0.5) / 8
    b = (torch.rand(H, generator=g, device=dev) - 0.5) / 8
    K = hip.rhs(A, X, W, b)
    S = hip.spmm(A, X)
    up = torch.randn(n, H, generator=g, device=dev)
    gW, gb = torch.zeros(H, H, device=dev), torch.zeros(H, device=dev)
    return {'vjp, S re-formed': lambda: hip.rhs_vjp(A, X, W, K, up, gW=gW, gb=gb),
            'vjp, S supplied': lambda: hip.rhs_vjp(A, X, W, K, up, S=S, gW=gW, gb=gb)}


def adam_steps(m, H, dev):
    """one optimizer step of the reference's model (input 1, hidden H, output 1) through each solver: forward, loss, backward, Adam"""
    A = graphs.to_device(m, dev)
    n = m.shape[0]
    x0 = torch.rand(n, 1, generator=torch.Generator().manual_seed(1)).to(dev)
    target = torch.rand(5, n, 1, generator=torch.Generator().manual_seed(2)).to(dev)
    t = torch.linspace(0., 1., 5).to(dev)
    fns = {}
    for method in ('rk4', 'dopri5'):
        torch.manual_seed(0)
        model = NDCN(1, H, A, 1, rtol=0.01, atol=0.001, method=method).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)

        def run(model=model, opt=opt):
            opt.zero_grad()
            loss = (model(t, x0) - target).abs().mean()
            loss.backward()
            opt.step()
        fns['adam step, %s' % method] = run
    return fns


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--iters', type=int, default=30)
    p.add_argument('--out', default=None)
    p.add_argument('--quick', action='store_true', help='one width and a 64 x 64 lattice: a rehearsal of every code path')
    a = p.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the device'
    dev = torch.device('cuda:0')
    sink = open(a.out, 'w') if a.out else None
    side = 64 if a.quick else 316
    widths = (64,) if a.quick else (16, 20, 32, 64, 96, 128)
    cases = [('lattice %d x %d' % (side, side), lattice(side), widths)]
    if not a.quick:
        cases.append(('pubmed', pubmed(), (64,)))
    for graph, m, hs in cases:
        for H in hs:
            res, routes = alternate(calls(m, H, dev), (0, 2), a.rounds, a.iters)
            report('call', graph, m.shape[0], H, res, routes, sink)
    for H in ((64,) if a.quick else (20, 64)):
        m = lattice(side)
        res, routes = alternate(adam_steps(m, H, dev), (0, 2), a.rounds, max(1, a.iters // 10))
        report('train', 'lattice %d x %d' % (side, side), m.shape[0], H, res, routes, sink)
    if sink:
        sink.close()


if __name__ == '__main__':
    main()
