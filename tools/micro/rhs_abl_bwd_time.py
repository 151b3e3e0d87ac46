"""Timing aid: the one-launch reverse of the no_control / no_graph ablations (csrc/rhs_abl_bwd.hip, ndcn_set_rhs_abl_bwd) against the
composed launches (switch off: relu_bwd + transposed SpMM, or linear_bwd's three launches + the scaling pass) in ONE process, the two
alternating round by round: one ndcn_rhs_vjp_f32 call per form with alpha 1 and 2, and whole Adam steps - NDCN(1, 20, no_control /
no_graph) through dopri5 and through rk4 with dropout 0.5, and the train part of one dgnn --no_control --hidden 16 epoch on the Pubmed
topology - with the forward switch (ndcn_set_rhs_abl) on in both arms.  Prints one JSON line per measurement (median, min and max over
the rounds, in ms; "mode": the switch, 0 / 1; "route": ndcn_debug_last_rhs_vjp_path after the warm-up) and, with --out FILE, writes them
there too.

    python tools/micro/rhs_abl_bwd_time.py [--rounds 7] [--iters 30] [--out profiles/NAME.jsonl] [--quick]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import rhs_abl_time as F
import rhs_mid_bwd_time as B
from ndcn_amd import _lib, graphs, hip
from ndcn_amd.neural_dynamics import NDCN


def alternate(fns, rounds, iters):
    """fns: name -> callable; per round the switch off then on, every callable inside it.  Returns {(name, mode): [ms per round]}, routes"""
    out, routes = {}, {}
    for mode in (0, 1):                                        # warm every shape in both arms
        prev = hip.set_rhs_abl_bwd(mode)
        try:
            for name, fn in fns.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                routes[(name, mode)] = int(_lib.load().ndcn_debug_last_rhs_vjp_path())
        finally:
            hip.set_rhs_abl_bwd(prev)
    for _ in range(rounds):
        for mode in (0, 1):
            prev = hip.set_rhs_abl_bwd(mode)
            try:
                for name, fn in fns.items():
                    out.setdefault((name, mode), []).append(B.timed(fn, iters))
            finally:
                hip.set_rhs_abl_bwd(prev)
    return out, routes


def calls(m, H, dev, form):
    """ndcn_rhs_vjp_f32 as a reverse pass issues it: gX wanted, gW / gb accumulated; alpha = acc_scale 1 and 2 (2: dropout's s at p = 0.5)"""
    n = m.shape[0]
    A = graphs.to_device(m, dev) if form == 'no_control' else None
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand(n, H, generator=g, device=dev) - 0.3
    W = b = gW = gb = None
    if form == 'no_graph':
        W = (torch.rand(H, H, generator=g, device=dev) - 0.5) / 8
        b = (torch.rand(H, generator=g, device=dev) - 0.5) / 8
        gW, gb = torch.zeros(H, H, device=dev), torch.zeros(H, device=dev)
    K = hip.rhs(A, X, W, b, **{form: True})
    up = torch.randn(n, H, generator=g, device=dev)
    return {'vjp %s alpha=%g' % (form, s): (lambda s=s: hip.rhs_vjp(A, X, W, K, up, gW=gW, gb=gb, acc_scale=s, **{form: True}))
            for s in (1.0, 2.0)}


def adam_step_rk4(side, dev, form):
    """one Adam step of NDCN(1, 20) through rk4 with dropout 0.5: the fixed-grid sweep, every reverse evaluation masked and scaled"""
    L = graphs.normalized_laplacian(graphs.grid_8_neighbor(side))
    n = side * side
    torch.manual_seed(0)
    model = NDCN(1, 20, graphs.to_device(L, dev), 1, dropout=0.5, method='rk4', **{form: True}).to(dev)
    model.train(True)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    x0 = torch.from_numpy(graphs.x0_blocks(side)[:n]).to(dev)
    t = torch.linspace(0., 5., 12).to(dev)
    target = torch.rand(n, 12, generator=torch.Generator().manual_seed(1)).to(dev)

    def run():
        opt.zero_grad()
        loss = torch.nn.functional.l1_loss(model(t, x0).squeeze().t(), target)
        loss.backward()
        opt.step()
    return {'adam_step_rk4_p0.5': run}


def report(what, graph, n, H, res, routes, sink):
    for (name, mode), ms in sorted(res.items()):
        row = {'what': what, 'call': name, 'graph': graph, 'n': n, 'H': H, 'mode': mode, 'route': routes.get((name, mode)),
               'ms_median': round(statistics.median(ms), 5), 'ms_min': round(min(ms), 5), 'ms_max': round(max(ms), 5), 'rounds': len(ms)}
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + '\n')
            sink.flush()


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
    widths = (20,) if a.quick else (16, 20, 32, 64, 96, 128)
    cases = [('lattice %d x %d' % (side, side), B.lattice(side), widths)]
    if not a.quick:
        cases.append(('pubmed', B.pubmed(), (16,)))
    for graph, m, hs in cases:
        for H in hs:
            for form in ('no_control', 'no_graph'):
                res, routes = alternate(calls(m, H, dev, form), a.rounds, a.iters)
                report('call', graph, m.shape[0], H, res, routes, sink)
    fwd = hip.set_rhs_abl(1)                                   # the forward launches fused in both arms
    try:
        whole = []
        for form in ('no_control', 'no_graph'):
            fns = dict(F.adam_step(side, dev, form))
            fns.update(adam_step_rk4(side, dev, form))
            whole.append(('lattice %d x %d' % (side, side), side * side, 20, fns, form))
        if not a.quick:
            whole.append(('pubmed', 19717, 16, F.dgnn_train(dev), 'no_control'))
        for graph, n, H, fns, form in whole:
            res, routes = alternate(fns, a.rounds, max(1, a.iters // 10))
            report('whole run %s' % form, graph, n, H, res, routes, sink)
    finally:
        hip.set_rhs_abl(fwd)
    if sink:
        sink.close()


if __name__ == '__main__':
    main()
