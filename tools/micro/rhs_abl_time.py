"""Timing aid: the one-launch right-hand side of the no_control / no_graph ablations (csrc/rhs_abl.hip, ndcn_set_rhs_abl) against the
composed path (switch off: SpMM or MFMA Linear, mask pass, stand-alone stage kernel) in ONE process, the two alternating round by round:
launch times of PLAIN, COMBINE with 5 earlier stages and RK4 stage 3, with p = 0 and with --dropout P, and whole-run figures - one Adam
step of NDCN(1, 20, no_control / no_graph) through dopri5 on both lattices and the train part of one dgnn --no_control --hidden 16 epoch
on the Pubmed topology.  Prints one JSON line per measurement (median, min and max over the rounds, in ms; "mode": the switch, 0 / 1;
"what" names the form and p) and, with --out FILE, writes them there too.

    python tools/micro/rhs_abl_time.py [--rounds 7] [--iters 30] [--dropout 0.5] [--out profiles/NAME.jsonl] [--quick]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import rhs_mid_time as M
from ndcn_amd import graphs, hip
from ndcn_amd.neural_dynamics import NDCN, ODEBlock2, ODEFunc

CS = M.CS


def launches(m, H, dev, form, dropout=None):
    n = m.shape[0]
    A = graphs.to_device(m, dev) if form == 'no_control' else None
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand(n, H, generator=g, device=dev) - 0.3
    W = b = None
    if form == 'no_graph':
        W = (torch.rand(H, H, generator=g, device=dev) - 0.5) / 8
        b = (torch.rand(H, generator=g, device=dev) - 0.5) / 8
    y0 = torch.randn(n, H, generator=g, device=dev)
    ks = [torch.randn(n, H, generator=g, device=dev) for _ in range(5)]
    K, yn = torch.empty_like(X), torch.empty_like(X)
    kw = {form: True}
    d = (lambda e: {}) if dropout is None else (lambda e: {'dropout': (dropout, 1234567, e)})
    return {'plain': lambda: hip.rhs(A, X, W, b, out=K, **kw, **d(0)),
            'combine5': lambda: hip.rhs_rk(A, X, W, b, 'combine', y0, ks, CS, out_K=K, out_y=yn, **kw, **d(1)),
            'rk4_stage3': lambda: hip.rhs_rk(A, X, W, b, 'rk4', y0, ks[:3], [0.37], out_K=K, out_y=yn, **kw, **d(2))}


def adam_step(side, dev, form):
    """one Adam step of the drivers' loop (heat_dynamics.py:313-334) at --hidden 20 through dopri5"""
    L = graphs.normalized_laplacian(graphs.grid_8_neighbor(side))
    n = side * side
    torch.manual_seed(0)
    model = NDCN(1, 20, graphs.to_device(L, dev), 1, rtol=.01, atol=.001, method='dopri5', **{form: True}).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    x0 = torch.from_numpy(graphs.x0_blocks(side)[:n]).to(dev)
    t = torch.linspace(0., 5., 12).to(dev)
    target = torch.rand(n, 12, generator=torch.Generator().manual_seed(1)).to(dev)

    def run():
        opt.zero_grad()
        loss = torch.nn.functional.l1_loss(model(t, x0).squeeze().t(), target)
        loss.backward()
        opt.step()
    return {'adam_step_dopri5': run}


def dgnn_train(dev):
    """the train part of one dgnn.py --no_control --hidden 16 epoch on the Pubmed topology (dgnn.py:192-206): encoder, ODEBlock2 over
    relu(A x) by dopri5 to its terminal time, decoder, NLL loss on the training rows, Adam"""
    m = M.pubmed()
    n = m.shape[0]
    A = graphs.to_device(m, dev)
    torch.manual_seed(0)
    H, C, Fin = 16, 3, 500
    vt = torch.tensor([0., 1.2]).to(dev)
    model = torch.nn.Sequential(torch.nn.Linear(Fin, H), torch.nn.Tanh(),
                                ODEBlock2(ODEFunc(H, A, dropout=0.0, no_control=True), vt, rtol=.1, atol=.1, method='dopri5', terminal=True),
                                torch.nn.Linear(H, C), torch.nn.LogSoftmax(dim=1)).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=0.024)
    x = torch.rand(n, Fin, generator=torch.Generator().manual_seed(1)).to(dev)
    labels = torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(2)).to(dev)
    idx = torch.arange(60, device=dev)

    def run():
        opt.zero_grad()
        loss = torch.nn.functional.nll_loss(model(x)[idx], labels[idx])
        loss.backward()
        opt.step()
    return {'dgnn_train_epoch': run}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--iters', type=int, default=30)
    p.add_argument('--out', default=None)
    p.add_argument('--dropout', type=float, default=0.5, metavar='P', help='the probability of the dropout launches')
    p.add_argument('--quick', action='store_true', help='one width and a 64 x 64 lattice: a rehearsal of every code path')
    a = p.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the device'
    dev = torch.device('cuda:0')
    sink = open(a.out, 'w') if a.out else None
    rows = []
    sides = (20, 64) if a.quick else (20, 316)
    widths = (20,) if a.quick else (16, 20, 64, 96, 128)
    cases = [('lattice %d x %d' % (s, s), M.lattice(s), widths) for s in sides]
    if not a.quick:
        cases.append(('pubmed', M.pubmed(), (16,)))
    for graph, m, hs in cases:
        for H in hs:
            for form in ('no_control', 'no_graph'):
                for drop in (None, a.dropout):
                    res, paths = M.alternate(launches(m, H, dev, form, drop), (0, 1), a.rounds, a.iters, switch=hip.set_rhs_abl)
                    M.report(rows, 'launch %s p=%g' % (form, drop or 0.0), graph, m.shape[0], H, res, paths, sink)
    whole = [('lattice %d x %d' % (s, s), s * s, 20, adam_step(s, dev, form), form) for s in sides for form in ('no_control', 'no_graph')]
    if not a.quick:
        whole.append(('pubmed', 19717, 16, dgnn_train(dev), 'no_control'))
    for graph, n, H, fns, form in whole:
        res, paths = M.alternate(fns, (0, 1), a.rounds, max(1, a.iters // 10), switch=hip.set_rhs_abl)
        M.report(rows, 'whole run %s' % form, graph, n, H, res, paths, sink)
    if sink:
        sink.close()


if __name__ == '__main__':
    main()
