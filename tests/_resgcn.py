"""The static-GCN modules of ndcn_amd (ode_gcn.ResBlock, models.GCN, the resGCN Sequential of drivers/dgnn.py) restated on the CPU in
float64 torch autograd with a dense operator, from the formulas of those files:

    rownorm(x)   x / max(row L1 norm, float32(1e-12)), infinities zeroed
    block        x + relu([rownorm]([W (.) + b](A [rownorm] x) * mask)) * time_step       (the mask after the Linear, where
                                                                                            ResBlock.forward applies its dropout)
    gcn layer    A (x W^T + b);  GCN: relu(gc1) -> relu(conv_middle[i]) ... -> gc2
    resGCN       Linear -> ReLU -> blocks -> Linear

Every function takes an optional `pre` list and appends each ReLU pre-activation to it (what the tests' input conditions are about),
and `norms` for the L1 norms of the rows that are normalised."""
import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

EPS = float(np.float32(1e-12))


def rownorm(x, norms=None):
    if norms is not None:
        norms.append(x.detach().abs().sum(1))
    y = F.normalize(x, 1, 1, eps=EPS)
    return y.masked_fill(torch.isinf(y), 0.0)


def block(A, x, W=None, b=None, time_step=1.0, normalize=False, mask=None, pre=None, norms=None):
    shortcut = x
    if normalize:
        x = rownorm(x, norms)
    f = A @ x
    if W is not None:
        f = f @ W.t() + b
    if mask is not None:
        f = f * mask
    if normalize:
        f = rownorm(f, norms)
    if pre is not None:
        pre.append(f.detach())
    return shortcut + torch.relu(f) * time_step


def gcn_layer(A, x, W, b):
    return A @ (x @ W.t() + b)


def gcn(A, x, p, n_middle, pre=None):
    """p: parameters by the state_dict keys of models.GCN"""
    layers = ['gc1'] + ['conv_middle.%d' % i for i in range(n_middle)]
    for name in layers:
        z = gcn_layer(A, x, p[name + '.fc.weight'], p[name + '.fc.bias'])
        if pre is not None:
            pre.append(z.detach())
        x = torch.relu(z)
    return gcn_layer(A, x, p['gc2.fc.weight'], p['gc2.fc.bias'])


def resgcn(A, x, p, n_blocks, normalize=False, pre=None, norms=None):
    """p: parameters by the state_dict keys of the Sequential (0.weight, 0.bias, 2.time_step, ..)"""
    z = x @ p['0.weight'].t() + p['0.bias']
    if pre is not None:
        pre.append(z.detach())
    x = torch.relu(z)
    for i in range(n_blocks):
        ts = p.get('%d.time_step' % (2 + i), 1.0)
        x = block(A, x, time_step=ts, normalize=normalize, pre=pre, norms=norms)
    k = 2 + n_blocks
    return x @ p['%d.weight' % k].t() + p['%d.bias' % k]


def clear_of_the_kink(pre):
    """a property of the INPUTS: in the float64 run no ReLU pre-activation other than an exact zero lies within 1e-6 of zero, where the
    float32 and the float64 mask may differ"""
    a = torch.cat([z.reshape(-1) for z in pre]).abs()
    return bool(((a == 0) | (a > 1e-6)).all())


def clear_of_the_clamp(norms):
    """no normalised row's L1 norm within a factor 2 of the clamp at 1e-12"""
    s = torch.cat([n.reshape(-1) for n in norms]) if norms else torch.zeros(0)
    return bool(((s < 0.5e-12) | (s > 2e-12)).all())


def graph(n=300, seed=0, alone=17):
    """the power-law graph of the drivers with dgnn's operator (alpha = 0.5) as sorted CSR, node `alone` cut off by hand: an empty row
    and an empty column"""
    from ndcn_amd import graphs
    m = graphs.zipf_smoothing_alpha(graphs.make_graph('power_law', n, seed=seed), 0.5).tolil()
    m[alone, :] = 0
    m[:, alone] = 0
    m = sp.csr_matrix(m.tocsr(), dtype=np.float32)
    m.eliminate_zeros()
    m.sort_indices()
    assert m.indptr[alone] == m.indptr[alone + 1]
    return m
