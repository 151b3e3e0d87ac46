"""The ground-truth dynamics of the reference's three experiment drivers as modules: the reference's constructor signatures and
attribute names (heat_dynamics.py:186-204, gene_dynamics.py:186-205, mutualistic_dynamics.py:186-216), evaluated by the O(nnz) HIP
kernels on an N x 1 state.

`forward(t, x)` is the stand-alone operation of `ndcn_amd.hip` (applied to each tensor where odeint hands over a tuple state), so
every path that calls the module back - tuple states, decreasing `t`, `adams`, anything that needs a gradient - computes what a
closure over that operation computes.  `odeint` recognises exactly
these three classes (not subclasses: a subclass may override `forward`) and runs a float32 (N, 1) solve without a gradient inside
the device solver, whose right-hand-side launches carry the Runge-Kutta algebra in their epilogue (ndcn_dyn_rk_f32): the same
trajectory bit for bit, without a Python callback per evaluation.

The operator may be anything `as_csr` converts (a CsrOperator, a dense or sparse torch tensor).  One deviation from the reference's
attributes: HeatDiffusion keeps `L` as it was given - the reference stores `-L` - and puts the sign into the product's alpha.
"""
import torch.nn as nn

from . import _lib
from .ops import hip


def _each(op, x):
    """op(x), or (op(x_0), ...) for the tuple a tuple-state solve passes (misc.py:175-182)"""
    return tuple(op(x_) for x_ in x) if isinstance(x, tuple) else op(x)


class HeatDiffusion(nn.Module):
    """dX/dt = -k L X  (heat_dynamics.py:186-204)"""
    ndcn_autonomous = True

    def __init__(self, L, k=1):
        super().__init__()
        self.L = L
        self.k = k

    def forward(self, t, x):
        return _each(lambda x_: hip.spmm(self.L, x_, alpha=-float(self.k)), x)

    def ndcn_dynamics(self):
        """(operator, NDCN_DYN_* kind, scalar parameters in the order of struct ndcn_dynamics)"""
        return self.L, _lib.DYN_HEAT, (float(self.k),)


class GeneDynamics(nn.Module):
    """dx_i/dt = -b x_i^f + sum_j A_ij x_j^h / (x_j^h + 1)  (gene_dynamics.py:186-205)"""
    ndcn_autonomous = True

    def __init__(self, A, b, f=1, h=2):
        super().__init__()
        self.A = A
        self.b = b
        self.f = f
        self.h = h

    def forward(self, t, x):
        return _each(lambda x_: hip.gene_rhs(self.A, x_, b=self.b, f=self.f, h=self.h), x)

    def ndcn_dynamics(self):
        return self.A, _lib.DYN_GENE, (float(self.b), float(self.f), float(self.h))


class MutualDynamics(nn.Module):
    """dx_i/dt = b + x_i (1 - x_i / k) (x_i / c - 1) + sum_j A_ij x_i x_j / (d + e x_j + h x_i): the branch of
    mutualistic_dynamics.py:206-216 that executes for an N x 1 state, e and h as executed"""
    ndcn_autonomous = True

    def __init__(self, A, b=0.1, k=5., c=1., d=5., e=0.9, h=0.1):
        super().__init__()
        self.A = A
        self.b = b
        self.k = k
        self.c = c
        self.d = d
        self.e = e
        self.h = h

    def forward(self, t, x):
        return _each(lambda x_: hip.mutual_rhs(self.A, x_, b=self.b, k=self.k, c=self.c, d=self.d, e=self.e, h=self.h), x)

    def ndcn_dynamics(self):
        return self.A, _lib.DYN_MUTUAL, tuple(float(v) for v in (self.b, self.k, self.c, self.d, self.e, self.h))


TRUTH_CLASSES = (HeatDiffusion, GeneDynamics, MutualDynamics)

__all__ = ['HeatDiffusion', 'GeneDynamics', 'MutualDynamics']
