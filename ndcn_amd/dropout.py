"""The dropout stream of the fused right-hand side: which (seed, evaluation) every evaluation of ODEFunc gets.

The mask itself is a pure function of (p, seed, evaluation, element index) computed inside the kernels (csrc/dropout.h).  This
module owns the two numbers that vary:
  seed        64 bits drawn from torch's default (CPU) generator - `torch.manual_seed` makes a training run repeatable - ONCE per
              `odeint` call, at the first evaluation that asks (a solve without an active dropout draws nothing and leaves the
              generator where it was), or per direct `ODEFunc.forward` call outside a solve;
  evaluation  the number of the evaluation inside that solve, from 0, in the order the solver makes them.
No two evaluations share (seed, evaluation).  A path that runs several evaluations per launch sequence (the fixed-grid training
path) takes a block of counters with `Stream.take(n)` and re-forms the same stages with the same counters in its reverse pass.
"""
import threading

import numpy as np
import torch


def scale(p):
    """s = 1.0f / (1.0f - float32(p)): what a kept element is multiplied by"""
    one = np.float32(1.0)
    return float(one / (one - np.float32(p)))


def is_active(module):
    """the module's dropout takes the fused form: training mode and 0 < p < 1 (p >= 1 keeps the un-fused branch)"""
    return bool(module.training) and 0.0 < float(np.float32(module.dropout)) < 1.0


def draw_seed():
    words = torch.randint(0, 2 ** 32, (2,), dtype=torch.int64)           # the default CPU generator
    return (int(words[0]) << 32) | int(words[1])


class Stream:
    """seed (drawn when first read) and evaluation counter of one solve"""

    def __init__(self):
        self._seed = None
        self.evaluations = 0

    @property
    def seed(self):
        if self._seed is None:
            self._seed = draw_seed()
        return self._seed

    def take(self, n=1):
        """the first of n consecutive evaluation numbers"""
        first = self.evaluations
        self.evaluations += n
        return first


_local = threading.local()


def _stack():
    st = getattr(_local, 'stack', None)
    if st is None:
        st = _local.stack = []
    return st


class solve_scope:
    """`with solve_scope():` brackets one solve (odeint does): evaluations inside it number from 0 under one seed"""

    def __enter__(self):
        self.stream = Stream()
        _stack().append(self.stream)
        return self.stream

    def __exit__(self, *exc):
        _stack().pop()
        return False


def current():
    """the stream of the innermost solve of this thread, or None outside any"""
    st = _stack()
    return st[-1] if st else None


def next_evaluation(p):
    """(p, seed, evaluation) for the next evaluation: of the current solve, or - outside a solve - of a one-evaluation stream"""
    stream = current() or Stream()
    return (float(p), stream.seed, stream.take())
