"""The dropout form of the dopri5 training tape, host side (no GPU): the entry points are declared and bound alike, the numbering of a
solve's evaluations (ndcn_tape_attempt_evaluation: a pure function - f0, the initial step's f1 when it is evaluated, six per
attempted step) on hand-made sequences, and the routing decision of `_odeint` with NDCN_TAPE_DROPOUT set and unset."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()


def _prototype_args(name):
    m = re.search(r'NDCN_API[^;(]*?\b%s\s*\(([^;]*?)\)\s*;' % name, _header(), re.S)
    assert m, name + ' is not declared'
    return [a.strip() for a in m.group(1).split(',')]


def test_entry_points_are_declared_and_bound_with_the_same_argument_counts():
    import ctypes
    from ndcn_amd import _lib
    for name in ('ndcn_tape_dopri5_drop_f32', 'ndcn_tape_attempt_evaluation', 'ndcn_tape_evaluations', 'ndcn_dropout_combine_f32'):
        assert name in _lib.SIGNATURES
        assert len(_prototype_args(name)) == len(_lib.SIGNATURES[name][1]), name
    # the argument list of ndcn_tape_dopri5_budget_f32 plus the descriptor
    budget, drop = _prototype_args('ndcn_tape_dopri5_budget_f32'), _prototype_args('ndcn_tape_dopri5_drop_f32')
    assert drop[:-1] == budget and drop[-1] == 'const ndcn_dropout *desc'
    assert _lib.SIGNATURES['ndcn_tape_dopri5_drop_f32'][1][:-1] == _lib.SIGNATURES['ndcn_tape_dopri5_budget_f32'][1]
    assert _lib.SIGNATURES['ndcn_tape_dopri5_drop_f32'][1][-1] is ctypes.POINTER(_lib.DropoutDesc)
    version = int(re.search(r'#define NDCN_ABI_VERSION (\d+)', _header()).group(1))
    assert version == _lib.ABI_VERSION >= 29


def _numbers(lib, first, probe, accepted, thin_from=None):
    """the forward pass's numbering over a sequence of attempts (accepted[i]: 1 / 0) -> (the six numbers of every attempt, numbers
    consumed); thin_from: attempts from this index on are thin - what the reverse pass re-forms them with is asked a second time"""
    out = []
    for i, _ in enumerate(accepted):
        e = lib.ndcn_tape_attempt_evaluation(first, probe, i)
        out.append(list(range(e, e + 6)))
    consumed = lib.ndcn_tape_attempt_evaluation(first, probe, len(accepted)) - first
    if thin_from is not None:
        for i in range(thin_from, len(accepted)):                 # a re-formed attempt runs with exactly its forward numbers ...
            e = lib.ndcn_tape_attempt_evaluation(first, probe, i)
            assert list(range(e, e + 6)) == out[i]
        assert lib.ndcn_tape_attempt_evaluation(first, probe, len(accepted)) - first == consumed      # ... and consumes none
    return out, consumed


def test_evaluation_numbering():
    from ndcn_amd import _lib
    lib = _lib.load()
    # with the initial-step probe: f0 = first, f1 = first + 1, the first attempt starts at first + 2
    seq, used = _numbers(lib, 0, 1, [1, 1, 1])
    assert seq == [[2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13], [14, 15, 16, 17, 18, 19]] and used == 20
    # first_step given: no f1
    seq, used = _numbers(lib, 0, 0, [1, 1])
    assert seq == [[1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11, 12]] and used == 13
    # a rejected attempt consumes its six like an accepted one (every evaluation of the solve has another mask)
    a, ua = _numbers(lib, 0, 1, [1, 0, 0, 1])
    b, ub = _numbers(lib, 0, 1, [1, 1, 1, 1])
    assert a == b and ua == ub == 26
    # the count autograd_path.integrate_dopri5_grad reports as nfe is the same number: 2 + 6 per attempt
    assert ua == 2 + 6 * 4
    # a solve that is not the first user of its stream starts where the stream stands
    seq, used = _numbers(lib, 100, 1, [0, 1])
    assert seq[0][0] == 102 and seq[1][-1] == 113 and used == 14
    # budget: thin attempts (ndcn_tape_attempt_is_full says which) keep their numbers; re-forming them consumes none
    pb = 1000
    full_panels, thin, kinds = 0, 0, []
    for _ in range(5):
        full = lib.ndcn_tape_attempt_is_full(24 * pb, full_panels, pb, 0, thin)            # (with dropout S is never kept: 12 per attempt)
        kinds.append(full)
        full_panels, thin = full_panels + (12 if full else 0), thin or (0 if full else 1)
    assert kinds == [1, 1, 0, 0, 0]
    c, uc = _numbers(lib, 7, 1, [1, 0, 1, 1, 1], thin_from=kinds.index(0))
    d, ud = _numbers(lib, 7, 1, [1, 0, 1, 1, 1])
    assert c == d and uc == ud == 32
    # numbers beyond 2^32 (the descriptor's evaluation is 64 bits wide)
    assert lib.ndcn_tape_attempt_evaluation(2 ** 40, 1, 3) == 2 ** 40 + 20


def test_routing_with_the_switch_set_and_unset(monkeypatch):
    """A dopri5 solve of a plain ODEFunc with an ACTIVE dropout takes the tape only under NDCN_TAPE_DROPOUT=1; eval mode, p = 0 and the
    other methods are untouched by the switch; p >= 1, NDCN_GRAD_TAPE=0, a time grid with gradient and options the device-resident
    solve declines keep the per-operation graph whatever the switch says.  CPU tensors: the decision, up to the device check."""
    from ndcn_amd.neural_dynamics import ODEFunc
    from ndcn_amd.torchdiffeq._impl import tape
    from ndcn_amd.torchdiffeq._impl.odeint import _dopri5_tape_route
    y = torch.zeros(5, 8)
    t = torch.linspace(0, 1, 3)
    src = open(os.path.join(ROOT, 'ndcn_amd', 'torchdiffeq', '_impl', 'tape.py')).read()
    assert "env_str('NDCN_TAPE_DROPOUT', '0')" in src             # read through the shared reader

    def route(f, method='dopri5', options=None, tt=t):
        return _dopri5_tape_route(f, True, (y,), tt, method, options or {})

    drop = ODEFunc(8, None, dropout=0.5, no_graph=True).train()
    plain = ODEFunc(8, None, no_graph=True).train()
    monkeypatch.delenv('NDCN_TAPE_DROPOUT', raising=False)
    assert not tape.dropout_enabled()
    assert route(drop) == (False, False)                           # as before this switch existed
    assert route(plain) == (True, True)
    assert route(ODEFunc(8, None, dropout=0.5, no_graph=True).eval()) == (True, True)
    monkeypatch.setenv('NDCN_TAPE_DROPOUT', '0')
    assert route(drop) == (False, False)
    monkeypatch.setenv('NDCN_TAPE_DROPOUT', '1')
    assert tape.dropout_enabled()
    # taped, but never `plain`: the per-operation graph must not fuse its stage algebra into evaluations that have no mask
    assert route(drop) == (False, True)
    assert route(ODEFunc(8, None, dropout=0.1, no_graph=True, no_control=True).train()) == (False, True)
    assert route(plain) == (True, True)
    assert route(drop, method='rk4') == (False, False)
    assert route(ODEFunc(8, None, dropout=1.0, no_graph=True).train()) == (False, False)       # p >= 1 keeps the un-fused branch
    assert route(drop, options={'first_step': 0.1}) == (False, False)
    assert route(drop, tt=t.clone().requires_grad_(True)) == (False, False)
    assert _dopri5_tape_route(drop, False, (y,), t, 'dopri5', {}) == (False, False)            # a tuple state
    assert _dopri5_tape_route(drop, True, (torch.zeros(5, 2, 8),), t, 'dopri5', {}) == (False, False)
    monkeypatch.setenv('NDCN_GRAD_TAPE', '0')
    assert route(drop) == (False, False) and route(plain) == (True, False)
    monkeypatch.delenv('NDCN_GRAD_TAPE')
    monkeypatch.setenv('NDCN_VJP', 'torch')
    assert route(drop) == (False, False)
