"""The budgeted training tape's host side (no GPU): the new entry points are declared and bound alike, the ABI numbers agree, and the
full / thin decision of an attempted step (ndcn_tape_attempt_is_full: a pure function, asked before every attempt) on hand-made
sequences."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()


def _prototype_args(name):
    m = re.search(r'NDCN_API[^;(]*?\b%s\s*\(([^;]*?)\)\s*;' % name, _header(), re.S)
    assert m, name + ' is not declared'
    return [a.strip() for a in m.group(1).split(',')]


def test_new_entry_points_are_declared_and_bound_with_the_same_argument_counts():
    from ndcn_amd import _lib
    for name in ('ndcn_tape_dopri5_budget_f32', 'ndcn_tape_record', 'ndcn_tape_attempt_is_full'):
        assert name in _lib.SIGNATURES
        assert len(_prototype_args(name)) == len(_lib.SIGNATURES[name][1]), name
    # the argument list of ndcn_tape_dopri5_f32 plus the budget, as int64
    plain, budget = _prototype_args('ndcn_tape_dopri5_f32'), _prototype_args('ndcn_tape_dopri5_budget_f32')
    assert budget[:-1] == plain and budget[-1] == 'int64_t record_budget_bytes'
    assert _lib.SIGNATURES['ndcn_tape_dopri5_budget_f32'][1][:-1] == _lib.SIGNATURES['ndcn_tape_dopri5_f32'][1]
    assert _lib.SIGNATURES['ndcn_tape_dopri5_budget_f32'][1][-1] is _lib._L


def test_abi_version_is_28_or_later_everywhere():
    from ndcn_amd import _lib
    version = int(re.search(r'#define NDCN_ABI_VERSION (\d+)', _header()).group(1))
    assert version == _lib.ABI_VERSION >= 28


def _walk(lib, budget, panel_bytes, keep_s, held_per_attempt):
    """the forward pass's bookkeeping over a sequence of attempts that each hold `held_per_attempt[i]` panels when full"""
    full_panels, thin, out = 0, 0, []
    for held in held_per_attempt:
        full = lib.ndcn_tape_attempt_is_full(budget, full_panels, panel_bytes, keep_s, thin)
        out.append(full)
        if full:
            full_panels += held
        else:
            thin = 1
    return out


def test_full_or_thin_decision():
    from ndcn_amd import _lib
    lib = _lib.load()
    pb = 1000
    # below zero: unlimited, whatever is held
    assert _walk(lib, -1, pb, 1, [18] * 5) == [1] * 5
    assert lib.ndcn_tape_attempt_is_full(-1, 10 ** 12, pb, 1, 0) == 1
    # zero: every attempt is thin
    assert _walk(lib, 0, pb, 0, [12] * 4) == [0] * 4
    # the exact boundary, keep_s off: an attempt costs 12 panels; 36 panels of budget hold three, one byte less holds two
    assert _walk(lib, 36 * pb, pb, 0, [12] * 5) == [1, 1, 1, 0, 0]
    assert _walk(lib, 36 * pb - 1, pb, 0, [12] * 5) == [1, 1, 0, 0, 0]
    # keep_s on: the test charges 18 although the attempts held 17 (the seventh evaluation kept no S)
    assert _walk(lib, (17 + 18) * pb, pb, 1, [17] * 4) == [1, 1, 0, 0]
    assert _walk(lib, (17 + 18) * pb - 1, pb, 1, [17] * 4) == [1, 0, 0, 0]
    assert _walk(lib, 18 * pb - 1, pb, 1, [17] * 3) == [0, 0, 0]
    assert _walk(lib, 18 * pb - 1, pb, 0, [12] * 3) == [1, 0, 0]
    # once thin, always thin: the flag decides even where the budget would hold the attempt
    assert lib.ndcn_tape_attempt_is_full(10 ** 9, 0, pb, 0, 1) == 0
    assert lib.ndcn_tape_attempt_is_full(10 ** 9, 0, pb, 0, 0) == 1
    # panels of the size this project is judged on: 1.024 GB, 25 attempts of 18, 288 GB of budget -> no 64-bit trouble
    big = 10 ** 6 * 256 * 4 + 16
    seq = _walk(lib, 288 * 10 ** 9, big, 1, [18] * 25)
    assert seq == [1] * 15 + [0] * 10


def test_budget_switch_is_read_through_the_shared_reader(monkeypatch):
    """NDCN_TAPE_BUDGET_MB: unset / empty = -1 (unlimited), a number = that many MiB"""
    from ndcn_amd import _lib
    monkeypatch.delenv('NDCN_TAPE_BUDGET_MB', raising=False)
    assert _lib.env_int('NDCN_TAPE_BUDGET_MB', -1) == -1
    monkeypatch.setenv('NDCN_TAPE_BUDGET_MB', '0')
    assert _lib.env_int('NDCN_TAPE_BUDGET_MB', -1) == 0
    src = open(os.path.join(ROOT, 'ndcn_amd', 'torchdiffeq', '_impl', 'tape.py')).read()
    assert "env_int('NDCN_TAPE_BUDGET_MB', -1)" in src
