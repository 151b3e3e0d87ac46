"""The solver's switch for the one-launch kernels of hidden widths 16..128 (ndcn_set_solver_mid / NDCN_SOLVER_MID, csrc/solver.hip): what
can be said without a GPU - the four calls and the kind names in the header and the binding (ABI 29 unchanged), the switch's semantics,
and the sizes' part of the decision (ndcn_solver_mid_takes) as a pure function against a table."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ('ndcn_set_solver_mid', 'ndcn_solver_mid_mode', 'ndcn_solver_mid_takes', 'ndcn_solver_rhs_kind')


def test_header_and_binding_declare_the_calls_and_the_kinds():
    from ndcn_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()
    assert re.search(r'#define NDCN_ABI_VERSION 29\b', text) and _lib.ABI_VERSION == 29
    for name in NEW_CALLS:
        assert re.search(r'NDCN_API int %s\(' % name, text), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES['ndcn_solver_mid_takes'][1]) == 4 and len(_lib.SIGNATURES['ndcn_solver_mid_mode'][1]) == 0
    # the names of DeviceSolver.rhs_kind() are the header's, by value
    values = dict((k.lower(), int(v)) for k, v in re.findall(r'#define NDCN_SOLVER_RHS_(\w+)\s+(\d+)\b', text))
    assert values == dict((name, i) for i, name in enumerate(_lib.SOLVER_RHS_KINDS))
    assert _lib.SOLVER_RHS_KINDS[-2:] == ('mid', 'abl')
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert '`NDCN_SOLVER_MID`' in doc and '`ndcn_set_solver_mid`' in doc


def test_library_exports_the_calls():
    from ndcn_amd import _lib
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NEW_CALLS) <= set(re.findall(r' T (ndcn_\w+)', out))


def test_switch_returns_the_previous_mode_and_clamps():
    from ndcn_amd import _lib, hip
    lib = _lib.load()
    first = lib.ndcn_set_solver_mid(1)
    try:
        assert lib.ndcn_solver_mid_mode() == 1
        assert lib.ndcn_set_solver_mid(2) == 1 and lib.ndcn_solver_mid_mode() == 2
        assert lib.ndcn_set_solver_mid(9) == 2 and lib.ndcn_solver_mid_mode() == 2        # clamped
        assert lib.ndcn_set_solver_mid(0) == 2 and hip.solver_mid_mode() == 0
        assert hip.set_solver_mid(1) == 0 and hip.set_solver_mid(0) == 1
        # the training switches are others
        before = lib.ndcn_set_rhs_mid(0), lib.ndcn_set_rhs_abl(0)
        lib.ndcn_set_solver_mid(2)
        assert lib.ndcn_set_rhs_mid(before[0]) == 0 and lib.ndcn_set_rhs_abl(before[1]) == 0
        assert lib.ndcn_solver_rhs_kind(None) == _lib.EINVAL
    finally:
        lib.ndcn_set_solver_mid(first)


def test_default_is_off_and_the_environment_sets_it():
    code = ('from ndcn_amd import _lib\nlib = _lib.load()\nenv = lib.ndcn_solver_mid_mode()\nlib.ndcn_set_solver_mid(1 if env != 1 else 2)\n'
            'print(env, lib.ndcn_set_solver_mid(-1) != env, lib.ndcn_solver_mid_mode())')
    for value, want in ((None, '0 True 0'), ('1', '1 True 1'), ('2', '2 True 2'), ('7', '2 True 2'), ('0', '0 True 0')):
        env = dict(os.environ, PYTHONPATH=ROOT)
        env.pop('NDCN_SOLVER_MID', None)
        if value is not None:
            env['NDCN_SOLVER_MID'] = value
        out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True).stdout
        assert out.split() == want.split(), (value, out)


NG, NC = 'no_graph', 'no_control'
# (n_rows, H, ablation flags, mode) -> does the solver take 'mid' / 'abl' from the sizes?
TABLE = [
    # graph and control: rhs_mid.hip's widths; mode 1 stops at H = 96 and leaves the narrow-panel sizes alone
    ((16448, 16, (), 1), True), ((16448, 16, (), 2), True), ((13171, 20, (), 1), True), ((4099, 64, (), 1), True),
    ((2755, 96, (), 1), True), ((2647, 100, (), 1), False), ((2647, 100, (), 2), True), ((2051, 128, (), 1), False),
    ((2051, 128, (), 2), True), ((16384, 16, (), 1), False), ((16384, 16, (), 2), True), ((16385, 16, (), 1), True),
    ((400, 20, (), 1), False), ((400, 20, (), 2), True),
    ((100000, 12, (), 2), False), ((100000, 18, (), 2), False), ((100000, 132, (), 2), False), ((100000, 256, (), 2), False),
    ((0, 64, (), 2), False), ((2 ** 31, 64, (), 2), False),
    # exactly one ablation flag: rhs_abl.hip's widths at any size; mode 1 leaves H > 96 composed here too
    ((400, 20, (NC,), 1), True), ((13171, 20, (NC,), 1), True), ((4099, 64, (NC,), 1), True), ((2755, 96, (NC,), 1), True), ((2647, 100, (NC,), 1), False), ((2051, 128, (NC,), 1), False), ((2051, 128, (NC,), 2), True),
    ((400, 20, (NG,), 1), True), ((4099, 64, (NG,), 1), True), ((2755, 96, (NG,), 1), True), ((2647, 100, (NG,), 1), False),
    ((2051, 128, (NG,), 1), False), ((2051, 128, (NG,), 2), True), ((2647, 100, (NG,), 2), True),
    ((4099, 256, (NC,), 2), False), ((4099, 256, (NG,), 2), False), ((4099, 12, (NC,), 2), False), ((4099, 22, (NG,), 2), False),
    ((4099, 64, (NG, NC), 2), False), ((4099, 64, (NG, NC), 1), False),
]


@pytest.mark.parametrize('case,want', TABLE)
def test_sizes_decision_table(case, want):
    from ndcn_amd import hip
    n, H, abl, mode = case
    assert hip.solver_mid_takes(n, H, no_graph=NG in abl, no_control=NC in abl, mode=mode) is want
    assert hip.solver_mid_takes(n, H, no_graph=NG in abl, no_control=NC in abl, mode=0) is False
    assert hip.solver_mid_takes(n, H, no_graph=NG in abl, no_control=NC in abl, mode=3) is False
