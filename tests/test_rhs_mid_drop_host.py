"""ndcn_set_rhs_mid_drop (csrc/rhs_mid.hip): the process-wide switch that lets the dropout calls take the one-launch right-hand side for
hidden widths 16..128.  Host code only: no device is touched."""
import os
import subprocess
import sys

import pytest

from ndcn_amd import _lib


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def test_switch_returns_the_previous_value(lib):
    first = lib.ndcn_set_rhs_mid_drop(1)
    try:
        assert first in (0, 1)
        assert lib.ndcn_set_rhs_mid_drop(0) == 1
        assert lib.ndcn_set_rhs_mid_drop(1) == 0
        assert lib.ndcn_set_rhs_mid_drop(7) == 1                 # any positive value is "on"
        assert lib.ndcn_set_rhs_mid_drop(0) == 1
        assert lib.ndcn_set_rhs_mid_drop(1) == 0
        assert lib.ndcn_set_rhs_mid_drop(-1) == 1                # back to the environment's
        assert lib.ndcn_set_rhs_mid_drop(first) == first
        from ndcn_amd import hip
        assert hip.set_rhs_mid_drop(1) == first and hip.set_rhs_mid_drop(first) == 1
    finally:
        lib.ndcn_set_rhs_mid_drop(first)


def test_independent_of_the_mode_switches(lib):
    fwd, bwd, drop = lib.ndcn_set_rhs_mid(0), lib.ndcn_set_rhs_mid_bwd(0), lib.ndcn_set_rhs_mid_drop(1)
    try:
        assert lib.ndcn_set_rhs_mid(2) == 0 and lib.ndcn_set_rhs_mid_bwd(2) == 0 and lib.ndcn_set_rhs_mid_drop(1) == 1
        assert lib.ndcn_set_rhs_mid_drop(0) == 1 and lib.ndcn_set_rhs_mid(2) == 2 and lib.ndcn_set_rhs_mid_bwd(2) == 2
        # the shape predicate does not follow the dropout switch
        assert lib.ndcn_rhs_mid_supported(10 ** 5, 64, _lib.F_RELU, 2) == 1
    finally:
        lib.ndcn_set_rhs_mid(fwd)
        lib.ndcn_set_rhs_mid_bwd(bwd)
        lib.ndcn_set_rhs_mid_drop(drop)


CHILD = '''
from ndcn_amd import _lib
lib = _lib.load()
env = lib.ndcn_set_rhs_mid_drop(1)               # returns the environment's value
back = lib.ndcn_set_rhs_mid_drop(-1)
print(env, back, lib.ndcn_set_rhs_mid_drop(-1), lib.ndcn_set_rhs_mid(-1))
'''


@pytest.mark.parametrize('value,on', [(None, 0), ('0', 0), ('1', 1)])
def test_default_and_environment_fallback(value, on):
    """off by default; NDCN_RHS_MID_DROP is read once per process: a fresh interpreter per value (host code only).  The mode of
    ndcn_set_rhs_mid does not follow it."""
    env = dict(os.environ)
    env.pop('NDCN_RHS_MID_DROP', None)
    env.pop('NDCN_RHS_MID', None)
    if value is not None:
        env['NDCN_RHS_MID_DROP'] = value
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env['PYTHONPATH'] = root + os.pathsep + env.get('PYTHONPATH', '')
    out = subprocess.run([sys.executable, '-c', CHILD], env=env, cwd=root, capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [on, 1, on, 0]
