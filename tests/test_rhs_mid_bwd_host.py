"""ndcn_rhs_mid_bwd_supported / ndcn_set_rhs_mid_bwd (csrc/rhs_mid_bwd.hip): the shape predicate of the one-launch reverse of the
right-hand side for hidden widths 16..128 and its process-wide switch.  Host code only: no device is touched."""
import os
import subprocess
import sys

import pytest

from ndcn_amd import _lib

WIDTHS = (16, 20, 32, 64, 96, 100, 128)
NO_WIDTHS = (12, 18, 132, 256)
MODE_1_MAX_H = 128          # kMbMode1MaxH: the largest measured width at which the fused reverse is not slower - the widest one
SIZES = (1, 15, 16, 17, 37, 4096, 4097, 99856, 10 ** 7)


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def test_route_values():
    assert (_lib.VJP_COMPOSED, _lib.VJP_MID) == (1, 2)


@pytest.mark.parametrize('H', WIDTHS)
def test_mode_2_takes_every_size(lib, H):
    for n in SIZES:
        assert lib.ndcn_rhs_mid_bwd_supported(n, H, _lib.F_RELU, 2) == 1, (n, H)
        assert lib.ndcn_rhs_mid_bwd_supported(n, H, 0, 2) == 1, (n, H)
    assert lib.ndcn_rhs_mid_bwd_supported(0, H, _lib.F_RELU, 2) == 0
    assert lib.ndcn_rhs_mid_bwd_supported((1 << 31) - 65, H, _lib.F_RELU, 2) == 1
    assert lib.ndcn_rhs_mid_bwd_supported((1 << 31) - 64, H, _lib.F_RELU, 2) == 0       # declined from 2^31 - 64 rows on


@pytest.mark.parametrize('H', NO_WIDTHS)
def test_other_widths_never(lib, H):
    for mode in (0, 1, 2):
        for n in SIZES:
            assert lib.ndcn_rhs_mid_bwd_supported(n, H, _lib.F_RELU, mode) == 0, (n, H, mode)


@pytest.mark.parametrize('flag', (_lib.F_NO_GRAPH, _lib.F_NO_CONTROL, _lib.F_NO_GRAPH | _lib.F_NO_CONTROL))
def test_no_graph_and_no_control_never(lib, flag):
    for H in WIDTHS:
        for mode in (1, 2):
            assert lib.ndcn_rhs_mid_bwd_supported(10 ** 5, H, _lib.F_RELU | flag, mode) == 0


def test_mode_0_and_unknown_modes_never(lib):
    for H in WIDTHS:
        for n in (1, 10 ** 5):
            for mode in (0, 3, 7):
                assert lib.ndcn_rhs_mid_bwd_supported(n, H, _lib.F_RELU, mode) == 0


@pytest.mark.parametrize('H', WIDTHS)
def test_mode_1_takes_the_measured_widths(lib, H):
    want = 1 if H <= MODE_1_MAX_H else 0
    for n in SIZES:
        assert lib.ndcn_rhs_mid_bwd_supported(n, H, _lib.F_RELU, 1) == want, (n, H)


def test_switch_returns_the_previous_mode(lib):
    first = lib.ndcn_set_rhs_mid_bwd(2)
    try:
        assert first in (0, 1, 2)
        assert lib.ndcn_set_rhs_mid_bwd(1) == 2
        assert lib.ndcn_set_rhs_mid_bwd(0) == 1
        assert lib.ndcn_set_rhs_mid_bwd(7) == 0                  # clamped
        assert lib.ndcn_set_rhs_mid_bwd(-1) == 2                 # back to the environment's
        assert lib.ndcn_set_rhs_mid_bwd(first) == first
        from ndcn_amd import hip
        assert hip.set_rhs_mid_bwd(2) == first and hip.set_rhs_mid_bwd(first) == 2
    finally:
        lib.ndcn_set_rhs_mid_bwd(first)


def test_negative_mode_asks_for_the_current_one(lib):
    first = lib.ndcn_set_rhs_mid_bwd(2)
    try:
        assert lib.ndcn_rhs_mid_bwd_supported(100, 128, _lib.F_RELU, -1) == 1
        lib.ndcn_set_rhs_mid_bwd(0)
        assert lib.ndcn_rhs_mid_bwd_supported(100, 128, _lib.F_RELU, -1) == 0
    finally:
        lib.ndcn_set_rhs_mid_bwd(first)


def test_the_two_switches_are_independent(lib):
    fwd, bwd = lib.ndcn_set_rhs_mid(0), lib.ndcn_set_rhs_mid_bwd(2)
    try:
        assert lib.ndcn_set_rhs_mid(1) == 0 and lib.ndcn_set_rhs_mid_bwd(2) == 2
        assert lib.ndcn_set_rhs_mid_bwd(0) == 2 and lib.ndcn_set_rhs_mid(1) == 1
    finally:
        lib.ndcn_set_rhs_mid(fwd)
        lib.ndcn_set_rhs_mid_bwd(bwd)


CHILD = '''
import sys
from ndcn_amd import _lib
lib = _lib.load()
env = lib.ndcn_set_rhs_mid_bwd(2)                # returns the environment's mode
back = lib.ndcn_set_rhs_mid_bwd(-1)
print(env, back, lib.ndcn_set_rhs_mid_bwd(-1), lib.ndcn_rhs_mid_bwd_supported(100, 64, 1, -1))
'''


@pytest.mark.parametrize('value,mode', [(None, 0), ('0', 0), ('1', 1), ('2', 2), ('9', 2)])
def test_environment_fallback(value, mode):
    """NDCN_RHS_MID_BWD is read once per process: a fresh interpreter per value (host code only)"""
    env = dict(os.environ)
    env.pop('NDCN_RHS_MID_BWD', None)
    if value is not None:
        env['NDCN_RHS_MID_BWD'] = value
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env['PYTHONPATH'] = root + os.pathsep + env.get('PYTHONPATH', '')
    out = subprocess.run([sys.executable, '-c', CHILD], env=env, cwd=root, capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [mode, 2, mode, 1 if mode else 0]
