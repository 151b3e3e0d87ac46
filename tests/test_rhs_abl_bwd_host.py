"""ndcn_rhs_abl_bwd_supported / ndcn_set_rhs_abl_bwd / ndcn_rhs_abl_bwd_on (csrc/rhs_abl_bwd.hip): the shape predicate of the one-launch
reverse of the no_control and no_graph ablations and its process-wide switch.  Host code only: no device is touched."""
import os
import re
import subprocess
import sys

import pytest

from ndcn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (16, 20, 32, 64, 96, 100, 128)
NO_WIDTHS = (12, 18, 132, 256)
SIZES = (1, 15, 16, 17, 37, 4096, 4097, 99856, 10 ** 7, (1 << 31) - 65)
NO_SIZES = (0, (1 << 31) - 64)
FORMS = (_lib.F_NO_CONTROL, _lib.F_NO_GRAPH)


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def test_route_values():
    assert (_lib.VJP_COMPOSED, _lib.VJP_MID, _lib.VJP_ABL) == (1, 2, 3)
    header = open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()
    assert re.search(r'#define NDCN_VJP_ABL\s+3\b', header)


@pytest.mark.parametrize('flag', FORMS)
@pytest.mark.parametrize('H', WIDTHS)
def test_exactly_one_flag_takes_every_size(lib, H, flag):
    for n in SIZES:
        assert lib.ndcn_rhs_abl_bwd_supported(n, H, _lib.F_RELU | flag) == 1, (n, H)
        assert lib.ndcn_rhs_abl_bwd_supported(n, H, flag) == 1, (n, H)
    for n in NO_SIZES:
        assert lib.ndcn_rhs_abl_bwd_supported(n, H, _lib.F_RELU | flag) == 0, (n, H)


@pytest.mark.parametrize('flag', FORMS)
@pytest.mark.parametrize('H', NO_WIDTHS)
def test_other_widths_never(lib, H, flag):
    for n in SIZES:
        assert lib.ndcn_rhs_abl_bwd_supported(n, H, _lib.F_RELU | flag) == 0, (n, H)


@pytest.mark.parametrize('H', WIDTHS)
def test_both_flags_or_neither_never(lib, H):
    for n in SIZES:
        assert lib.ndcn_rhs_abl_bwd_supported(n, H, _lib.F_RELU) == 0
        assert lib.ndcn_rhs_abl_bwd_supported(n, H, 0) == 0
        assert lib.ndcn_rhs_abl_bwd_supported(n, H, _lib.F_RELU | _lib.F_NO_GRAPH | _lib.F_NO_CONTROL) == 0


def test_the_predicate_does_not_follow_the_switch(lib):
    prev = lib.ndcn_set_rhs_abl_bwd(0)
    try:
        for on in (0, 1):
            lib.ndcn_set_rhs_abl_bwd(on)
            assert lib.ndcn_rhs_abl_bwd_supported(100, 20, _lib.F_RELU | _lib.F_NO_GRAPH) == 1
            assert lib.ndcn_rhs_abl_bwd_supported(100, 256, _lib.F_RELU | _lib.F_NO_GRAPH) == 0
    finally:
        lib.ndcn_set_rhs_abl_bwd(prev)


def test_the_full_model_predicate_and_the_scratch_keep_their_answers(lib):
    """ndcn_rhs_mid_bwd_supported still declines the ablation flags, and ndcn_rhs_vjp_work_bytes does not follow the switch"""
    prev = lib.ndcn_set_rhs_abl_bwd(0)
    try:
        sizes = {}
        for on in (0, 1):
            lib.ndcn_set_rhs_abl_bwd(on)
            for flag in FORMS + (_lib.F_NO_GRAPH | _lib.F_NO_CONTROL,):
                for H in WIDTHS:
                    for mode in (1, 2):
                        assert lib.ndcn_rhs_mid_bwd_supported(10 ** 5, H, _lib.F_RELU | flag, mode) == 0
            sizes[on] = [lib.ndcn_rhs_vjp_work_bytes(n, H, _lib.F_RELU | flag) for n in (37, 99856) for H in WIDTHS for flag in FORMS]
        assert sizes[0] == sizes[1] and min(sizes[0]) > 0
    finally:
        lib.ndcn_set_rhs_abl_bwd(prev)


def test_switch_returns_the_previous_value(lib):
    assert 'NDCN_RHS_ABL_BWD' not in os.environ or os.environ['NDCN_RHS_ABL_BWD'] in ('', '0')
    first = lib.ndcn_set_rhs_abl_bwd(1)
    try:
        assert first == 0                                      # off by default
        assert lib.ndcn_rhs_abl_bwd_on() == 1
        assert lib.ndcn_set_rhs_abl_bwd(0) == 1
        assert lib.ndcn_rhs_abl_bwd_on() == 0
        assert lib.ndcn_set_rhs_abl_bwd(7) == 0                # any other positive value is on
        assert lib.ndcn_rhs_abl_bwd_on() == 1
        assert lib.ndcn_set_rhs_abl_bwd(-1) == 1               # back to the environment's
        assert lib.ndcn_rhs_abl_bwd_on() == 0
        assert lib.ndcn_set_rhs_abl_bwd(-5) == 0
        from ndcn_amd import hip
        assert hip.set_rhs_abl_bwd(1) == 0 and hip.rhs_abl_bwd_on() == 1 and hip.set_rhs_abl_bwd(0) == 1 and hip.rhs_abl_bwd_on() == 0
    finally:
        lib.ndcn_set_rhs_abl_bwd(first)


def test_the_switches_are_independent(lib):
    names = ('ndcn_set_rhs_abl', 'ndcn_set_rhs_mid_bwd', 'ndcn_set_rhs_mid')
    prev = [getattr(lib, nm)(0) for nm in names]
    mine = lib.ndcn_set_rhs_abl_bwd(0)
    try:
        assert lib.ndcn_set_rhs_abl_bwd(1) == 0
        assert [getattr(lib, nm)(1) for nm in names] == [0, 0, 0]      # the others did not move with it ...
        assert lib.ndcn_set_rhs_abl_bwd(0) == 1                       # ... and it did not move with them
        assert [getattr(lib, nm)(0) for nm in names] == [1, 1, 1]
        assert lib.ndcn_set_rhs_abl_bwd(0) == 0
    finally:
        for nm, v in zip(names, prev):
            getattr(lib, nm)(v)
        lib.ndcn_set_rhs_abl_bwd(mine)


CHILD = '''
from ndcn_amd import _lib
lib = _lib.load()
now = lib.ndcn_rhs_abl_bwd_on()
env = lib.ndcn_set_rhs_abl_bwd(1 - now)          # returns the environment's value
back = lib.ndcn_set_rhs_abl_bwd(-1)
print(now, env, back, lib.ndcn_set_rhs_abl_bwd(-1), lib.ndcn_rhs_abl_bwd_on())
'''


@pytest.mark.parametrize('value,on', [(None, 0), ('', 0), ('0', 0), ('1', 1), ('2', 1), ('-3', 0)])
def test_environment_fallback(value, on):
    """NDCN_RHS_ABL_BWD is read once per process: a fresh interpreter per value (host code only)"""
    env = dict(os.environ)
    env.pop('NDCN_RHS_ABL_BWD', None)
    if value is not None:
        env['NDCN_RHS_ABL_BWD'] = value
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    out = subprocess.run([sys.executable, '-c', CHILD], env=env, cwd=ROOT, capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [on, on, 1 - on, on, on]


def test_header_binding_and_documents_agree():
    """the calls stand in include/ndcn_hip.h with the binding's argument lists, under the current ABI number; the environment variable
    stands in INTEGRATION.md's table"""
    header = open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()
    assert re.search(r'NDCN_API int ndcn_set_rhs_abl_bwd\(int on\);', header)
    assert re.search(r'NDCN_API int ndcn_rhs_abl_bwd_on\(void\);', header)
    assert re.search(r'NDCN_API int ndcn_rhs_abl_bwd_supported\(int64_t n_rows, int H, uint32_t flags\);', header)
    assert len(_lib.SIGNATURES['ndcn_set_rhs_abl_bwd'][1]) == 1 and len(_lib.SIGNATURES['ndcn_rhs_abl_bwd_supported'][1]) == 3
    assert len(_lib.SIGNATURES['ndcn_rhs_abl_bwd_on'][1]) == 0
    assert int(re.search(r'#define NDCN_ABI_VERSION (\d+)', header).group(1)) == _lib.ABI_VERSION == 29
    assert '`NDCN_RHS_ABL_BWD`' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
