"""ndcn_rhs_abl_supported / ndcn_set_rhs_abl (csrc/rhs_abl.hip): the shape predicate of the one-launch right-hand side of the no_control
and no_graph ablations and its process-wide switch.  Host code only: no device is touched."""
import os
import re

import pytest

from ndcn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (16, 20, 36, 64, 96, 100, 128)
NO_WIDTHS = (1, 12, 18, 130, 132, 256)
FORMS = (_lib.F_NO_CONTROL, _lib.F_NO_GRAPH)


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def test_path_bit_is_the_next_free_one():
    assert _lib.PATH_ABL == 8192
    others = (_lib.PATH_FUSED2, _lib.PATH_FUSED3, _lib.PATH_HUB, _lib.PATH_HALO, _lib.PATH_SWEEP, _lib.PATH_REC, _lib.PATH_WIDE,
              _lib.PATH_SMALL, _lib.PATH_EXACT32, _lib.PATH_RANGE, _lib.PATH_DROP_EPI, _lib.PATH_DYN, _lib.PATH_MID)
    assert all(_lib.PATH_ABL & o == 0 for o in others) and _lib.PATH_ABL == 2 * max(others)
    header = open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()
    assert re.search(r'#define NDCN_PATH_ABL\s+8192\b', header)


@pytest.mark.parametrize('flag', FORMS)
@pytest.mark.parametrize('H', WIDTHS)
def test_exactly_one_flag_takes_every_size(lib, H, flag):
    for n in (1, 63, 64, 65, 4161, 99856, 10 ** 7, (1 << 31) - 65):
        assert lib.ndcn_rhs_abl_supported(n, H, _lib.F_RELU | flag) == 1, (n, H)
        assert lib.ndcn_rhs_abl_supported(n, H, flag) == 1, (n, H)            # without the ReLU: K = S
    for n in (0, -1, (1 << 31) - 64, 1 << 31):
        assert lib.ndcn_rhs_abl_supported(n, H, _lib.F_RELU | flag) == 0, (n, H)


@pytest.mark.parametrize('H', WIDTHS)
def test_both_flags_or_neither_never(lib, H):
    for n in (1, 4096, 10 ** 6):
        assert lib.ndcn_rhs_abl_supported(n, H, _lib.F_RELU) == 0
        assert lib.ndcn_rhs_abl_supported(n, H, 0) == 0
        assert lib.ndcn_rhs_abl_supported(n, H, _lib.F_RELU | _lib.F_NO_GRAPH | _lib.F_NO_CONTROL) == 0


@pytest.mark.parametrize('flag', FORMS)
@pytest.mark.parametrize('H', NO_WIDTHS)
def test_other_widths_never(lib, H, flag):
    for n in (1, 4096, 10 ** 6):
        assert lib.ndcn_rhs_abl_supported(n, H, _lib.F_RELU | flag) == 0, (n, H)


def test_the_other_predicates_keep_their_answers(lib):
    """the ablation flags stay declined by the with-control launches, and the scratch size does not follow the switch"""
    prev = lib.ndcn_set_rhs_abl(1)
    try:
        for flag in FORMS:
            for H in WIDTHS:
                for mode in (1, 2):
                    assert lib.ndcn_rhs_mid_supported(10 ** 6, H, _lib.F_RELU | flag, mode) == 0
                    assert lib.ndcn_rhs_mid_bwd_supported(10 ** 6, H, _lib.F_RELU | flag, mode) == 0
                assert lib.ndcn_rhs_work_bytes(10 ** 6, H, _lib.F_RELU | flag) == 0
        assert lib.ndcn_rhs_work_bytes(10 ** 6, 20, _lib.F_RELU) == 10 ** 6 * 20 * 4
    finally:
        lib.ndcn_set_rhs_abl(prev)


def test_switch_returns_the_previous_value(lib):
    assert 'NDCN_RHS_ABL' not in os.environ or os.environ['NDCN_RHS_ABL'] in ('', '0')
    first = lib.ndcn_set_rhs_abl(1)
    try:
        assert first == 0                                      # off by default
        assert lib.ndcn_set_rhs_abl(0) == 1
        assert lib.ndcn_set_rhs_abl(7) == 0                    # any other positive value is on
        assert lib.ndcn_set_rhs_abl(-1) == 1                   # back to the environment's
        assert lib.ndcn_set_rhs_abl(-5) == 0
        from ndcn_amd import hip
        assert hip.set_rhs_abl(1) == 0 and hip.set_rhs_abl(0) == 1
    finally:
        lib.ndcn_set_rhs_abl(first)


def test_header_binding_and_call_list_agree():
    """the two calls stand in include/ndcn_hip.h with the binding's argument lists, under the current ABI number, and in INTEGRATION.md's
    list of calls"""
    header = open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()
    assert re.search(r'NDCN_API int ndcn_set_rhs_abl\(int on\);', header)
    assert re.search(r'NDCN_API int ndcn_rhs_abl_supported\(int64_t n_rows, int H, uint32_t flags\);', header)
    assert len(_lib.SIGNATURES['ndcn_set_rhs_abl'][1]) == 1 and len(_lib.SIGNATURES['ndcn_rhs_abl_supported'][1]) == 3
    assert int(re.search(r'#define NDCN_ABI_VERSION (\d+)', header).group(1)) == _lib.ABI_VERSION == 29
    calls = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert '`ndcn_set_rhs_abl`, `ndcn_rhs_abl_supported` (added to ABI 29' in calls
