"""ndcn_rhs_mid_supported / ndcn_set_rhs_mid (csrc/rhs_mid.hip): the shape predicate of the one-launch right-hand side for
hidden widths 16..128 and its process-wide switch.  Host code only: no device is touched."""
import pytest

from ndcn_amd import _lib

SMALL_MAX = 1 << 18          # rhs_small.hip takes n H up to here (rhs_small_wanted)
WIDTHS = (16, 20, 32, 64, 100, 128)
NO_WIDTHS = (12, 18, 132, 256)
MODE_1_MAX_H = 96            # above it (P = 128, one workgroup per CU) the launch measured slower than composed: mode 2 only


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def test_path_bit():
    assert _lib.PATH_MID == 4096
    others = (_lib.PATH_FUSED2, _lib.PATH_FUSED3, _lib.PATH_HUB, _lib.PATH_HALO, _lib.PATH_SWEEP, _lib.PATH_REC, _lib.PATH_WIDE,
              _lib.PATH_SMALL, _lib.PATH_EXACT32, _lib.PATH_RANGE, _lib.PATH_DROP_EPI, _lib.PATH_DYN)
    assert all(_lib.PATH_MID & o == 0 for o in others)


@pytest.mark.parametrize('H', WIDTHS)
def test_mode_2_takes_every_size(lib, H):
    for n in (1, 63, 64, 65, 129, 2049, 99856, 10 ** 7):
        assert lib.ndcn_rhs_mid_supported(n, H, _lib.F_RELU, 2) == 1, (n, H)
        assert lib.ndcn_rhs_mid_supported(n, H, 0, 2) == 1, (n, H)
    assert lib.ndcn_rhs_mid_supported(0, H, _lib.F_RELU, 2) == 0


@pytest.mark.parametrize('H', NO_WIDTHS)
def test_other_widths_never(lib, H):
    for mode in (0, 1, 2):
        for n in (1, 4096, 10 ** 6):
            assert lib.ndcn_rhs_mid_supported(n, H, _lib.F_RELU, mode) == 0, (n, H, mode)


@pytest.mark.parametrize('flag', (_lib.F_NO_GRAPH, _lib.F_NO_CONTROL, _lib.F_NO_GRAPH | _lib.F_NO_CONTROL))
def test_no_graph_and_no_control_never(lib, flag):
    for H in WIDTHS:
        for mode in (1, 2):
            assert lib.ndcn_rhs_mid_supported(10 ** 6, H, _lib.F_RELU | flag, mode) == 0


def test_mode_0_and_unknown_modes_never(lib):
    for H in WIDTHS:
        for n in (1, 10 ** 6):
            for mode in (0, -1, 3):
                assert lib.ndcn_rhs_mid_supported(n, H, _lib.F_RELU, mode) == 0


@pytest.mark.parametrize('H', [h for h in WIDTHS if h > MODE_1_MAX_H] + [MODE_1_MAX_H + 4])
def test_mode_1_leaves_the_widest_to_the_composed_path(lib, H):
    for n in (1, SMALL_MAX // H, SMALL_MAX // H + 1, 99856, 10 ** 7):
        assert lib.ndcn_rhs_mid_supported(n, H, _lib.F_RELU, 1) == 0, (n, H)
        assert lib.ndcn_rhs_mid_supported(n, H, _lib.F_RELU, 2) == 1, (n, H)


@pytest.mark.parametrize('H', [h for h in WIDTHS if h <= MODE_1_MAX_H] + [MODE_1_MAX_H])
def test_mode_1_starts_where_the_narrow_kernel_stops(lib, H):
    n_last = SMALL_MAX // H                                  # the largest n with n H <= 2^18
    assert n_last * H <= SMALL_MAX < (n_last + 1) * H
    assert lib.ndcn_rhs_mid_supported(n_last, H, _lib.F_RELU, 1) == 0
    assert lib.ndcn_rhs_mid_supported(1, H, _lib.F_RELU, 1) == 0
    assert lib.ndcn_rhs_mid_supported(n_last + 1, H, _lib.F_RELU, 1) == 1
    if SMALL_MAX % H == 0:
        assert lib.ndcn_rhs_mid_supported(SMALL_MAX // H + 1, H, _lib.F_RELU, 1) == 1       # n H = 2^18 + H
    # the scratch size does not follow the mode: it can flip between calls
    assert lib.ndcn_rhs_work_bytes(n_last + 1, H, _lib.F_RELU) == (n_last + 1) * H * 4


def test_switch_returns_the_previous_mode(lib):
    first = lib.ndcn_set_rhs_mid(2)
    try:
        assert first in (0, 1, 2)
        assert lib.ndcn_set_rhs_mid(1) == 2
        assert lib.ndcn_set_rhs_mid(0) == 1
        assert lib.ndcn_set_rhs_mid(7) == 0                  # clamped
        assert lib.ndcn_set_rhs_mid(-1) == 2                 # back to the environment's
        assert lib.ndcn_set_rhs_mid(first) == first
        from ndcn_amd import hip
        assert hip.set_rhs_mid(1) == first and hip.set_rhs_mid(first) == 1
    finally:
        lib.ndcn_set_rhs_mid(first)
