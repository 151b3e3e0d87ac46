"""ndcn_dropout_combine_f32 (csrc/dropout.hip: the dropout factor and the stage sum that consumes the masked derivative as ONE pass)
against the two kernels it replaces, ndcn_dropout_apply_f32 followed by ndcn_rk_combine_f32: the contract is bits, on K and on out -
at every size edge of its lanes (16-byte lanes, the n & 3 tail, the scalar lanes of misaligned views), for every number of earlier
stages, with and without y0, and with the mask's index origin at K wherever K starts."""
import ctypes

import numpy as np
import pytest
import torch

import _philox

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 4099, 2 ** 18 + 3]            # below a lane, tail only, one lane, lane + tail, odd, several blocks + tail, large
ALIGN = ['aligned', 'K_offset', 'out_offset', 'kprev_offset']
P_BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
# (p, seed, evaluation): three probabilities, two seeds, an evaluation number above 2^32 - cycled over the inner cases
DESCS = [(0.1, 0x1234567890ABCDEF, 0), (0.5, 7, 3), (P_BELOW_ONE, 7, 2 ** 32 + 5), (0.5, 0x1234567890ABCDEF, 2 ** 32 + 5),
         (0.1, 7, 2 ** 40 + 1), (P_BELOW_ONE, 0x1234567890ABCDEF, 11)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need a ROCm device'
    return torch.device('cuda:0')


def bits(x):
    return x.contiguous().view(torch.int32)


def _view(buf, off, n):
    """n floats of a (256-byte aligned) buffer from float `off` on: off = 1 is a view no 16-byte lane can serve"""
    v = buf[off:off + n]
    assert (v.data_ptr() % 16 == 0) == (off % 4 == 0)
    return v


def _reference(lib, K, desc, out, y0, kprev, cs):
    from ndcn_amd import _lib
    n = K.numel()
    _lib.check(lib.ndcn_dropout_apply_f32(_lib.ptr(K), n, _lib.dropout_desc(desc), _lib.stream_ptr()))
    ks = list(kprev) + [K]
    arr_k = (ctypes.c_void_p * len(ks))(*[k.data_ptr() for k in ks])
    arr_c = (ctypes.c_float * len(ks))(*cs)
    _lib.check(lib.ndcn_rk_combine_f32(_lib.ptr(out), _lib.ptr(y0), arr_k, arr_c, len(ks), n, _lib.stream_ptr()))


@pytest.mark.parametrize('align', ALIGN)
@pytest.mark.parametrize('n', SIZES)
def test_one_pass_equals_apply_then_combine(dev, n, align):
    from ndcn_amd import _lib, hip
    lib = _lib.load()
    assert lib.ndcn_abi_version() == 29
    g = torch.Generator().manual_seed(n)
    src = torch.randn(8, n + 8, generator=g).to(dev)                  # K, y0 and up to five earlier stages
    src[0, :n + 8][::max(n // 3, 1)] = 0.0                           # (exact zeros, as a ReLU leaves them)
    cs_all = [0.3, -0.0117, 1.75, -2.5e-3, 0.0421, 0.2]
    case = 0
    for n_prev in range(6):
        for with_y0 in (True, False):
            for rep in range(3):
                desc = DESCS[case % len(DESCS)]
                case += 1
                offK = 1 if align == 'K_offset' else 0
                offO = 1 if align == 'out_offset' else 0
                bufs = [torch.empty(n + 8, device=dev) for _ in range(4)]
                K1, K2 = _view(bufs[0], offK, n), _view(bufs[1], offK, n)
                K1.copy_(src[0, :n])
                K1[0] = -0.0
                if n >= 2:
                    K1[n - 1] = float('nan')
                if n >= 5:
                    K1[n // 2] = float('inf')
                K2.copy_(K1)
                o1, o2 = _view(bufs[2], offO, n).fill_(-7.0), _view(bufs[3], offO, n).fill_(-9.0)
                y0 = src[1, :n].clone() if with_y0 else None
                kprev = []
                for j in range(n_prev):
                    off = 1 if (align == 'kprev_offset' and j == n_prev - 1) else 0
                    kprev.append(_view(torch.empty(n + 8, device=dev), off, n).copy_(src[2 + j, :n]))
                cs = cs_all[:n_prev] + [cs_all[5 - rep]]
                hip.dropout_combine(K1, desc, kprev, cs, y0=y0, out=o1)
                _reference(lib, K2, desc, o2, y0, kprev, cs)
                assert torch.equal(bits(K1), bits(K2)), (n_prev, with_y0, desc)
                assert torch.equal(bits(o1), bits(o2)), (n_prev, with_y0, desc)
    assert case == 36


def test_nothing_is_written_outside_the_panels(dev):
    """guard floats before and behind K and out keep their values, aligned and misaligned, lane-sized and tail-sized n"""
    from ndcn_amd import hip
    for n in (1, 4, 5, 1023):
        for off in (4, 5):
            bK, bO = torch.full((n + 16,), 3.0, device=dev), torch.full((n + 16,), 4.0, device=dev)
            K, out = bK[off:off + n], bO[off:off + n]
            K.copy_(torch.rand(n))
            hip.dropout_combine(K, (0.5, 1, 2), [], [0.5], y0=None, out=out)
            assert bool((bK[:off] == 3.0).all()) and bool((bK[off + n:] == 3.0).all())
            assert bool((bO[:off] == 4.0).all()) and bool((bO[off + n:] == 4.0).all())


@pytest.mark.parametrize('off', [0, 1])
def test_against_the_numpy_philox_contract(dev, off):
    """one small case against tests/_philox.py and float32 numpy arithmetic in the kernel's order: the mask index starts at K[0]
    wherever K lies in memory"""
    from ndcn_amd import hip
    n, p, seed, ev = 37, 0.5, 0xDEADBEEF12345678, 2 ** 32 + 9
    rng = np.random.default_rng(4)
    Kh, y0h, k0h, k1h = [rng.standard_normal(n).astype(np.float32) for _ in range(4)]
    c = [np.float32(0.25), np.float32(-1.5), np.float32(0.0625 * 3)]
    m = _philox.mask(p, seed, ev, 1, n).reshape(-1)
    Kd = (Kh * m).astype(np.float32)
    acc = np.float32(0.0) + c[0] * k0h
    acc = (acc + (c[1] * k1h).astype(np.float32)).astype(np.float32)
    acc = (acc + (c[2] * Kd).astype(np.float32)).astype(np.float32)
    want = (y0h + acc).astype(np.float32)
    buf = torch.empty(n + 8, device=dev)
    K = buf[off:off + n].copy_(torch.from_numpy(Kh))
    _, out = hip.dropout_combine(K, (p, seed, ev), [torch.from_numpy(k0h).to(dev), torch.from_numpy(k1h).to(dev)], [float(x) for x in c],
                                 y0=torch.from_numpy(y0h).to(dev))
    assert 0 < int((m == 0).sum()) < n
    assert np.array_equal(K.cpu().numpy().view(np.int32), Kd.view(np.int32))
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))


def test_the_composed_stage_launch_runs_the_one_pass_kernel_and_keeps_its_bits(dev):
    """ndcn_rhs_rk_drop_f32 in combine mode at H = 256 (a route without a dropout epilogue): K and the next stage input equal
    rhs + dropout_apply + combine, and the mask is still not inside the right-hand-side launch (NDCN_PATH_DROP_EPI clear)"""
    from ndcn_amd import _lib, graphs, hip
    side, H = 12, 256
    A = graphs.to_device(graphs.normalized_laplacian(graphs.grid_8_neighbor(side)), dev)
    g = torch.Generator().manual_seed(1)
    X, y0, k1 = [torch.rand(side * side, H, generator=g).to(dev) for _ in range(3)]
    W = (torch.randn(H, H, generator=g) / 16).to(dev)
    b = torch.randn(H, generator=g).to(dev)
    desc = (0.5, 99, 2 ** 33)
    for no_control in (False, True):
        K, u = hip.rhs_rk(A, X, W, b, 'combine', y0, [k1], [0.125, -0.75], no_control=no_control, dropout=desc)
        assert not int(_lib.load().ndcn_debug_last_rhs_path()) & _lib.PATH_DROP_EPI
        Kr = hip.dropout_apply(hip.rhs(A, X, W, b, no_control=no_control), desc)
        ur = hip.combine(y0, [k1, Kr], [0.125, -0.75])
        assert torch.equal(bits(K), bits(Kr)) and torch.equal(bits(u), bits(ur))
        assert 0.3 < float((K == 0).float().mean()) < 0.9
