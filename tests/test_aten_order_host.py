"""The numpy models of tests/_aten_order.py ARE torch's single-thread float32 `sum` and `norm`, bit for bit, at every size the GPU test
(tests/test_gpu_rk_routes.py) compares the ATen-order kernels with them.  A torch build that sums in another order fails HERE, naming
its version and CPU capability, not inside a GPU test.  Runs without a GPU."""
import warnings

import numpy as np
import pytest
import torch

import _aten_order as ao


def _who():
    try:
        cap = torch.backends.cpu.get_cpu_capability()
    except Exception:                                   # older builds
        cap = 'unknown'
    return 'torch %s, CPU capability %s' % (torch.__version__, cap)


def _data(n, seed):
    """non-negative float32 with a spread of exponents: the addends of an error record"""
    rs = np.random.RandomState(seed)
    return (np.abs(rs.randn(n)) * np.exp2(rs.randint(-6, 7, n))).astype(np.float32)


def test_models_equal_torch_under_one_thread():
    bad_sum, bad_norm = [], []
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for n in ao.ATEN_SIZES + ao.ATEN_SIZES_RAISED_BOUND:
            v = _data(n, n)
            t = torch.from_numpy(v)
            if n >= 8 and np.float32(t.sum().item()) != ao.cascade_sum(v):          # below 8 elements the kernel takes the fp64 route
                bad_sum.append(n)
            if np.float32(t.norm().item()) != np.sqrt(ao.lane8_fma_sumsq(v)):
                bad_norm.append(n)
    finally:
        torch.set_num_threads(prev)
    assert torch.get_num_threads() == prev
    assert not bad_sum and not bad_norm, (
        '%s sums float32 in another order than tests/_aten_order.py (the order rk.hip reproduces): sum differs at n = %s, norm at n = %s'
        % (_who(), bad_sum[:20], bad_norm[:20]))


def test_vectorised_cascade_equals_the_serial_statement():
    """the hand-over conditions as SumKernel.cpp spells them, one 32-element step at a time, at the level edges"""
    for n in [1, 7, 8, 39, 40, 63, 64, 511, 512, 544, 8191, 8192, 8192 + 33, 131072 - 32, 131072, 131072 + 33, 173312, 1 << 18,
              (1 << 20) + 37]:
        v = _data(n, n + 1)
        assert ao.cascade_sum(v) == ao.cascade_sum_serial(v), n


def test_models_are_not_a_plain_sum():
    """the models distinguish their order from a left-to-right float32 sum and from a float32 sum of squares without fma (they would
    be useless oracles otherwise); max(|y0|, |y1|) propagates NaN from either side as torch.max does"""
    plain_differs = sq_differs = 0
    for seed in range(8):
        v = _data(8000, seed)
        s = q = np.float32(0)
        for x in v:
            s = np.float32(s + x)
            q = np.float32(q + np.float32(x * x))
        plain_differs += int(ao.cascade_sum(v) != s)
        sq_differs += int(ao.lane8_fma_sumsq(v) != q)
    assert plain_differs and sq_differs
    for y0, y1 in ((np.nan, 1.0), (1.0, np.nan)):
        assert np.isnan(ao.ratio_sq(np.float32(1), np.float32(y0), np.float32(y1), 1e-2, 1e-3))
        assert bool(torch.isnan(torch.max(torch.tensor(y0).abs(), torch.tensor(y1).abs())))


def test_thread_dependence_of_torch_sum_is_recorded():
    """Above 32768 elements torch.sum depends on the size of the thread pool; the kernels reproduce the single-thread order.  This test
    RECORDS where the threaded sum leaves the model and asserts nothing about it: if it never does (a torch whose sum no longer
    depends on the pool), it warns so that the oracle's one-thread wrapper can be revisited."""
    sizes = [32767, 32768, 32769, 65536, 65569, 131072, 173312, 200000, (1 << 18) - 1, 1 << 18]
    prev = torch.get_num_threads()
    differ = {}
    try:
        for threads in (8, 16):
            torch.set_num_threads(threads)
            differ[threads] = [n for n in sizes if np.float32(torch.from_numpy(_data(n, n)).sum().item()) != ao.cascade_sum(_data(n, n))]
    finally:
        torch.set_num_threads(prev)
    print('torch.sum vs the single-thread model (%s): differs at %s' % (_who(), differ))
    if not any(differ.values()):
        warnings.warn('torch.sum equals the single-thread cascade model at every size with 8 and 16 threads (%s): the thread '
                      'dependence the oracle guards against was not observed here - revisit tests/_oracle_ops.py' % _who())


def _sumsq_with_tail(q, base, fused):
    s = ao.lane8_fma_sumsq(q[:base])
    for x, f in zip(q[base:], fused):
        s = ao._fma32(x, x, s) if f else np.float32(s + np.float32(x * x))
    return s


def test_norm_tail_is_four_unfused_products_then_fma():
    """the n % 8 tail of torch.norm: a tail of 4..7 elements adds its first four as separately rounded products and the rest by fma; a
    shorter tail is all fma.  For every tail length, behind 8 and 16 full-vector elements, vectors are searched (in numpy alone) on
    which the model's norm differs from the all-fma tail's and from the all-unfused tail's: torch must side with the model on each."""
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for base in (8, 16):
            for t in range(1, 8):
                n = base + t
                model = tuple(0 if (t >= 4 and j < 4) else 1 for j in range(t))
                for other in ((1,) * t, (0,) * t):
                    if other == model:
                        continue
                    found = 0
                    for seed in range(4000):
                        q = _data(n, 7919 * seed + n)
                        m = np.sqrt(ao.lane8_fma_sumsq(q))
                        assert m == np.sqrt(_sumsq_with_tail(q, base, model))
                        if m == np.sqrt(_sumsq_with_tail(q, base, other)):
                            continue
                        found += 1
                        assert np.float32(torch.from_numpy(q).norm().item()) == m, (n, seed, model, other, _who())
                        if found == 5:
                            break
                    assert found == 5, (n, other)
    finally:
        torch.set_num_threads(prev)
