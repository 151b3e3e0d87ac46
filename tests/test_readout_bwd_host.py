"""The decoder-in-the-sweep entry points exist on every side of the C ABI, and the numpy restatement of the kernel's tick gradient
(tests/_readout_chain.py) is the exactly rounded fma chain (CPU only; tests/test_cabi.py compares the three export lists in full)."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np

from _readout_chain import combine, decoder_sums, tick_gradient
from test_fma_chain import _exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ndcn_readout_bwd_f32', 'ndcn_fixed_grid_backward_readout_f32')


def test_new_exports_are_declared_built_and_bound():
    from ndcn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()
    declared = set(re.findall(r'NDCN_API[^;(]*?\b(ndcn_\w+)\s*\(', header))
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r' T (ndcn_\w+)', out))
    for name in NEW:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION >= 27 and int(re.search(r'#define NDCN_ABI_VERSION (\d+)', header).group(1)) == _lib.ABI_VERSION


def test_tick_gradient_is_the_exact_fma_chain_at_c3():
    """gi = fma(gd2, W2, fma(gd1, W1, fma(gd0, W0, +0))) with every fma rounded once: against Fraction arithmetic, on operands with
    cancellation between the terms (where a separately rounded product would lose the low bits) and wide exponents"""
    rng = np.random.RandomState(0)
    N, H, C = 40, 7, 3
    gd = (rng.randn(N, C) * 2.0 ** rng.randint(-20, 20, (N, C))).astype(np.float32)
    Wd = (rng.randn(C, H) * 2.0 ** rng.randint(-8, 8, (C, H))).astype(np.float32)
    gd[:10, 1] = -gd[:10, 0]                               # cancellation: W rows 0 and 1 nearly equal below
    Wd[1] = Wd[0] * np.float32(1 + 2.0 ** -12)
    gd[10, :] = 0.0
    gd[11, 0] = -0.0
    got = tick_gradient(gd, Wd)
    for n in range(N):
        for h in range(H):
            acc = np.float32(0.0)
            for c in range(C):
                acc = _exact(gd[n, c], Wd[c, h], acc)
            assert got[n, h].view(np.int32) == np.float32(acc).view(np.int32), (n, h, float(got[n, h]), float(acc))
    # the chain is not the rounded exact sum: somewhere the two differ (else this test could not tell a chain from a dot product)
    exact = np.array([[float(sum(Fraction(float(gd[n, c])) * Fraction(float(Wd[c, h])) for c in range(C))) for h in range(H)]
                      for n in range(N)]).astype(np.float32)
    assert np.any(exact.view(np.int32) != got.view(np.int32))


def test_combine_order_and_decoder_sums():
    """out = a + ((0 + p0) + p1 + gi): the base last; -0 + -0 through the +0 start gives +0; no base and no addend: gi untouched"""
    gi = np.float32([[-0.0, 1.0, 2.0 ** -24]])
    assert np.signbit(combine(gi)[0, 0])
    assert not np.signbit(combine(gi, addends=[np.float32([[-0.0, 0, 0]])])[0, 0])
    a = np.float32([[0.0, 1.0, 1.0]])
    p = np.float32([[0.0, 0.0, 2.0 ** -24]])
    # (p + gi) = 2^-23 is added to 1 as a whole: 1 + 2^-23; base first would have lost both halves (ties to even)
    assert combine(gi, base=a, addends=[p])[0, 2] == np.float32(1 + 2.0 ** -23)
    gW, gb, mW, mb = decoder_sums(np.float32([[1, -2], [3, 4]]), np.float32([[1, 1, 1], [2, 0, -1]]))
    assert np.array_equal(gW, [[7, 1, -2], [6, -2, -6]]) and np.array_equal(gb, [4, 2])
    assert np.array_equal(mW, [[7, 1, 4], [10, 2, 6]]) and np.array_equal(mb, [4, 6])
