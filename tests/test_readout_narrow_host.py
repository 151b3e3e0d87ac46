"""Host side of the narrow-width readout (rk.hip readout_narrow_kernel, 16 <= H <= 60): the decode of one (row, output) restated
in numpy - acc = 0, acc = fma(s[k], w[k], acc) for k = 0 .. H - 1 in order, then acc + bias, the arithmetic of linear_small_kernel
that the kernel must keep - pinned against the sequential chain of tests/_fma_chain.py, and the route bit NDCN_READOUT_NARROW in the
header and the binding."""
import os
import re

import numpy as np

from _fma_chain import chain, fma32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = list(range(16, 64, 4))


def decode_one(s, w, bias=None):
    """one (row, o) of the kernel: the in-order fma chain from +0, then the bias as a separate fp32 addition"""
    acc = np.float32(0.0)
    for k in range(len(s)):
        acc = fma32(s[k], w[k], acc)[()]
    if bias is not None:
        with np.errstate(invalid='ignore', over='ignore'):
            acc = np.float32(acc + np.float32(bias))
    return np.float32(acc)


def rows(H, seed):
    """random rows with the values a last-bit or order mistake shows on: -0.0, denormals, magnitudes 2^20 apart, one NaN"""
    g = np.random.default_rng(seed)
    S = (g.standard_normal((9, H)) * np.exp2(g.integers(-10, 11, (9, H)))).astype(np.float32)
    S[1, 0] = S[1, H - 1] = np.float32(-0.0)
    S[2, :] = np.float32(-0.0)                                   # every product a zero: the chain from +0 ends in +0
    S[3, 1::3] = np.float32(1e-41)                               # denormal elements
    S[4, :] = (g.standard_normal(H) * 1e-40).astype(np.float32)  # a denormal row: denormal products and sums
    S[5, H // 2] = np.float32('nan')
    w = (g.standard_normal(H) * np.exp2(g.integers(-4, 5, H))).astype(np.float32)
    w[3] = np.float32(-0.0)
    return S, w


def bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def test_the_decode_of_one_row_is_the_sequential_chain():
    for H in WIDTHS:
        S, w = rows(H, H)
        n = S.shape[0]
        # the dot product of row r as a sparse row: entries (k, s[r, k]) in order against the column vector w
        ref = chain(np.arange(n + 1) * H, np.tile(np.arange(H), n), S.reshape(-1), w.reshape(H, 1))[:, 0]
        for bias in (None, np.float32(0.375), np.float32(-0.0)):
            got = np.array([decode_one(S[r], w, bias) for r in range(n)], np.float32)
            with np.errstate(invalid='ignore'):
                want = ref if bias is None else (ref + bias).astype(np.float32)
            assert np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)]), (H, bias)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 1
        assert bits(decode_one(S[2], w))[()] == 0                                   # +0, not -0
        assert bits(decode_one(S[2], w, np.float32(-0.0)))[()] == 0                 # +0 + -0 = +0: why a null bias adds nothing
        assert np.any(np.abs(S[4]) < np.float32(1.17549435e-38))


def test_the_order_of_the_chain_shows_in_the_last_bit():
    """the restatement pins an ORDER: the same rows summed from the other end, or in two halves, round differently somewhere"""
    differs_rev = differs_halves = 0
    for H in WIDTHS:
        S, w = rows(H, 100 + H)
        for r in (0, 1, 6, 7, 8):
            fwd = decode_one(S[r], w)
            differs_rev += bits(fwd) != bits(decode_one(S[r][::-1], w[::-1]))
            with np.errstate(invalid='ignore', over='ignore'):
                halves = np.float32(decode_one(S[r][:H // 2], w[:H // 2]) + decode_one(S[r][H // 2:], w[H // 2:]))
            differs_halves += bits(fwd) != bits(halves)
    assert differs_rev > 0 and differs_halves > 0


def header():
    return open(os.path.join(ROOT, 'include', 'ndcn_hip.h')).read()


def test_the_narrow_bit_in_header_and_binding():
    from ndcn_amd import _lib
    defs = {k: int(v) for k, v in re.findall(r'#define\s+NDCN_READOUT_(\w+)\s+(\d+)', header())}
    assert defs == {'FUSED': 1, 'STAGED': 2, 'FIXED': 4, 'NARROW': 8}
    assert _lib.READOUT_NARROW == 8
    assert (_lib.READOUT_FUSED, _lib.READOUT_STAGED, _lib.READOUT_FIXED) == (1, 2, 4)
    others = _lib.READOUT_FUSED | _lib.READOUT_STAGED | _lib.READOUT_FIXED
    assert _lib.READOUT_NARROW & others == 0 and bin(others).count('1') == 3


def test_the_abi_number_is_the_bindings():
    from ndcn_amd import _lib
    m = re.search(r'#define\s+NDCN_ABI_VERSION\s+(\d+)', header())
    assert m and int(m.group(1)) == _lib.ABI_VERSION
