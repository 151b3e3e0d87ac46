"""The fp32 fma emulation of tests/_fma_chain.py against exact rational arithmetic (CPU only): 200 000+ adversarial cases -
cancellation, magnitudes far apart, exact and near halfway patterns (where rounding the fp64 sum again would tie wrongly), subnormal
results, signed zeros, Inf / NaN operands - and one short chain worked out by hand."""
from fractions import Fraction

import numpy as np

from _fma_chain import chain, chain_hub, fma32, hub_segments

F32_MAX_EXP = 128


def _round_f32(q):
    """Fraction -> nearest fp32 (ties to even), overflow to Inf; q != 0"""
    s = -1.0 if q < 0 else 1.0
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)                                   # subnormal range: quantum 2^-149
    quantum = Fraction(2) ** (e - 23)
    m = q / quantum
    fl = m.numerator // m.denominator
    rem = m - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    v = fl * quantum
    if v >= Fraction(2) ** F32_MAX_EXP:
        return np.float32(s * np.inf)
    return np.float32(s * float(v))


def _exact(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return np.float32(a * b + c)                     # Inf / NaN: IEEE rules, exact in fp64 (no finite rounding involved)
    q = Fraction(a) * Fraction(b) + Fraction(c)
    if q == 0:
        neg_p = (a * b == 0) and np.signbit(a) != np.signbit(b)
        return np.float32(-0.0 if (neg_p and np.signbit(c)) else 0.0)
    return _round_f32(q)


def _cases(n, seed=0):
    rng = np.random.RandomState(seed)
    k = np.arange(n) % 8
    a = (rng.randn(n) * 2.0 ** rng.randint(-40, 40, n)).astype(np.float32)
    b = (rng.randn(n) * 2.0 ** rng.randint(-40, 40, n)).astype(np.float32)
    ab = a.astype(np.float64) * b
    c = (rng.randn(n) * 2.0 ** rng.randint(-40, 40, n)).astype(np.float32)
    # 0: cancellation - c within 2^-20..2^-30 of -ab
    m = k == 0
    c[m] = (-ab[m] * (1 + rng.randn(m.sum()) * 2.0 ** -rng.randint(20, 31, m.sum()))).astype(np.float32)
    # 1: magnitudes up to 2^70 apart
    m = k == 1
    c[m] = (ab[m] * 2.0 ** rng.randint(-70, 71, m.sum())).astype(np.float32)
    # 2: exact halfway: c in [1, 2) * 2^e, a b = +-half an ulp of c (ties to even)
    m = k == 2
    cm = (1 + rng.randint(0, 1 << 23, m.sum()) * 2.0 ** -23) * 2.0 ** rng.randint(-100, 100, m.sum())
    c[m] = (cm * rng.choice([-1, 1], m.sum())).astype(np.float32)
    ec = np.floor(np.log2(np.abs(c[m].astype(np.float64))))
    a[m] = (2.0 ** (ec - 24)).astype(np.float32)
    b[m] = rng.choice([-1.0, 1.0], m.sum()).astype(np.float32)
    # 3: just off halfway by less than an fp64 ulp of c: a b = half ulp * (1 -+ 2^-46) - rounding the fp64 sum ties wrongly
    m = k == 3
    cm = (1 + rng.randint(0, 1 << 23, m.sum()) * 2.0 ** -23) * 2.0 ** rng.randint(-90, 90, m.sum())
    c[m] = (cm * rng.choice([-1, 1], m.sum())).astype(np.float32)
    ec = np.floor(np.log2(np.abs(c[m].astype(np.float64))))
    sgn = rng.choice([-1.0, 1.0], m.sum())
    a[m] = (2.0 ** (ec - 24) * (1 + 2.0 ** -23)).astype(np.float32)
    b[m] = (sgn * (1 - 2.0 ** -23)).astype(np.float32)
    # 4: subnormal results (products and sums below 2^-126), subnormal operands
    m = k == 4
    a[m] = (rng.randn(m.sum()) * 2.0 ** rng.randint(-75, -60, m.sum())).astype(np.float32)
    b[m] = (rng.randn(m.sum()) * 2.0 ** rng.randint(-75, -60, m.sum())).astype(np.float32)
    c[m] = (rng.randn(m.sum()) * 2.0 ** rng.randint(-149, -120, m.sum())).astype(np.float32)
    # 5: signed zeros in every position, exact zero sums
    m = np.nonzero(k == 5)[0]
    z = rng.randint(0, 4, m.size)
    a[m[z == 0]] = np.float32(-0.0)
    b[m[z == 1]] = np.float32(0.0)
    c[m[z == 2]] = np.where(rng.rand((z == 2).sum()) < 0.5, np.float32(0.0), np.float32(-0.0))
    exact_zero = m[z == 3]
    ez = exact_zero.size
    a[exact_zero] = rng.randn(ez).astype(np.float16).astype(np.float32) * np.float32(2.0) ** rng.randint(-20, 21, ez)  # 11-bit
    b[exact_zero] = rng.randn(ez).astype(np.float16).astype(np.float32) * np.float32(2.0) ** rng.randint(-20, 21, ez)  # mantissas
    c[exact_zero] = (-(a[exact_zero].astype(np.float64) * b[exact_zero])).astype(np.float32)
    both = m[z == 0]
    c[both[: both.size // 2]] = np.float32(-0.0)
    b[both[: both.size // 4]] = np.float32(3.0)
    # 6: Inf / NaN operands, overflow
    m = np.nonzero(k == 6)[0]
    spec = np.array([np.inf, -np.inf, np.nan, 0.0, 3e38, -3e38], np.float32)
    where = rng.randint(0, 3, m.size)
    pick = spec[rng.randint(0, spec.size, m.size)]
    a[m[where == 0]] = pick[where == 0]
    b[m[where == 1]] = pick[where == 1]
    c[m[where == 2]] = pick[where == 2]
    # 7: random with wide exponents (the rest of the set as generated)
    return a, b, c


def test_fma32_equals_exact_rounding():
    n = 200_000
    a, b, c = _cases(n)
    got = fma32(a, b, c)
    bad = []
    for i in range(n):
        want = _exact(a[i], b[i], c[i])
        g = got[i]
        same = (np.isnan(want) and np.isnan(g)) or (g.view(np.int32) == np.float32(want).view(np.int32))
        if not same:
            bad.append((i % 8, float(a[i]), float(b[i]), float(c[i]), float(g), float(want)))
    print('fma32: %d cases, %d mismatches' % (n, len(bad)))
    assert not bad, bad[:10]
    # the set reaches what it is meant to reach
    kinds = np.arange(n) % 8
    assert np.any((np.abs(got) < 2.0 ** -126) & (got != 0) & (kinds == 4))
    assert np.any(np.isnan(got)) and np.any(np.isinf(got)) and np.any(np.signbit(got) & (got == 0))
    with np.errstate(invalid='ignore', over='ignore'):
        naive = (a.astype(np.float64) * b + c).astype(np.float32)
    assert np.sum((naive.view(np.int32) != got.view(np.int32)) & (kinds == 3)) > 1000     # double rounding would have failed


def test_chain_by_hand():
    """acc = fma(v_j, x_j, acc) from +0: (1 + 2^-12)^2 rounds to 1 + 2^-11 (a tie, to even); the fma with -(1 + 2^-12) leaves its
    exact remainder -2^-24 (a separate product would have rounded it away); + 2^-30 * 1 is exact."""
    v = np.array([1 + 2.0 ** -12, -(1 + 2.0 ** -12), 2.0 ** -30], np.float32)
    x = np.array([[1 + 2.0 ** -12], [1 + 2.0 ** -12], [1.0]], np.float32)
    y = chain([0, 3], [0, 1, 2], v, x)
    assert y.shape == (1, 1) and y[0, 0] == np.float32(-(2.0 ** -24 - 2.0 ** -30))
    assert chain([0, 3], [0, 1, 2], v, x, alpha=-2.0)[0, 0] == np.float32(2.0 ** -23 - 2.0 ** -29)
    assert chain([0, 3], [0, 1, 2], v, x, relu=True)[0, 0] == 0.0
    # -0 stays under relu, NaN passes
    assert np.signbit(chain([0, 1], [0], np.float32([-1.0]), np.float32([[0.0]]), alpha=1.0, relu=True)[0, 0]) is np.False_
    nz = chain([0, 0], [], np.float32([]), np.float32([[1.0]]), alpha=-1.0, relu=True)[0, 0]
    assert nz == 0 and np.signbit(nz)
    assert np.isnan(chain([0, 1], [0], np.float32([1.0]), np.float32([[np.nan]]), relu=True)[0, 0])


def test_chain_equals_a_loop_and_hub_segments():
    """the ELL vectorisation against a plain per-element loop; the hub form with segments of 4 against the same loop per segment"""
    rng = np.random.RandomState(3)
    n, m, H = 23, 17, 3
    deg = rng.randint(0, 12, n)
    deg[5] = 0
    indptr = np.r_[0, np.cumsum(deg)]
    indices = rng.randint(0, m + 4, indptr[-1])
    data = rng.randn(indptr[-1]).astype(np.float32)
    X = rng.randn(m, H).astype(np.float32)
    Xh = rng.randn(4, H).astype(np.float32)
    Xall = np.concatenate([X, Xh])
    want = np.zeros((n, H), np.float32)
    for r in range(n):
        for j in range(indptr[r], indptr[r + 1]):
            want[r] = fma32(data[j], Xall[indices[j]], want[r])
    got = chain(indptr, indices, data, X, X_halo=Xh, n_own=m, alpha=-2.5, relu=True)
    assert np.array_equal(got.view(np.int32), np.where((want * np.float32(-2.5)) < 0, np.float32(0), want * np.float32(-2.5)).view(np.int32))
    sel = indices < m
    want_hub = np.zeros((n, H), np.float32)
    hubs, starts, lens, nseg = hub_segments(indptr, 6, seg=4)
    assert hubs.size > 0 and np.all(lens <= 4)
    idx2, dat2 = np.where(sel, indices, 0), np.where(sel, data, 0).astype(np.float32)
    for r in range(n):
        if r in hubs:
            acc = np.zeros(H, np.float32)
            for s0 in range(indptr[r], indptr[r + 1], 4):
                part = np.zeros(H, np.float32)
                for j in range(s0, min(s0 + 4, indptr[r + 1])):
                    part = fma32(dat2[j], X[idx2[j]], part)
                acc = fma32(np.float32(1), part, acc)
            want_hub[r] = fma32(np.float32(1), acc, np.zeros(H, np.float32))
        else:
            for j in range(indptr[r], indptr[r + 1]):
                want_hub[r] = fma32(dat2[j], X[idx2[j]], want_hub[r])
    got_hub = chain_hub(indptr, idx2, dat2, X, 6, seg=4)
    assert np.array_equal(got_hub.view(np.int32), want_hub.view(np.int32))
