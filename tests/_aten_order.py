"""ATen's SINGLE-THREAD float32 summation orders as plain numpy float32 arithmetic - the contract of rk_error_aten_kernel and
scaled_sumsq_aten_kernel (ndcn_amd/csrc/rk.hip), stated without a torch reduction so that the GPU tests have an oracle that depends on
neither the device nor a thread pool.  tests/test_aten_order_host.py pins both models against torch.sum / torch.norm under one thread.

TEST INFRASTRUCTURE: never imported by product code.

Every array operation below is an ELEMENTWISE numpy float32 operation (one IEEE rounding per element and operation); nothing calls a
numpy or torch reduction, whose own summation order (pairwise, threaded) would otherwise leak into the oracle.  Where a chain is serial
in the contract it is a Python loop here; independent chains (the 32 running sums, the runs of one cascade level) are the vector axis.
"""
import numpy as np

F = np.float32


def f32(v):
    return np.asarray(v, dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------ element formers
def wsum(ks, cs):
    """sum_j c_j k_j, left to right, every product and sum rounded on its own (misc.py:22-25; rk.hip wsum1 / wsum4)"""
    with np.errstate(all='ignore'):
        acc = F(0) + F(cs[0]) * f32(ks[0])           # Python's sum() starts from 0: a -0 first product becomes +0
        for c, k in zip(cs[1:], ks[1:]):
            acc = acc + F(c) * f32(k)
    return acc


def max_nan(a, b):
    """torch.max(a, b): a NaN in either operand gives NaN (np.maximum propagates, np.fmax would not)"""
    return np.maximum(f32(a), f32(b))


def ratio_sq(e, y0, y1, rtol, atol):
    """misc.py:151-156: tol = atol + rtol max(|y0|, |y1|); r = e / tol; r r - four roundings"""
    with np.errstate(all='ignore'):
        tol = F(atol) + F(rtol) * max_nan(np.abs(f32(y0)), np.abs(f32(y1)))
        r = f32(e) / tol
        return r * r


def error_elements(y0, y1, ks, cs, rtol, atol):
    """the addends r^2 of ndcn_rk_error_f32"""
    with np.errstate(all='ignore'):
        return ratio_sq(wsum(ks, cs), y0, y1, rtol, atol)


def scaled_q(a, b, y, rtol, atol):
    """misc.py:121-138: q = (a - b) / (atol + |y| rtol); b None: a / scale, no subtraction at all"""
    with np.errstate(all='ignore'):
        scale = F(atol) + np.abs(f32(y)) * F(rtol)
        return (f32(a) / scale) if b is None else ((f32(a) - f32(b)) / scale)


def nonfinite_count(x):
    return int((~np.isfinite(f32(x))).sum())        # a count of booleans: integer arithmetic, no float summation order


# ------------------------------------------------------------------------------------------------------------------ the cascade sum
def ceil_log2(x):
    """ATen's utils::CeilLog2: 1 for x <= 2"""
    if x <= 2:
        return 1
    lg = 0
    while (1 << lg) < x:
        lg += 1
    return lg


def level_step(n):
    return 1 << max(4, ceil_log2((n // 8) // 4) // 4)


def _runs(rows, step):
    """rows (m, 32): the addends one cascade level receives, in order.  Whole runs of `step` addends are summed from zero one addend
    at a time (the runs are independent: the vector axis) -> (m // step, 32); the trailing partial run -> (32,), also from zero."""
    m = rows.shape[0]
    g = m // step
    full = rows[:g * step].reshape(g, step, 32)
    acc = np.zeros((g, 32), F)
    for j in range(step):
        acc = acc + full[:, j, :]
    rem = np.zeros(32, F)
    for r in rows[g * step:]:
        rem = rem + r
    return acc, rem


def cascade_sum(v):
    """ATen's float32 `sum` of a contiguous row on one thread (SumKernel.cpp, 8-lane vectors): 32 running sums - sum (k, w) owns
    elements 32 i + 8 k + w - kept in 4 cascade levels; level 0 takes the elements and is added into level 1 and cleared after every
    `step` = 2^max(4, ceil_log2(n / 32) / 4) of them, level 1 into level 2 after step^2, level 2 into level 3 after step^3; a trailing
    partial run stays where it is.  Then levels 1, 2, 3 are added into level 0, the left-over 8-lane vectors (0..3 of them) into
    interleave slot 0, slots 1..3 into slot 0, and finally, starting from 0: the n % 8 tail elements, then the 8 lanes, left to right."""
    v = f32(v).ravel()
    n = v.size
    with np.errstate(all='ignore'):
        nv = n // 8
        size_ilp = nv // 4
        n_main = size_ilp * 32
        step = level_step(n)
        s0, r0 = _runs(v[:n_main].reshape(size_ilp, 32), step)
        s1, r1 = _runs(s0, step)
        s2, r2 = _runs(s1, step)
        a3 = np.zeros(32, F)
        for r in s2:                                   # level 3 is never cleared
            a3 = a3 + r
        a0 = ((r0 + r1) + r2) + a3
        left_vecs = nv - 4 * size_ilp
        slot0 = a0[:8]
        for u in range(left_vecs):
            slot0 = slot0 + v[n_main + 8 * u:n_main + 8 * u + 8]
        p = ((slot0 + a0[8:16]) + a0[16:24]) + a0[24:32]
        s = F(0)
        for x in v[n_main + 8 * left_vecs:]:
            s = F(s + x)
        for w in range(8):
            s = F(s + p[w])
    return F(s)


def cascade_sum_serial(v):
    """the same order as ONE loop over the 32-element steps with the hand-over conditions spelled out as in SumKernel.cpp
    (slow: the host test uses it to check the vectorised form above at the level hand-overs)"""
    v = f32(v).ravel()
    n = v.size
    with np.errstate(all='ignore'):
        nv = n // 8
        size = nv // 4
        p_ = max(4, ceil_log2(size) // 4)
        step, mask = 1 << p_, (1 << p_) - 1
        acc = np.zeros((4, 32), F)
        i = 0
        while i + step <= size:
            for _ in range(step):
                acc[0] = acc[0] + v[32 * i:32 * i + 32]
                i += 1
            for j in range(1, 4):
                acc[j] = acc[j] + acc[j - 1]
                acc[j - 1] = 0
                if i & (mask << (j * p_)):
                    break
        while i < size:
            acc[0] = acc[0] + v[32 * i:32 * i + 32]
            i += 1
        for j in range(1, 4):
            acc[0] = acc[0] + acc[j]
        a0 = acc[0].copy()
        n_main = 32 * size
        slot0 = a0[:8]
        for u in range(nv - 4 * size):
            slot0 = slot0 + v[n_main + 8 * u:n_main + 8 * u + 8]
        p = ((slot0 + a0[8:16]) + a0[16:24]) + a0[24:32]
        s = F(0)
        for x in v[8 * nv:]:
            s = F(s + x)
        for w in range(8):
            s = F(s + p[w])
    return F(s)


# ------------------------------------------------------------------------------------------------------------------ the norm's order
def _fma32(x, y, z):
    """the correctly rounded fp32 fma of tests/_fma_chain.py (pinned against rational arithmetic by tests/test_fma_chain.py)"""
    from _fma_chain import fma32
    return fma32(x, y, z)


_TIE = np.int64(0x10000000)
_LOW29 = np.int64(0x1fffffff)


def lane8_fma_sumsq(q):
    """ATen's float32 `norm` (p = 2) before the square root: EIGHT running sums - lane j owns elements j, j + 8, j + 16, ... and takes
    acc_j = fma(q, q, acc_j) in index order - added up left to right, then the n % 8 tail elements with fma.  One exception, measured
    against torch 2.10.0 (tests/test_aten_order_host.py: 400 random vectors per tail length, every fused / unfused assignment of the
    tail tried, exactly one fits all): the build's compiler ran the tail loop `acc += x * x` four elements at a time with an in-order
    reduction, so a tail of 4..7 elements adds its FIRST FOUR as separately rounded products and only the rest by fma."""
    q = f32(q).ravel()
    n8 = q.size - q.size % 8
    with np.errstate(all='ignore'):
        rows = q[:n8].reshape(-1, 8)
        sq = rows.astype(np.float64) ** 2                           # exact products
        acc = np.zeros(8, F)
        for r, x in zip(sq, rows):
            # a float64 product-and-add rounded once to float32; the float64 addition has rounded to 53 bits first, which can only
            # matter when that sum sits exactly on a float32 tie (its low 29 bits 1000...0; normal float32 results, which sums
            # of these squares are): then the exact fma decides
            s64 = r + acc.astype(np.float64)
            acc = _fma32(x, x, acc) if ((s64.view(np.int64) & _LOW29) == _TIE).any() else s64.astype(F)
        s = acc[0]
        for j in range(1, 8):
            s = F(s + acc[j])
        tail = q[n8:]
        for j, x in enumerate(tail):
            s = F(s + F(x * x)) if (tail.size >= 4 and j < 4) else _fma32(x, x, s)
    return F(s)


# ------------------------------------------------------------------------------------------------------------------ the sizes under test
# the left-over vectors (0..3) and the n % 8 tail at every small n; the 2048-element double-buffer edges of the kernels (2048, 4096,
# 8192); the level hand-overs of the cascade at 16 steps (512 elements), 256 steps (8192) and 4096 steps (131072), each with a partial
# trailing run on either side; the README-sized records (8000, 173312) and the default bound 2^18
EDGE_OFFSETS = (-33, -32, -31, -8, -1, 0, 1, 8, 31, 32, 33)
ATEN_SIZES = sorted(set(list(range(1, 301)) +
                        [c + d for c in (512, 2048, 4096, 8192, 131072) for d in EDGE_OFFSETS] +
                        [8000, 16401, 65536, 65569, 173312, (1 << 18) - 1, 1 << 18]))
ATEN_SIZES_RAISED_BOUND = [(1 << 20) + 37, (1 << 22) + 4105, 1 << 24]          # with ndcn_set_aten_norm_max(1 << 24)
