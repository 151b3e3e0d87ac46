"""The SpMM kernels' arithmetic restated in numpy (DESIGN.md sections 2 and 4): per output element one correctly rounded fp32 fma
per stored entry, in stored order, starting from +0; then acc * alpha (one fp32 rounding) and, with relu, `v < 0 ? 0 : v`
(csrc/common.h relu_nan: a NaN passes, -0 stays).  The long-row (hub) plan sums a hub row as <= 256-entry segment chains, then a
chain over its segments (csrc/csr_plan.hip build_hub_plan, csrc/spmm.hip spmm_f32).

fma32 is exact: the product of two fp32 values is exact in fp64 (48 significant bits); the fp64 sum is corrected to round to odd
with TwoSum (sticky bit), and a round-to-odd value at 53 bits rounds to any format of <= 51 bits exactly as the real number
would (subnormal fp32 results included).  tests/test_fma_chain.py pins it against Fraction arithmetic."""
import numpy as np

U = 2.0 ** -24


def fma32(a, b, c):
    """correctly rounded fp32 fma(a, b, c), elementwise with broadcasting"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid='ignore', over='ignore'):
        p = a * b                                        # exact
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                    # TwoSum: s + e == p + c exactly (finite s)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (e != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def finish(acc, alpha=1.0, relu=False):
    """vfinish / the wide and record kernels' epilogue: acc * alpha, then relu_nan"""
    with np.errstate(invalid='ignore', over='ignore'):
        out = (np.asarray(acc, np.float32) * np.float32(alpha)).astype(np.float32)
    if relu:
        out = np.where(out < 0, np.float32(0.0), out).astype(np.float32)
    return out


def chain(indptr, indices, data, X, X_halo=None, n_own=None, alpha=1.0, relu=False, rows=None):
    """Y[rows] of Y = finish(A X) as the sequential fma chain, vectorised in ELL form: step j applies entry j of every row that
    has one to all H columns at once.  Columns >= n_own (default: X's rows) address X_halo[c - n_own]."""
    indptr = np.asarray(indptr, np.int64)
    indices = np.asarray(indices, np.int64)
    data = np.asarray(data, np.float32)
    X = np.asarray(X, np.float32)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    n_own = X.shape[0] if n_own is None else int(n_own)
    if X_halo is not None:
        X_halo = np.asarray(X_halo, np.float32)
        Xall = np.concatenate([X[:n_own], X_halo])
    else:
        Xall = X
    rows = np.arange(indptr.size - 1) if rows is None else np.asarray(rows, np.int64)
    H = X.shape[1]
    deg = indptr[rows + 1] - indptr[rows]
    order = np.argsort(-deg, kind='stable')
    sd, start = deg[order], indptr[rows][order]
    acc = np.zeros((rows.size, H), np.float32)
    neg = -sd
    for j in range(int(sd.max()) if sd.size else 0):
        k = int(np.searchsorted(neg, -j, side='left'))   # rows with more than j entries
        e = start[:k] + j
        acc[:k] = fma32(data[e][:, None], Xall[indices[e]], acc[:k])
    out = np.empty_like(acc)
    out[order] = acc
    return finish(out, alpha, relu)


def hub_segments(indptr, threshold, seg=256):
    """build_hub_plan's rules: hub rows are those with more than `threshold` entries; each is cut into <= seg-entry segments in
    stored order.  Returns (hub rows, segment start offsets into the operator's arrays, segment lengths, segments per hub)."""
    indptr = np.asarray(indptr, np.int64)
    deg = indptr[1:] - indptr[:-1]
    hubs = np.nonzero(deg > threshold)[0]
    nseg = (deg[hubs] + seg - 1) // seg
    starts = np.concatenate([indptr[r] + seg * np.arange(k) for r, k in zip(hubs, nseg)]) if hubs.size else np.zeros(0, np.int64)
    ends = np.concatenate([np.minimum(indptr[r] + seg * np.arange(1, k + 1), indptr[r + 1]) for r, k in zip(hubs, nseg)]) \
        if hubs.size else np.zeros(0, np.int64)
    return hubs, starts, ends - starts, nseg


def chain_hub(indptr, indices, data, X, threshold, alpha=1.0, relu=False, seg=256):
    """Y = finish(A X) through the long-row plan: light rows as `chain`; hub row h as S_h = chain over its segments' chains (the
    combine operator: entries (segment, 1.0) in order), then read as the light operator's single entry (n_cols + h, 1.0)."""
    indptr = np.asarray(indptr, np.int64)
    indices = np.asarray(indices, np.int64)
    data = np.asarray(data, np.float32)
    Y = chain(indptr, indices, data, X, alpha=alpha, relu=relu)
    hubs, starts, lens, nseg = hub_segments(indptr, threshold, seg)
    if hubs.size == 0:
        return Y
    take = np.concatenate([np.arange(s, s + n) for s, n in zip(starts, lens)])
    seg_ptr = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=seg_ptr[1:])
    Sseg = chain(seg_ptr, indices[take], data[take], X)
    cmb_ptr = np.zeros(hubs.size + 1, np.int64)
    np.cumsum(nseg, out=cmb_ptr[1:])
    S = chain(cmb_ptr, np.arange(lens.size), np.ones(lens.size, np.float32), Sseg)
    one = np.arange(hubs.size + 1, dtype=np.int64)
    Y[hubs] = chain(one, np.arange(hubs.size), np.ones(hubs.size, np.float32), S, alpha=alpha, relu=relu)
    return Y


def row_terms(indptr, threshold=None, seg=256):
    """d of the error bound per row: the row length, and for hub rows d + its number of segments"""
    indptr = np.asarray(indptr, np.int64)
    d = (indptr[1:] - indptr[:-1]).astype(np.float64)
    if threshold is not None:
        hubs, _, _, nseg = hub_segments(indptr, threshold, seg)
        d[hubs] += nseg
    return d


# ---- the float64 bounds the GPU tests hold the kernels to, stated once (u = U = 2^-24; `mag` is the same expression on magnitudes)
def spmm_bound(indptr, mag, alpha=1.0, threshold=None):
    """|alpha (A X) - float64| per element: a chain of d fmas and the product with alpha, each rounded once, plus the subnormal floor
    (tests/test_gpu_spmm_routes.py holds every route to it); mag = |A| |X| in float64, one row of d per row of mag"""
    d = row_terms(indptr, threshold)[:, None]
    return 1.01 * (abs(float(alpha)) * ((d + 1) * U * mag + d * 2.0 ** -150) + 2.0 ** -150)


def dot_bound(k, mag):
    """a float32 inner product of k terms plus a bias, in any order: (k + 2) u on the magnitudes (the forward bound of
    tests/test_gpu_linear_routes.py); mag = |S| |W|^T + |b|"""
    return (k + 2) * U * mag


def sum_bound(n_terms, mag):
    """y0 + ((c_0 k_0 + c_1 k_1) + ...): one rounding per product and per sum, n_terms + 1 roundings on any path, second order covered
    by the 1.01 (the combine / pull bound of tests/test_gpu_reverse_routes.py); mag = |y0| + sum |c_j k_j|"""
    return 1.01 * (n_terms + 1) * U * mag
