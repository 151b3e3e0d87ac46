"""Row-wise L1 normalisation and its reverse restated in float64 (numpy only), with the float32 error bounds the device kernels of
csrc/rownorm.hip are held to.  tests/test_rownorm_host.py pins this file to double-precision torch autograd and to the reference's
recorded output; tests/test_gpu_rownorm.py holds the kernels to it.

    forward   s = sum_j |x_j|,  den = max(s, eps),  y_j = x_j / den, infinite y_j replaced by 0
    reverse   gm_j = g_j where y_j was not replaced,  T = sum_i gm_i x_i
              gx_j = gm_j / den - sign(x_j) T / den^2     the second term only where s >= eps (the clamp passes no gradient), sign(0) = 0

eps is the float32 value of 1e-12, what F.normalize(X.float(), 1, 1) clamps with.  A NaN in a row makes s, den and with them the whole
row NaN (clamp_min passes a NaN on), in both directions; an infinite entry makes den infinite, the finite entries 0 and that entry
inf / inf = NaN.  With den >= every |x_j| no quotient of finite operands is infinite, so the replacement by 0 is live only in float32,
where the sum of finite entries can overflow - and then x_j / inf is 0 already.

Float32 model, u = 2^-24 (round to nearest), d = 2^-149 (the smallest denormal); first-order terms are derived, the constants carry a
margin for the second-order ones ((1 + H u)^3 - 1 <= 3 H u (1 + 4e-4) for H <= 2050):

  * |x_j| is exact.  A float32 sum of H non-negative terms in ANY order and grouping (lane partial sums, the butterfly across the wave)
    is s (1 + a), |a| <= (H - 1) u.  max(., eps) is exact and monotone, so den' = den (1 + a') with |a'| <= (H - 1) u as well, also
    where the float32 and the float64 run disagree about which side of the clamp they are on.
"""
import numpy as np

U = 2.0 ** -24
DENORMAL = 2.0 ** -149
EPS = float(np.float32(1e-12))


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _den(X):
    s = np.abs(X).sum(axis=1, keepdims=True)
    with np.errstate(invalid='ignore'):
        return s, np.maximum(s, EPS)                 # np.maximum passes a NaN on, like clamp_min


def forward(X):
    X = _f64(X)
    _, den = _den(X)
    with np.errstate(invalid='ignore', over='ignore'):
        y = X / den
    y[np.isinf(y)] = 0.0
    return y


def vjp(G, X):
    G, X = _f64(G), _f64(X)
    s, den = _den(X)
    with np.errstate(invalid='ignore', over='ignore'):
        gm = np.where(np.isinf(X / den), 0.0, G)
        T = (gm * X).sum(axis=1, keepdims=True)
        second = np.sign(X) * (T / (den * den))      # np.sign(0) = 0, np.sign(nan) = nan
        # s >= eps is False for a NaN s, but there den is NaN and the first term is already NaN
        return gm / den - np.where(s >= EPS, second, 0.0)


def forward_bound(X):
    """|y_kernel - y| <= (H + 2) u |y| + d, element by element.

    y' = fl(x / den') = x / (den (1 + a')) * (1 + e), |e| <= u (the division is correctly rounded), so the relative error is
    (H - 1) u + u = H u to first order; (H + 2) u covers the second-order terms.  Where the quotient is a denormal the rounding is
    absolute instead: at most d."""
    X = _f64(X)
    return (X.shape[1] + 2) * U * np.abs(forward(X)) + DENORMAL


def vjp_bound(G, X):
    """|gx_kernel - gx| <= u [ (H + 3) |g_j| / den + (3 H + 6) P / den^2 ] + H d / den^2 + 2 d,   P = sum_i |g_i x_i|,
    the P terms only where the second term applies (s >= eps).

    first term    fl(g / den'): (H - 1) u from den', u from the division: H u |g_j| / den
    T             every product fl(g_i x_i) carries u (or, where it is a denormal, d: H d in the sum), the float32 sum of H terms in
                  any order (H - 1) u of sum |g_i x_i|: |T' - T| <= H u P + H d       (a fused multiply-add only removes roundings)
    den' * den'   2 (H - 1) u from den', u from the product; the division T' / (den' den') another u.  With |T| <= P:
                  |t' - T / den^2| <= (H + 2 (H - 1) + 2) u P / den^2 + H d / den^2 = 3 H u P / den^2 + H d / den^2
    difference    fl(a - sign t) carries u of the result, at most u (|g_j| / den + P / den^2)
    in all        u [ (H + 1) |g_j| / den + (3 H + 1) P / den^2 ] to first order; (H + 3) and (3 H + 6) cover the second-order terms.  A
                  quotient or a difference that lands in the denormals is rounded absolutely: 2 d covers the two that reach the
                  result.  den^2 >= 1e-24 never underflows; den <= 1e15 (the test's range) keeps it from overflowing."""
    G, X = _f64(G), _f64(X)
    H = X.shape[1]
    s, den = _den(X)
    with np.errstate(invalid='ignore', over='ignore'):
        P = np.where(s >= EPS, np.abs(G * X).sum(axis=1, keepdims=True), 0.0)
        tail = np.where(s >= EPS, H * DENORMAL / (den * den), 0.0)
        return U * ((H + 3) * np.abs(G) / den + (3 * H + 6) * P / (den * den)) + tail + 2 * DENORMAL


# ------------------------------------------------------------------------------------------------ the special rows
SPECIAL = ('zeros', 'signed_zeros', 'clamped', 'not_clamped', 'denormal', 'one_hot', 'negative', 'one_zero', 'huge', 'nan', 'pos_inf',
           'neg_inf')
NONFINITE = ('nan', 'pos_inf', 'neg_inf')


def panel(n_rows, H, seed):
    """(X, index): float32 random normal rows with the special rows planted at index[name] (as many of them as n_rows holds, in the
    order of SPECIAL rotated by the seed so that small panels see all of them over the seeds).  Every finite row's L1 norm is at most
    1e15."""
    rng = np.random.RandomState(seed)
    X = rng.normal(0, 1, (n_rows, H)).astype(np.float32)
    order = list(SPECIAL[seed % len(SPECIAL):] + SPECIAL[:seed % len(SPECIAL)])
    slots = rng.permutation(n_rows)[:len(order)]
    index = {}
    for name, r in zip(order, slots.tolist()):
        j = int(rng.randint(H))
        mag = np.abs(X[r]) + np.float32(0.1)
        if name == 'zeros':
            X[r] = 0.0
        elif name == 'signed_zeros':
            X[r] = np.where(np.arange(H) % 2 == 0, np.float32(0.0), np.float32(-0.0))
        elif name == 'clamped':
            X[r] = (X[r].astype(np.float64) * (1e-13 / np.abs(X[r]).astype(np.float64).sum())).astype(np.float32)
        elif name == 'not_clamped':
            X[r] = (X[r].astype(np.float64) * (1e-11 / np.abs(X[r]).astype(np.float64).sum())).astype(np.float32)
        elif name == 'denormal':
            X[r] = (np.sign(X[r]) * rng.randint(1, 1 << 20, H)).astype(np.float64) * DENORMAL
        elif name == 'one_hot':
            X[r] = 0.0
            X[r, j] = -2.5 if seed % 2 else 2.5
        elif name == 'negative':
            X[r] = -mag
        elif name == 'one_zero':
            X[r] = np.where(X[r] == 0, np.float32(1.0), X[r])
            if H > 1:
                X[r, j] = 0.0
        elif name == 'huge':
            X[r] = np.sign(X[r] + np.float32(1e-30)) * np.float32(9e14 / H)
        elif name == 'nan':
            X[r, j] = np.nan
        elif name == 'pos_inf':
            X[r, j] = np.inf
        elif name == 'neg_inf':
            X[r, j] = -np.inf
        index[name] = (r, j)
    return X, index
