"""The three passes of csrc/adams_vc.hip restated in numpy float32 from core.Adams.step (adams.py:62-170): every product and every
sum rounded on its own, sums left to right from +0 - what step's sequence of ops.scale / ops.combine / ops.error computes, written
without that sequence.  No torch, no kernel.

  e_0 = phi_0,  e_j = fl(beta_j * phi_j)             the explicit phi (ops.scale)
  a - b  =  a + (0 + (-1) * b)                       ops.combine(a, [b], [-1])
"""
import numpy as np

f32 = np.float32
ZERO, NEG1 = f32(0.0), f32(-1.0)


def explicit(phis, betas, j):
    return phis[0] if j == 0 else f32(betas[j]) * phis[j]


def minus(a, b):
    return a + (ZERO + NEG1 * b)


def predict(y, phis, betas, cs, order):
    """p_next = y + ((0 + c_0 e_0) + c_1 e_1 + ...), max(1, order - 1) terms"""
    m = max(1, order - 1)
    with np.errstate(all='ignore'):
        acc = ZERO + f32(cs[0]) * explicit(phis, betas, 0)
        for j in range(1, m):
            acc = acc + f32(cs[j]) * explicit(phis, betas, j)
        return y + acc


def ratio_sq(e, a, b, rtol, atol):
    """misc.py:151-156, float32; torch.max propagates NaN, as np.maximum does"""
    tol = f32(atol) + f32(rtol) * np.maximum(np.abs(a), np.abs(b))
    r = e / tol
    return r * r


def correct(nf, phis, betas, order, p_next, y0, c_corr, coefs, rtol, atol):
    """(y_next, [r^2 array of sum q, or None where coefs[q] is None]); sum 0 and 3 weigh ip_order, sum 1 ip_{order-1}, sum 2 ip_{order-2}"""
    with np.errstate(all='ignore'):
        ip = [nf]
        for j in range(1, order + 1):
            ip.append(minus(ip[j - 1], explicit(phis, betas, j - 1)))
        y_next = p_next + (ZERO + f32(c_corr) * ip[order - 1])
        link = [order, order - 1, order - 2, order]
        r2 = [None if coefs[q] is None else ratio_sq(ZERO + f32(coefs[q]) * ip[link[q]], y0, y_next, rtol, atol) for q in range(4)]
    return y_next, r2


def update(nf2, phis, betas, order, n_out):
    """[nf2, nf2 - e_0, (nf2 - e_0) - e_1, ...]: n_out panels"""
    with np.errstate(all='ignore'):
        out = [nf2]
        for j in range(1, n_out):
            out.append(minus(out[j - 1], explicit(phis, betas, j - 1)))
    return out
