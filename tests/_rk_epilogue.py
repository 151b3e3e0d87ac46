"""The Runge-Kutta epilogue of the fused right-hand sides restated in numpy float32 - what rhs_fused3.hip, rhs_fused2.hip (and its fp32
build), rhs_fused.hip, rhs_small.hip, spmm_rec.hip and spmm_wide_rk each carry a private copy of, as their comments cite the reference
(rk_common.py:45-60, 72-78; misc.py:22-25, 146-157).

TEST INFRASTRUCTURE: never imported by product code.  tests/test_rk_epilogue_host.py pins every function on hand-worked vectors.

Every operation below is ONE elementwise numpy float32 operation: one IEEE rounding per element, subnormals kept, overflow to +-Inf,
Inf - Inf and 0 * Inf = NaN.  Nothing is contracted (the kernels are built with fp contract off around this algebra) and nothing is a
reduction.  `kk` lists the stages in order, the NEW one (the K the launch forms) LAST; `cs` their coefficients in the same order.

The fused epilogues form the new stage's product FIRST and add the earlier stages' running sum to it (`u + s`); the stand-alone
kernels of rk.hip (the composed fallback of rhs.hip) start Python's sum() from 0 instead (tests/_aten_order.py: wsum).  The two
agree in every bit except the sign of a sum whose terms are all zeros: -0 products sum to -0 here and to +0 there."""
import numpy as np

F = np.float32


def f32(v):
    return np.asarray(v, dtype=np.float32)


def stage_sum(kk, cs, from_zero=False):
    """s = kk[-1] * cs[-1] first; u = kk[0] * cs[0], then u = u + kk[j] * cs[j] left to right over the earlier stages; the result is
    u + s, with no earlier stage s alone.  from_zero: the stand-alone kernels' form, (0 + kk[0] * cs[0]) + ... with the new stage as
    the last addend (rk.hip wsum1)."""
    assert len(kk) == len(cs) >= 1
    with np.errstate(all='ignore'):
        if from_zero:
            acc = F(0) + f32(kk[0]) * F(cs[0])
            for k, c in zip(kk[1:], cs[1:]):
                acc = acc + f32(k) * F(c)
            return acc
        s = f32(kk[-1]) * F(cs[-1])
        if len(kk) == 1:
            return s
        u = f32(kk[0]) * F(cs[0])
        for k, c in zip(kk[1:-1], cs[1:-1]):
            u = u + f32(k) * F(c)
        return u + s


def combine(y0, kk, cs, from_zero=False):
    """y_next = y0 + stage_sum (rk_common.py:51)"""
    with np.errstate(all='ignore'):
        return f32(y0) + stage_sum(kk, cs, from_zero)


def aux(kk, c2, from_zero=False):
    """y_aux: the same sum with the second coefficient set and without y0 (dopri5's partial error sum)"""
    return stage_sum(kk, c2, from_zero)


def rk4_stage(i, y0, kk, dt):
    """stage i = len(kk) - 1 of the 3/8-rule step (rk_common.py:72-78): the input of the next stage, i = 3: the step itself"""
    assert len(kk) == i + 1
    kk = [f32(k) for k in kk]
    dt = F(dt)
    with np.errstate(all='ignore'):
        if i == 0:
            s = (kk[0] * dt) / F(3)
        elif i == 1:
            s = (kk[0] / F(-3) + kk[1]) * dt
        elif i == 2:
            s = ((kk[0] - kk[1]) + kk[2]) * dt
        elif i == 3:
            s = (((kk[0] + kk[1] * F(3)) + kk[2] * F(3)) + kk[3]) * (dt / F(8))
        else:
            raise ValueError(i)
        return f32(y0) + s


def max_nan(a, b):
    """csrc/common.h max_nan = torch.max: the larger operand, a NaN on either side wins"""
    a, b = f32(a), f32(b)
    with np.errstate(all='ignore'):
        return np.where((a > b) | np.isnan(a), a, b)


def error_terms(y0, y1, kk, cs, rtol, atol, from_zero=False):
    """(the fp32 z * z terms widened to fp64, the count of non-finite y1): tol = atol + rtol * max_nan(|y0|, |y1|), z = stage_sum / tol
    (misc.py:146-157) - product, sum, quotient and square each rounded to fp32.  What the division yields at the edges: tol = +Inf
    (an infinite y0 or y1) gives z = +-0 for a finite sum and NaN for an infinite one; tol = 0 (atol = 0 and y0 = y1 = 0) gives
    z = +-Inf for a non-zero sum (the term is +Inf) and NaN for a zero sum; a NaN anywhere gives a NaN term."""
    with np.errstate(all='ignore'):
        s = stage_sum(kk, cs, from_zero)
        a1 = np.abs(f32(y1))
        tol = F(atol) + F(rtol) * max_nan(np.abs(f32(y0)), a1)
        z = s / tol
        zz = (z * z).astype(np.float64)
    return zz, int((~(a1 <= F(3.402823466e38))).sum())
