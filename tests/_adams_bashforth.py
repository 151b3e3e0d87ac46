"""The explicit_adams method (the reference's AdamsBashforth, torchdiffeq/_impl/fixed_adams.py:151-211) restated in numpy: the
derivation of its coefficients from exact rationals, the arithmetic of one step to the bit, and the solve around them.  Independent
of the package (tests compare the package, the library and the golden fixtures with it).

A step of order k from (t, y) with size dt, f_0 the evaluation at (t, y) and f_1 .. f_{k-1} the ones before it:
    a_i = float32((1 / div) * c_i)      the product in Python doubles; beta_i = c_i / div, div the least common denominator
    p_i = a_i * f_i                     rounded to float32
    s   = ((0 + p_0) + p_1) + ...       left to right, every sum rounded; the start is an exact zero: a lone -0.0 becomes +0.0
    y1  = y + dt * s                    product and sum rounded on their own
with beta_i = integral_0^1 prod_{j != i} (u + j) / (j - i) du.  Below three evaluations the step is RK4 by the 3/8 rule
(rk_common.py:72-78) with k1 = f_0.
"""
import collections
import fractions
import math

import numpy as np

f32 = np.float32
MIN_TERMS, MAX_ORDER = 3, 12


def betas(order):
    """beta_0 .. beta_{order-1} as exact rationals, newest evaluation first"""
    out = []
    for i in range(order):
        poly = [fractions.Fraction(1)]                       # prod_{j != i} (u + j), lowest power first
        den = fractions.Fraction(1)
        for j in range(order):
            if j == i:
                continue
            shifted = [fractions.Fraction(0)] + poly          # u * poly
            poly = [shifted[m] + (j * poly[m] if m < len(poly) else 0) for m in range(len(shifted))]
            den *= j - i
        out.append(sum(c / (m + 1) for m, c in enumerate(poly)) / den)
    return out


def integer_form(order):
    """([c_i], div) with beta_i = c_i / div and div the least common denominator"""
    bs = betas(order)
    div = 1
    for b in bs:
        div = div * b.denominator // math.gcd(div, b.denominator)
    cs = [b * div for b in bs]
    assert all(c.denominator == 1 for c in cs)
    return [int(c) for c in cs], div


def weights(order):
    cs, div = integer_form(order)
    return [f32((1 / div) * c) for c in cs]


def ab_step(y, fs, a, dt):
    """One step, bit for bit: y, fs[i] float32 arrays of one shape, a[i] float32 scalars, dt a float32 scalar."""
    y = np.asarray(y, dtype=f32)
    dt = f32(dt)
    with np.errstate(all='ignore'):
        s = (f32(0) + (f32(a[0]) * np.asarray(fs[0], dtype=f32)).astype(f32)).astype(f32)
        for ai, fi in zip(a[1:], fs[1:]):
            s = (s + (f32(ai) * np.asarray(fi, dtype=f32)).astype(f32)).astype(f32)
        return (y + (dt * s).astype(f32)).astype(f32)


def rk4_step(f, y, dt, k1):
    """rk_common.py:72-78 + solvers.py:92 in float32 (autonomous f)"""
    dt = f32(dt)
    k2 = f((y + dt * k1 / f32(3)).astype(f32))
    k3 = f((y + dt * (k1 / f32(-3) + k2)).astype(f32))
    k4 = f((y + dt * (k1 - k2 + k3)).astype(f32))
    return (y + (k1 + f32(3) * k2 + f32(3) * k3 + k4) * (dt / f32(8))).astype(f32)


def grid_of(t, step_size=None):
    """solvers.py:55-68 in float32: t itself, or t[0] + arange(ceil((t[-1] - t[0]) / h + 1)) * h with the last point clamped"""
    t = np.asarray(t, dtype=f32)
    if step_size is None:
        return t
    h = f32(step_size)
    n = int(np.ceil(f32(f32(f32(t[-1] - t[0]) / h) + f32(1))))
    g = (np.arange(n, dtype=f32) * h + t[0]).astype(f32)
    if g[-1] > t[-1]:
        g[-1] = t[-1]
    assert g[0] == t[0] and g[-1] == t[-1]
    return g


def solve(f, y0, t, max_order=MAX_ORDER, step_size=None):
    """(trajectory at the ticks, evaluations, states after every grid step).  f: float32 array -> float32 array (autonomous).  Ticks
    are reported as solvers.py:92-108 does after y0 was overwritten with y1: the state at the end of the first step that reaches
    the tick - through y1 + ((y1 - y1) / dt) * (t - t0) where the tick lies strictly inside the step."""
    t = np.asarray(t, dtype=f32)
    grid = grid_of(t, step_size)
    max_order = int(min(max_order, MAX_ORDER))
    hist = collections.deque(maxlen=max_order - 1)
    y = np.asarray(y0, dtype=f32)
    nfe = 0

    def fn(x):
        nonlocal nfe
        nfe += 1
        return np.asarray(f(x), dtype=f32)

    sol, states, j = [y], [], 1
    for i in range(len(grid) - 1):
        t0, t1 = grid[i], grid[i + 1]
        dt = f32(t1 - t0)
        hist.appendleft(fn(y))
        order = min(len(hist), max_order - 1)
        if order < MIN_TERMS:
            y = rk4_step(fn, y, dt, hist[0])
        else:
            y = ab_step(y, list(hist), weights(order), dt)
        states.append(y)
        while j < len(t) and t1 >= t[j]:
            if t[j] == t0 or t[j] == t1:
                sol.append(y)
            else:
                with np.errstate(all='ignore'):
                    sol.append((y + ((y - y) / dt) * f32(t[j] - t0)).astype(f32))
            j += 1
    return np.stack(sol), nfe, states
