"""The fixed_adams method (the reference's AdamsBashforthMoulton, torchdiffeq/_impl/fixed_adams.py:151-205) restated in numpy: the
derivation of the Adams-Moulton coefficients from exact rationals, the arithmetic of the predictor and of one corrector pass to the bit,
the convergence test and the solve around them.  Independent of the package; the Bashforth half comes from _adams_bashforth.

A step from (t, y) of size dt that holds n >= 3 evaluations f_0 (at t) .. f_{n-1}:
    dy    = dt * (((0 + a_0 f_0) + a_1 f_1) + ...)          a_i: the Adams-Bashforth weights of order n
    delta = dt * (((0 + w_1 f_0) + w_2 f_1) + ...)          w_i = float32((1 / div) * m_i), mu_i = m_i / div the Adams-Moulton
                                                            coefficients over the n + 1 points t + dt, t, t - dt, ..
    up to max_iters times:   f = func(y + dy);   dy' = c0 * f + delta,  c0 = float32(dt) * float32(m_0 / div);
                             converged when EVERY element has |dy - dy'| < atol + rtol * max(|dy|, |dy'|) (float32, strict);  dy = dy'
    y1 = y + dy;  a step that did not converge drops its oldest evaluation
with mu_i = integral_0^1 prod_{j != i} (u + j - 1) / (j - i) du.
"""
import collections
import fractions
import math

import numpy as np

import _adams_bashforth as ab

f32 = np.float32
MAX_ITERS = 4
WARNING = 'Warning: Functional iteration did not converge. Solution may be incorrect.'


def mus(n):
    """mu_0 .. mu_n of the Adams-Moulton formula over n + 1 points (n evaluations held), the point at the step's end first"""
    out = []
    for i in range(n + 1):
        nodes = [1 - j for j in range(n + 1) if j != i]       # the other points, in units of dt, the step being [0, 1]
        poly = [fractions.Fraction(1)]                        # prod (u - node), lowest power first
        den = fractions.Fraction(1)
        for x in nodes:
            shifted = [fractions.Fraction(0)] + poly
            poly = [shifted[m] - (x * poly[m] if m < len(poly) else 0) for m in range(len(shifted))]
            den *= (1 - i) - x
        out.append(sum(c / (m + 1) for m, c in enumerate(poly)) / den)
    return out


def integer_form(n):
    ms = mus(n)
    div = 1
    for m in ms:
        div = div * m.denominator // math.gcd(div, m.denominator)
    cs = [m * div for m in ms]
    assert all(c.denominator == 1 for c in cs)
    return [int(c) for c in cs], div


def weights(n):
    """(m_0 / div as a double, [float32((1 / div) * m_i) for i = 1 .. n])"""
    cs, div = integer_form(n)
    return cs[0] / div, [f32((1 / div) * c) for c in cs[1:]]


def dot(fs, a, dt):
    """dt * (((0 + a_0 f_0) + a_1 f_1) + ...), every product and sum rounded to float32"""
    dt = f32(dt)
    with np.errstate(all='ignore'):
        s = (f32(0) + (f32(a[0]) * np.asarray(fs[0], dtype=f32)).astype(f32)).astype(f32)
        for ai, fi in zip(a[1:], fs[1:]):
            s = (s + (f32(ai) * np.asarray(fi, dtype=f32)).astype(f32)).astype(f32)
        return (dt * s).astype(f32)


def predict(y, fs, dt):
    """(dy, delta, u = y + dy) of a step holding len(fs) evaluations"""
    n = len(fs)
    dy = dot(fs, ab.weights(n), dt)
    delta = dot(fs, weights(n)[1], dt)
    with np.errstate(all='ignore'):
        return dy, delta, (np.asarray(y, dtype=f32) + dy).astype(f32)


def lead(dt, n):
    return f32(f32(dt) * f32(weights(n)[0]))


def failed(dy_old, dy_new, rtol, atol):
    """the elements that do NOT satisfy |old - new| < atol + rtol * max(|old|, |new|) in float32 (a NaN fails)"""
    with np.errstate(all='ignore'):
        tol = (f32(atol) + (f32(rtol) * np.maximum(np.abs(dy_old), np.abs(dy_new))).astype(f32)).astype(f32)
        err = np.abs((dy_old - dy_new).astype(f32))
        return ~(err < tol)


def correct(f, delta, y, dy, c0, rtol, atol):
    """(dy', u' = y + dy', number of elements that fail the test) of one corrector pass"""
    with np.errstate(all='ignore'):
        new = ((f32(c0) * np.asarray(f, dtype=f32)).astype(f32) + delta).astype(f32)
        return new, (np.asarray(y, dtype=f32) + new).astype(f32), int(failed(dy, new, rtol, atol).sum())


def solve(f, y0, t, rtol=1e-7, atol=1e-9, max_order=ab.MAX_ORDER, max_iters=MAX_ITERS, step_size=None, fixed_iters=None):
    """(trajectory at the ticks, evaluations, [(iterations, converged) per grid step], states after every grid step).
    f: float32 array -> float32 array (autonomous).  fixed_iters: run exactly that many iterations per step instead of testing."""
    t = np.asarray(t, dtype=f32)
    grid = ab.grid_of(t, step_size)
    max_order = int(min(max_order, ab.MAX_ORDER))
    hist = collections.deque(maxlen=max_order - 1)
    y = np.asarray(y0, dtype=f32)
    nfe = 0

    def fn(x):
        nonlocal nfe
        nfe += 1
        return np.asarray(f(x), dtype=f32)

    sol, states, log, j = [y], [], [], 1
    for i in range(len(grid) - 1):
        t0, t1 = grid[i], grid[i + 1]
        dt = f32(t1 - t0)
        hist.appendleft(fn(y))
        n = len(hist)
        if n < ab.MIN_TERMS:
            y = ab.rk4_step(fn, y, dt, hist[0])
            log.append((0, True))
        else:
            dy, delta, u = predict(y, list(hist), dt)
            c0 = lead(dt, n)
            its, ok = 0, False
            for _ in range(max_iters if fixed_iters is None else fixed_iters[i]):
                dy, u, bad = correct(fn(u), delta, y, dy, c0, rtol, atol)
                its += 1
                ok = bad == 0
                if ok and fixed_iters is None:
                    break
            if not ok:
                hist.pop()
            y = u
            log.append((its, ok))
        states.append(y)
        while j < len(t) and t1 >= t[j]:
            if t[j] == t0 or t[j] == t1:
                sol.append(y)
            else:
                with np.errstate(all='ignore'):
                    sol.append((y + ((y - y) / dt) * f32(t[j] - t0)).astype(f32))
            j += 1
    return np.stack(sol), nfe, log, states
