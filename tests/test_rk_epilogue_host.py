"""tests/_rk_epilogue.py (the host restatement of the fused right-hand sides' Runge-Kutta epilogue) on hand-worked vectors: the order
of the sums, separate roundings, signed zeros, subnormals, overflow, Inf and NaN.  No GPU."""
import math

import numpy as np

import _rk_epilogue as E

F = np.float32
INF, NAN = float('inf'), float('nan')
P24 = F(2.0 ** 24)


def bits(v):
    return np.asarray(v, np.float32).view(np.uint32).tolist()


def a(*v):
    return np.array(v, dtype=np.float32)


def test_stage_sum_alone_and_signed_zero():
    # no earlier stage: the product alone - a zero K times a negative coefficient is -0; the stand-alone form adds it to +0
    got = E.stage_sum([a(1.5, -2.0, 0.0)], [-0.5])
    assert bits(got) == bits(a(-0.75, 1.0, -0.0))
    assert bits(E.stage_sum([a(1.5, -2.0, 0.0)], [-0.5], from_zero=True)) == bits(a(-0.75, 1.0, 0.0))
    assert bits(E.aux([a(0.0)], [-1.0])) == bits(a(-0.0)) and got.dtype == np.float32


def test_stage_sum_order_of_the_additions():
    # u = 1 + 2^24 = 2^24 (tie to even), u + s = 2^24 + 1 = 2^24; the new stage first in a left-to-right sum would give 2^24 + 2
    assert bits(E.stage_sum([a(1.0), a(P24), a(1.0)], [1.0, 1.0, 1.0])) == bits(a(P24))
    # the earlier stages left to right: (2^24 + 1) + 1 = 2^24; right to left would give 2^24 + 2
    assert bits(E.stage_sum([a(P24), a(1.0), a(1.0), a(0.0)], [1.0, 1.0, 1.0, 1.0])) == bits(a(P24))
    # ... and u + s with s formed on its own: 2^24 + (1 + ... ) never sees the small terms one by one
    assert bits(E.stage_sum([a(P24), a(1.0)], [1.0, 2.0])) == bits(a(P24 + F(2.0)))
    # from zero: the same bits wherever a term is non-zero
    assert bits(E.stage_sum([a(1.0), a(P24), a(1.0)], [1.0, 1.0, 1.0], from_zero=True)) == bits(a(P24))
    # a zero and a negative coefficient: 0 * 3 + (-0.5) * 4 + 2 * 0.25
    assert bits(E.stage_sum([a(3.0), a(4.0), a(0.25)], [0.0, -0.5, 2.0])) == bits(a(-1.5))


def test_products_are_rounded_on_their_own():
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 (tie to even); a fused multiply-add would leave 2^-24 behind
    k = F(1.0) + F(2.0 ** -12)
    y0 = -(F(1.0) + F(2.0 ** -11))
    assert bits(E.combine(a(y0), [a(k)], [k])) == bits(a(0.0))
    assert bits(E.combine(a(y0), [a(5.0), a(k)], [0.0, k])) == bits(a(0.0))


def test_combine_signed_zeros_subnormals_overflow():
    # -0 + -0 = -0 (fused form); -0 + +0 = +0 (stand-alone form)
    assert bits(E.combine(a(-0.0), [a(0.0)], [-1.0])) == bits(a(-0.0))
    assert bits(E.combine(a(-0.0), [a(0.0)], [-1.0], from_zero=True)) == bits(a(0.0))
    assert bits(E.combine(a(-0.0), [a(-0.0), a(0.0)], [1.0, -1.0])) == bits(a(-0.0))
    # subnormals are kept: 1e-40 * 0.5 stays subnormal; 1e-40 * 1e-10 underflows to zero with the product's sign
    sub = F(1e-40)
    got = E.combine(a(0.0, 0.0), [a(sub, -sub)], [0.5])
    assert bits(got) == bits(a(sub * F(0.5), -sub * F(0.5))) and 0 < float(got[0]) < 2.0 ** -126
    assert bits(E.stage_sum([a(sub, -sub)], [1e-10])) == bits(a(0.0, -0.0))
    # overflow: 3e38 * 2 = +Inf; Inf - Inf = NaN; 0 * Inf = NaN
    got = E.combine(a(0.0, -INF), [a(3e38, 3e38)], [2.0])
    assert float(got[0]) == INF and math.isnan(float(got[1]))
    assert math.isnan(float(E.combine(a(1.0), [a(INF)], [0.0])[0]))
    got = E.stage_sum([a(3e38), a(-3e38), a(1.0)], [1.0, 1.0, 1.0])
    assert bits(got) == bits(a(1.0))                        # (3e38 - 3e38) + 1


def test_rk4_stages():
    y0 = a(1.0)
    assert bits(E.rk4_stage(0, y0, [a(3.0)], 0.5)) == bits(a(1.5))                          # y + (k1 dt) / 3
    # a division, not a product with 1/3: 5 / 3 = 0x3fd55555, 5 * fl(1/3) = 0x3fd55556
    assert bits(E.rk4_stage(0, a(0.0), [a(5.0)], 1.0)) == [0x3fd55555]
    assert bits(E.rk4_stage(1, y0, [a(3.0), a(1.0)], 0.5)) == bits(a(1.0))                  # y + (k1 / -3 + k2) dt
    assert bits(E.rk4_stage(1, a(0.0), [a(5.0), a(0.0)], 1.0)) == [0xbfd55555]
    assert bits(E.rk4_stage(2, a(0.0), [a(P24), a(-1.0), a(1.0)], 1.0)) == bits(a(P24))     # ((k1 - k2) + k3) dt: both ones are lost
    assert bits(E.rk4_stage(2, y0, [a(4.0), a(1.0), a(2.0)], 0.25)) == bits(a(2.25))
    assert bits(E.rk4_stage(3, y0, [a(1.0), a(2.0), a(3.0), a(4.0)], 0.8)) == bits(a(3.0))  # 1 + 20 * (fl(0.8) / 8) = 1 + fl(2.00000003)
    # left to right: (2^24 + 0.75) + 0.75 = 2^24; the two small terms added first would give 2^24 + 2
    assert bits(E.rk4_stage(3, a(0.0), [a(P24), a(0.25), a(0.25), a(0.0)], 8.0)) == bits(a(P24))
    # specials: NaN propagates, Inf - Inf, -0
    got = E.rk4_stage(2, a(0.0, 0.0, -0.0), [a(NAN, INF, 0.0), a(1.0, INF, 0.0), a(1.0, 1.0, -0.0)], 1.0)
    assert math.isnan(float(got[0])) and math.isnan(float(got[1]))
    assert bits(got[2:]) == bits(a(0.0))                    # (0 - 0) + -0 = +0; +0 * 1 = +0; -0 + +0 = +0


def test_max_nan():
    got = E.max_nan(a(1.0, 2.0, NAN, 1.0, NAN, 0.0, INF), a(2.0, 1.0, 1.0, NAN, NAN, 0.0, 1.0))
    assert bits(got[:2]) == bits(a(2.0, 2.0)) and np.isnan(got[2:5]).all() and bits(got[5:]) == bits(a(0.0, INF))


def test_error_terms_plain_and_specials():
    rtol, atol = 0.5, 0.25
    #            tol = .25 + .5 * 2   .25 + .5 * 3   y1 = +Inf      y1 = -Inf     y1 = NaN   y0 = NaN   y0 = Inf, s = Inf
    y0 = a(1.0, -3.0, 1.0, 1.0, 1.0, NAN, INF)
    y1 = a(-2.0, 1.0, INF, -INF, NAN, 1.0, 1.0)
    K = a(2.5, 3.5, 7.0, 7.0, 7.0, 7.0, INF)
    zz, bad = E.error_terms(y0, y1, [K], [1.0], rtol, atol)
    assert zz.dtype == np.float64 and bad == 3
    assert zz[:4].tolist() == [4.0, 4.0, 0.0, 0.0] and np.isnan(zz[4:]).all()
    # two stages, a negative coefficient: s = 4 * 0.5 + 2 * -0.25 = 1.5; tol = 0.25 + 0.5 * 1 = 0.75; z = 2
    zz, bad = E.error_terms(a(1.0), a(0.5), [a(4.0), a(2.0)], [0.5, -0.25], rtol, atol)
    assert zz.tolist() == [4.0] and bad == 0
    # z * z is an fp32 product: z = 2^70 squares to +Inf before it is widened
    zz, _ = E.error_terms(a(0.0), a(0.0), [a(2.0 ** 68)], [1.0], 0.0, atol)
    assert zz.tolist() == [INF]
    # fp32 roundings of the quotient: 1 / 3 squared = fl(fl(1/3)^2), not the fp64 value
    zz, _ = E.error_terms(a(0.0), a(0.0), [a(1.0)], [1.0], 0.0, 3.0)
    z = F(1.0) / F(3.0)
    assert zz.tolist() == [float(F(z * z))] and zz[0] != float(z) * float(z)


def test_error_terms_zero_tolerance():
    # atol = 0 and y0 = y1 = 0: tol = 0; a non-zero sum gives z = +-Inf (term +Inf), a zero sum 0 / 0 = NaN
    zz, bad = E.error_terms(a(0.0, -0.0, 0.0, 2.0), a(0.0, 0.0, -0.0, 1.0), [a(1.0, -1.0, 0.0, 1.0)], [1.0], 0.5, 0.0)
    assert bad == 0 and zz[0] == INF and zz[1] == INF and math.isnan(zz[2]) and zz[3] == 1.0
    # subnormal tolerance and sum: 1e-40 / 1e-40
    zz, _ = E.error_terms(a(0.0), a(0.0), [a(1e-40)], [1.0], 0.0, 1e-40)
    assert zz.tolist() == [1.0]


def test_from_zero_changes_no_error_term():
    rng = np.random.RandomState(0)
    kk = [rng.randn(64).astype(np.float32) for _ in range(4)]
    kk[3][::3] = 0.0
    kk[0][::3] = -0.0
    cs = [0.3, 0.0, -0.2, -0.7]
    y0, y1 = rng.randn(64).astype(np.float32), rng.randn(64).astype(np.float32)
    z1, _ = E.error_terms(y0, y1, kk, cs, 1e-2, 1e-3)
    z2, _ = E.error_terms(y0, y1, kk, cs, 1e-2, 1e-3, from_zero=True)
    assert np.array_equal(z1, z2)
    import _aten_order as ao
    assert np.array_equal(E.stage_sum(kk, cs, from_zero=True).view(np.uint32), ao.wsum(kk, cs).view(np.uint32))
    assert np.array_equal(z2, ao.error_elements(y0, y1, kk, cs, 1e-2, 1e-3).astype(np.float64))
