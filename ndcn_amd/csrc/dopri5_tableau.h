// Dormand-Prince 5(4): dopri5.py:11-36, written as the same rational expressions (evaluated in double, rounded to float where the
// reference multiplies them with a float32 0-d tensor).  Shared by the device-resident solver (solver.hip) and the training tape
// (tape.hip).
#pragma once
#include <math.h>

namespace ndcn {

static const double kAlpha[6] = {1. / 5, 3. / 10, 4. / 5, 8. / 9, 1., 1.};
static const double kBeta[6][6] = {
    {1. / 5},
    {3. / 40, 9. / 40},
    {44. / 45, -56. / 15, 32. / 9},
    {19372. / 6561, -25360. / 2187, 64448. / 6561, -212. / 729},
    {9017. / 3168, -355. / 33, 46732. / 5247, 49. / 176, -5103. / 18656},
    {35. / 384, 0, 500. / 1113, 125. / 192, -2187. / 6784, 11. / 84},
};
static const double kCErr[7] = {
    35. / 384 - 1951. / 21600, 0, 500. / 1113 - 22642. / 50085, 125. / 192 - 451. / 720,
    -2187. / 6784 - -12231. / 42400, 11. / 84 - 649. / 6300, -1. / 60.,
};
static const double kCMid[7] = {
    6025192743. / 30085553152. / 2, 0, 51252292925. / 65400821598. / 2, -2691868925. / 45128329728. / 2,
    187940372067. / 1594534317056. / 2, -1776094331. / 19743644256. / 2, 11237099. / 235043384. / 2,
};

static inline double nan_max(double a, double b) { return (isnan(a) || isnan(b)) ? NAN : (a > b ? a : b); }
static inline double nan_min(double a, double b) { return (isnan(a) || isnan(b)) ? NAN : (a < b ? a : b); }

// The scalar arithmetic both files must agree on to the last bit: plain functions of floats and doubles, no state.

// The non-zero terms of a tableau row scaled by the step size ((scale * x) of misc.py:25 in float32; exact-zero entries are dropped,
// their product is 0): kp / cp get the stages and fl(dt32 * row[j]), idx (nullable) the stage indices.  Returns their number.
static inline int dt_terms(float dt32, const double *row, int n, const float *const *kall, const float **kp, float *cp,
                           int *idx = nullptr) {
    int m = 0;
    for (int j = 0; j < n; ++j) {
        const float bj = (float)row[j];
        if (bj == 0.f) continue;
        kp[m] = kall[j];
        cp[m] = dt32 * bj;
        if (idx) idx[m] = j;
        ++m;
    }
    return m;
}

// misc.py:160-170 for an error ratio != 0 (the caller handles ratio == 0: dt * ifactor): factor = max(a, min(b, c)) in float64, the
// square root in the ratio's float32; dt_next = dt / factor.  The candidates are kept for the training tape's reverse pass.
static const double kStepExpo = (double)0.2f;          // order 5 passed through a float32 tensor (dopri5.py:72-74)
struct StepFactor {
    double er, a, b, c, factor;
};
static inline StepFactor step_factor(float ratio, double safety, double ifactor, double dfactor) {
    StepFactor f;
    f.er = (double)sqrtf(ratio);
    f.a = 1.0 / ifactor;
    f.b = pow(f.er, kStepExpo) / safety;
    f.c = 1.0 / (ratio < 1.f ? 1.0 : dfactor);
    f.factor = nan_max(f.a, nan_min(f.b, f.c));
    return f;
}

// misc.py:84-143, the scalar finish of the initial step in the state dtype.  d0, d1: rms of y0 / scale and f0 / scale.
static inline float initial_h0(float d0, float d1, bool *is_const = nullptr) {
    const bool c = d0 < 1e-5 || d1 < 1e-5;
    if (is_const) *is_const = c;
    return c ? 1e-6f : 0.01f * (d0 / d1);
}
// `0.01 / m`, m = python max([d1, d2]), as torch evaluates it on a float32 0-d tensor (misc.py:141): python_scalar / tensor is
// tensor.reciprocal() * scalar - two float32 roundings.  max returns the first maximum: `>=` and `>` pick the same VALUE for every
// input (equal operands are one value - two zeros of either sign never get here, initial_h1; a NaN d1 fails both comparisons and
// yields d2, a NaN d2 fails both and yields d2 = NaN)
static inline float initial_h1_base(float d1, float d2, float *m_out = nullptr) {
    const float m = d1 >= d2 ? d1 : d2;
    if (m_out) *m_out = m;
    return (1.0f / m) * 0.01f;
}
// d2: rms of (f1 - f0) / scale, already divided by h0
static inline float initial_h1(float d1, float d2, float h0, bool *is_alt = nullptr) {
    const bool alt = d1 <= 1e-15 && d2 <= 1e-15;
    if (is_alt) *is_alt = alt;
    if (alt) {
        const float a = 1e-6f, b = h0 * 1e-3f;
        return a > b ? a : b;
    }
    // tensor ** python_float runs std::pow in double with the exponent at full double precision, rounded to float32 once
    return (float)pow((double)initial_h1_base(d1, d2), 1. / 5.);
}
static inline double initial_dt(float h0, float h1) {
    const float h100 = 100.f * h0;
    if (isnan(h100) || isnan(h1)) return NAN;
    return (double)(h100 < h1 ? h100 : h1);
}

// interp.py:51-65: the abscissa x = (at - a0) / (a1 - a0) and its powers {x^4, x^3, x^2, x, 1} in the state dtype.
// false: `at` lies outside [a0, a1] (xp untouched; the caller raises)
static inline bool interp_abscissa(float a0, float a1, float at, float xp[5]) {
    if (!(a0 <= at && at <= a1)) return false;
    const float x = (at - a0) / (a1 - a0);
    xp[4] = 1.f; xp[3] = x; xp[2] = xp[3] * x; xp[1] = xp[2] * x; xp[0] = xp[1] * x;
    return true;
}

}  // namespace ndcn
