// The arithmetic of one Adams-Bashforth step, shared by the translation units that form it (adams.hip: ab_step_kernel;
// adams_readout.hip: the step with the decoder).  Include it BEHIND `#pragma clang fp contract(off)`: every product and sum of ab1 is
// rounded on its own (fixed_adams.py:182, misc.py:22-25, solvers.py:92).
#pragma once

namespace ndcn {

namespace {

constexpr int kAbMinTerms = 3;         // fixed_adams.py:146,174: below order 3 the step is RK4
constexpr int kAbMaxTerms = 11;        // :147,163: max_order 12 keeps 11 evaluations
constexpr int kAbMaxOrder = 12;
constexpr int kDecMaxTicks = 8;        // ticks one step + decode launch takes (adams_readout.hip), as interp_readout_f32 / tick_emit_f32

struct AbArgs {
    const float *f[kAbMaxTerms];       // newest first
    float a[kAbMaxTerms];
    const float *y;
    float *out;
    float dt;
};

__device__ __forceinline__ float ab1(float y, const float *f, const float *a, int n, float dt) {
    float s = 0.f + a[0] * f[0];                            // Python's sum() starts from 0: a lone -0 product becomes +0
#pragma unroll
    for (int j = 1; j < n; ++j) s = s + a[j] * f[j];
    return y + dt * s;
}

}  // namespace

}  // namespace ndcn
