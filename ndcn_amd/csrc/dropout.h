// The dropout mask of ODEFunc (neural_dynamics.py:34: dropout between the Linear and the ReLU) as a PURE FUNCTION of
// (p, seed, evaluation, flat element index) - not of the route, the launch geometry, H or the thread that computes it, so that every
// kernel family applies the same mask and a reverse pass that re-forms a stage re-creates it from three numbers:
//
//   p32 = float32(p), 0 < p32 < 1;  s = 1.0f / (1.0f - p32) in float32;  T = floor(double(p32) * 2^32)      (below 2^32)
//   element i = row * H + col (int64):  Philox4x32-10 with counter (lo32(i >> 2), hi32(i >> 2), lo32(evaluation), hi32(evaluation))
//   and key (lo32(seed), hi32(seed));  u = output word i & 3;  kept iff u >= T;  m = kept ? s : 0
//   K' = relu_nan(z) * m, one rounded float32 product (NaN and Inf times 0 stay NaN, as x * mask * scale does in torch)
//
// The dropout factor is 0 or s > 0, so relu(z * m) = relu(z) * m: the mask multiplies the launch's own output.  One Philox call serves
// four consecutive elements - a 16-byte lane.  Philox4x32-10: Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2,
// 3" (SC'11); known answers in tests/test_dropout_host.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NDCN_HD __host__ __device__ __forceinline__

namespace ndcn {

// the descriptor of ndcn_dropout in the form the kernels read (host side: drop_args())
struct DropArgs {
    float s;                    // 1 / (1 - p32)
    uint32_t thresh;            // T; kept iff u >= T
    uint32_t k0, k1;            // seed
    uint32_t e0, e1;            // evaluation
};

struct Philox4 { uint32_t w[4]; };

NDCN_HD uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

NDCN_HD void philox_round(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t &k0, uint32_t &k1) {
    const uint32_t hi0 = philox_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = philox_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
}

// ROLLED: the ten rounds as a loop - the round keys are formed as it goes instead of living in twenty scalar registers (the
// narrow-panel launch, whose epilogues hold their coefficients there); the streaming pass unrolls
template <bool ROLLED = false>
NDCN_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    if (ROLLED) {
#pragma unroll 1
        for (int r = 0; r < 10; ++r) philox_round(c0, c1, c2, c3, k0, k1);
    } else {
#pragma unroll
        for (int r = 0; r < 10; ++r) philox_round(c0, c1, c2, c3, k0, k1);
    }
    Philox4 o;
    o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

// the four words of elements 4 q .. 4 q + 3
template <bool ROLLED = false>
NDCN_HD Philox4 drop_words(const DropArgs &d, int64_t q) {
    return philox4x32_10<ROLLED>((uint32_t)((uint64_t)q & 0xffffffffu), (uint32_t)((uint64_t)q >> 32), d.e0, d.e1, d.k0, d.k1);
}

// m of element i
template <bool ROLLED = false>
NDCN_HD float drop_factor(const DropArgs &d, int64_t i) {
    const Philox4 o = drop_words<ROLLED>(d, i >> 2);
    const int j = (int)(i & 3);
    const uint32_t u = j == 0 ? o.w[0] : (j == 1 ? o.w[1] : (j == 2 ? o.w[2] : o.w[3]));
    return u >= d.thresh ? d.s : 0.f;
}

}  // namespace ndcn
