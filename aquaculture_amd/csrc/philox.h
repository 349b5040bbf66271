// The one generator of the Monte-Carlo kernels (tonnage.hip: the production bootstrap; population.hip: the Bernoulli samples of the
// population bound).  tonnage.py's philox4x32 and uniform_from_words restate it word for word.
//   philox    Philox4x32-10, counter (c0, c1, c2, c3), key (k0, k1); per round (hi0, lo0) = M0 c0, (hi1, lo1) = M1 c2,
//             c <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key grows by (W0, W1) between rounds
//   uniform   x = (hi : lo) >> 11 (53 bits); u = ((double)x + 0.5) * 2^-53; u = u < 1 ? u : 1 - 2^-53
// Each 32 x 32 -> 64 product is written as one 64-bit multiply of two zero-extended words; the compiler forms it from a low and a high
// 32-bit multiply (or one v_mad_u64_u32), which is all the integer-multiply work a round has.
#pragma once
#include <stdint.h>

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

struct PhiloxWords { uint32_t w0, w1, w2, w3; };

__device__ inline PhiloxWords philox4x32(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    return {c0, c1, c2, c3};
}

// the 53-bit uniform of a pair of words, strictly inside (0, 1)
__device__ inline double philox_words_uniform(uint32_t lo, uint32_t hi) {
    const uint64_t x = (((uint64_t)hi << 32) | lo) >> 11;
    const double u = ((double)x + 0.5) * 0x1p-53;
    return u < 1.0 ? u : 0x1.fffffffffffffp-1;
}

__device__ inline double philox_uniform(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    const PhiloxWords w = philox4x32(k0, k1, c0, c1, c2, c3);
    return philox_words_uniform(w.w0, w.w1);
}
