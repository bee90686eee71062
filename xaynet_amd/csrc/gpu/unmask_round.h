// The exact float unmask: the float nearest to mag / q (ties to even), from
// integers only. mag = |t - nb*add_shift*exp_shift| is the offset-free
// aggregate and q = exp_shift * scalar_sum the exact divisor, so mag / q is
// the rational the coordinator publishes and the result is that rational
// rounded ONCE to the model's float type. Shared by the K4 exact kernel
// (kernels.hip) and the host (unmask_round in mask_bindings.cpp), so it
// compiles as plain C++ like limbs.h, and keeps its discipline: compile-time
// loop bounds, no run-time limb index.
//
// With bm, bq the bit lengths of mag and q, and p the float's precision (24
// or 53), K = p + 3 steps of restoring division give
//   X = floor(mag / q * 2^e),  e = K + bq - 1 - bm,
// an integer of K - 1 or K bits (2^(bm-bq-1) < mag/q < 2^(bm-bq+1)): the p
// result bits, a guard bit and at least one more. mag is left-aligned, its
// top bq - 1 bits are the first remainder (below 2^(bq-1) <= q), and every
// step shifts in the next bit of mag - zeros once it is used up - compares
// and subtracts on L + 1 limbs. What is left of mag and of the remainder is
// the sticky bit. Every element takes the same K steps.
//
// X is then cut to p bits, or to fewer where the unit of the last place
// would fall below the type's smallest subnormal, rounded on guard and
// sticky, and written as the bit pattern: with the exponent field counted
// from the subnormal unit, subnormals, normals and the carry out of an
// all-ones mantissa are one addition.
#pragma once

#include <cstring>

#include "mask_quant.h"  // ml_bits

template <typename F>
struct ur_format;
template <>
struct ur_format<float> {
    using bits_t = uint32_t;
    static constexpr int precision = 24;
    static constexpr int min_unit = -149;  // log2 of the smallest subnormal
    static constexpr int top_exponent = 255;
};
template <>
struct ur_format<double> {
    using bits_t = uint64_t;
    static constexpr int precision = 53;
    static constexpr int min_unit = -1074;
    static constexpr int top_exponent = 2047;
};

// The F nearest to mag / q, ties to even, negative if `neg` (mag == 0 is +0).
// Below the normal range the result lies on the subnormal grid; beyond the
// largest finite value it saturates there: no infinity, no NaN. q != 0.
template <typename F, int L>
ML_FN F ur_round(bool neg, limbs<L> mag, const limbs<L>& q) {
    using fmt = ur_format<F>;
    using bits_t = typename fmt::bits_t;
    constexpr int P = fmt::precision;
    constexpr int K = P + 3;
    if (ml_is_zero(mag)) return F(0);
    const int bm = ml_bits(mag), bq = ml_bits(q);
    ml_shl(mag, 64 * L - bm);  // left-aligned: the top bit is set
    limbs<L> head = mag;       // its top bq - 1 bits
    ml_shr_sticky(head, 64 * L - (bq - 1));
    ml_shl(mag, bq - 1);  // the bits still to shift in, from the top
    limbs<L + 1> rem = ml_resize<L + 1>(head);
    const limbs<L + 1> den = ml_resize<L + 1>(q);
    uint64_t x = 0;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const uint64_t bit = mag.w[L - 1] >> 63;
        ml_shl_bits(mag, 1);
        ml_shl_bits(rem, 1);  // rem < q < 2^(64L): fits L + 1 limbs
        rem.w[0] |= bit;
        limbs<L + 1> trial = rem;
        const uint64_t borrow = ml_sub(trial, den);
        if (!borrow) rem = trial;
        x = (x << 1) | (borrow ^ 1);
    }
    const bool sticky = !ml_is_zero(mag) || !ml_is_zero(rem);
    const int e = K + bq - 1 - bm;          // x = floor(mag / q * 2^e)
    int cut = 64 - __builtin_clzll(x) - P;  // x has K - 1 or K bits: 2 or 3
    int unit = cut - e;                     // log2 of the result's last place
    if (unit < fmt::min_unit) {
        cut += fmt::min_unit - unit;
        unit = fmt::min_unit;
    }
    uint64_t m = 0;
    if (cut < 64) {  // else even the guard bit is above x: zero
        m = x >> cut;
        const uint64_t guard = (x >> (cut - 1)) & 1;
        const bool below = sticky || (x & ((uint64_t(1) << (cut - 1)) - 1)) != 0;
        m += guard & (uint64_t(below) | (m & 1));
    }
    // the top mantissa bit of a normal adds the 1 the exponent field lacks
    // here, and m == 2^P carries into it
    uint64_t pattern = (uint64_t(unit - fmt::min_unit) << (P - 1)) + m;
    constexpr uint64_t inf = uint64_t(fmt::top_exponent) << (P - 1);
    if (pattern >= inf) pattern = inf - 1;  // the largest finite value
    if (neg) pattern |= uint64_t(1) << (8 * sizeof(F) - 1);
    const bits_t b = bits_t(pattern);
    F out;
    memcpy(&out, &b, sizeof out);
    return out;
}
