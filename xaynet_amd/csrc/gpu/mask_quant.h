// The exact update quantiser: v = trunc((clamp(scalar * w) + add_shift) *
// exp_shift) in integers only, the value the rational masker (mask_model in
// mask/masking.cpp) adds the mask to. Shared by the K5w exact kernel
// (kernels.hip) and the host (quantize_exact in mask_bindings.cpp), so it
// compiles as plain C++ like limbs.h, and keeps its discipline: compile-time
// loop bounds, no run-time limb index.
//
// With a = add_shift (an integer in every GPU config), E = exp_shift, the
// scalar p/q already clamped to the unit config's bound, and an element of
// magnitude |w| = m * 2^-K (integer m < 2^64):
//   w == 0 or p == 0:        v = aE
//   p*m >= a*q*2^K (clamp):  v = 2aE (w > 0) or 0 (w < 0)
//   else, with X = p*m*E * 2^max(0,-K), D = q * 2^max(0,K), t = floor(X / D):
//                            v = aE + t (w > 0), aE - t - [X mod D != 0] (w < 0)
// X / D is a shift by K with a sticky bit, then a division by the word q.
#pragma once

#include <cstring>

#include "limbs.h"

// Working width for an L-limb order: X = p*m*E is below 2^(127 + bits(E)),
// and past the clamp test below a*q*E < 2^63 * order / 2. E is 10^10 for u64
// orders, up to 10^20 for u128 ones (F64) and 10^45 beyond (F32 Bmax);
// mq_prepare checks that the constants fit.
constexpr int mq_width(int L) { return L <= 2 ? L + 2 : L + 1; }

// What the quantiser needs besides the element; made by mq_prepare.
struct mq_params {
    xhip_limbs aE;  // add_shift * exp_shift
    xhip_limbs aq;  // add_shift * q
    xhip_limbs pE;  // p * exp_shift
    uint64_t p, q;
};

// low N limbs of a * b
template <int N>
ML_FN limbs<N> ml_mul(const limbs<N>& a, const limbs<N>& b) {
    limbs<N> r = ml_zero<N>();
#pragma unroll
    for (int j = N - 1; j >= 0; --j) {
        ml_shl_limb(r);
        ml_add(r, ml_mul_word(a, b.w[j]));
    }
    return r;
}

// number of significant bits
template <int N>
ML_FN int ml_bits(const limbs<N>& a) {
    int bits = 0;
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (a.w[j]) bits = 64 * j + 64 - __builtin_clzll(a.w[j]);
    return bits;
}

// Derives the constants for an order of L limbs. False where the exact
// kernel does not apply: p or q out of range, 2*a*E not below the order, or
// an intermediate past the working width.
ML_FN bool mq_prepare(const xhip_limbs& order, int L, const xhip_limbs& a, const xhip_limbs& E,
                      uint64_t p, uint64_t q, mq_params& out) {
    constexpr int N = 2 * ML_MAX_LIMBS;  // holds any product of two constants
    if (L < 1 || L > ML_MAX_LIMBS || q == 0 || (p >> 63) || (q >> 63)) return false;
    const limbs<N> o = ml_resize<N>(ml_from<ML_MAX_LIMBS>(order));
    const limbs<N> av = ml_resize<N>(ml_from<ML_MAX_LIMBS>(a));
    const limbs<N> ev = ml_resize<N>(ml_from<ML_MAX_LIMBS>(E));
    if (ml_is_zero(av) || ml_is_zero(ev)) return false;
    limbs<N> aE = ml_mul(av, ev);
    limbs<N> twice = aE;
    ml_shl_bits(twice, 1);
    if (ml_geq(twice, o)) return false;
    const limbs<N> aq = ml_mul_word(av, q);
    const limbs<N> pE = ml_mul_word(ev, p);
    const int W = mq_width(L);
    const int cap = 64 * (W < ML_MAX_LIMBS ? W : ML_MAX_LIMBS);  // as launcher constants
    if (ml_bits(o) > 64 * L || 127 + ml_bits(ev) > 64 * W || ml_bits(aq) > cap ||
        ml_bits(pE) > cap)
        return false;
    out.aE = xhip_limbs{{aE.w[0], aE.w[1], aE.w[2], aE.w[3], aE.w[4]}};
    out.aq = xhip_limbs{{aq.w[0], aq.w[1], aq.w[2], aq.w[3], aq.w[4]}};
    out.pE = xhip_limbs{{pE.w[0], pE.w[1], pE.w[2], pE.w[3], pE.w[4]}};
    out.p = p;
    out.q = q;
    return true;
}

// a launcher constant widened to W limbs (W may exceed ML_MAX_LIMBS)
template <int W>
ML_FN limbs<W> mq_from(const xhip_limbs& c) {
    constexpr int K = W < ML_MAX_LIMBS ? W : ML_MAX_LIMBS;
    return ml_resize<W>(ml_from<K>(c));
}

// (u1:u0) / d for u1 < d: the quotient, which fits a word, and the remainder.
// Two rounds of 32-bit-digit long division on the normalised divisor, so no
// 128-bit division is needed.
ML_FN uint64_t mq_div_2by1(uint64_t u1, uint64_t u0, uint64_t d, uint64_t& rem) {
    const uint64_t b = uint64_t(1) << 32;
    const int s = __builtin_clzll(d);
    d <<= s;
    const uint64_t d1 = d >> 32, d0 = d & 0xffffffffu;
    const uint64_t n32 = s ? (u1 << s) | (u0 >> (64 - s)) : u1;
    const uint64_t n10 = u0 << s;
    const uint64_t n1 = n10 >> 32, n0 = n10 & 0xffffffffu;
    uint64_t q1 = n32 / d1, rhat = n32 - q1 * d1;
    while (q1 >= b || q1 * d0 > b * rhat + n1) {
        --q1;
        rhat += d1;
        if (rhat >= b) break;
    }
    const uint64_t n21 = n32 * b + n1 - q1 * d;
    uint64_t q0 = n21 / d1;
    rhat = n21 - q0 * d1;
    while (q0 >= b || q0 * d0 > b * rhat + n0) {
        --q0;
        rhat += d1;
        if (rhat >= b) break;
    }
    rem = (n21 * b + n0 - q0 * d) >> s;
    return q1 * b + q0;
}

// a = a / d, returns a % d (d != 0): ml_divrem_word on mq_div_2by1
template <int N>
ML_FN uint64_t mq_divrem_word(limbs<N>& a, uint64_t d) {
    uint64_t rem = 0;
#pragma unroll
    for (int j = N - 1; j >= 0; --j) a.w[j] = mq_div_2by1(rem, a.w[j], d, rem);
    return rem;
}

// An element as the rational masker sees it: sign, and |w| = m * 2^-K. NaN is
// 0 and an infinity the largest finite value of its type.
struct mq_value {
    uint64_t m;
    int K;
    bool neg;
};

ML_FN mq_value mq_decompose(float w) {
    uint32_t bits;
    memcpy(&bits, &w, sizeof bits);
    uint32_t exp = (bits >> 23) & 0xffu, frac = bits & 0x7fffffu;
    const bool neg = (bits >> 31) != 0;
    if (exp == 0xffu) {
        if (frac) return mq_value{0, 0, false};  // NaN
        exp = 0xfeu;                             // +-inf -> +-max
        frac = 0x7fffffu;
    }
    if (exp == 0) return mq_value{frac, 149, neg};  // zero and denormals
    return mq_value{uint64_t(frac) | (uint64_t(1) << 23), 150 - int(exp), neg};
}

ML_FN mq_value mq_decompose(double w) {
    uint64_t bits;
    memcpy(&bits, &w, sizeof bits);
    uint64_t exp = (bits >> 52) & 0x7ffu, frac = bits & ((uint64_t(1) << 52) - 1);
    const bool neg = (bits >> 63) != 0;
    if (exp == 0x7ffu) {
        if (frac) return mq_value{0, 0, false};
        exp = 0x7feu;
        frac = (uint64_t(1) << 52) - 1;
    }
    if (exp == 0) return mq_value{frac, 1074, neg};
    return mq_value{frac | (uint64_t(1) << 52), 1075 - int(exp), neg};
}

// the most negative value has magnitude 2^63 (2^31), which the unsigned
// negation yields
ML_FN mq_value mq_decompose(int64_t w) {
    return mq_value{w < 0 ? uint64_t(0) - uint64_t(w) : uint64_t(w), 0, w < 0};
}

ML_FN mq_value mq_decompose(int32_t w) { return mq_decompose(int64_t(w)); }

// The quantised value of one element for an order of L limbs, below the
// order (at most 2aE).
template <int L>
ML_FN limbs<L> mq_quantize(const mq_value& x, const mq_params& c) {
    constexpr int W = mq_width(L);
    limbs<L> v = ml_from<L>(c.aE);
    if (x.m == 0 || c.p == 0) return v;

    // clamp: p*m >= a*q * 2^K
    const unsigned __int128 pm128 = (unsigned __int128)c.p * x.m;
    limbs<W> pm = ml_zero<W>();
    pm.w[0] = uint64_t(pm128);
    pm.w[1] = uint64_t(pm128 >> 64);
    limbs<W> aq = mq_from<W>(c.aq);
    if (x.K >= 0)
        ml_shr_sticky(pm, x.K);  // floor(p*m / 2^K) >= a*q
    else if (ml_shr_sticky(aq, -x.K))
        ml_add_word(aq, 1);  // p*m >= ceil(a*q / 2^-K)
    if (ml_geq(pm, aq)) {
        if (x.neg) return ml_zero<L>();
        ml_shl_bits(v, 1);
        return v;
    }

    // t = floor(X / D), and whether the division left a remainder
    limbs<W> X = ml_mul_word(mq_from<W>(c.pE), x.m);
    bool inexact = false;
    if (x.K >= 0)
        inexact = ml_shr_sticky(X, x.K);
    else
        ml_shl(X, -x.K);  // not clamped: below a*q*E, and -K below 64*W
    if (c.q != 1) inexact |= mq_divrem_word(X, c.q) != 0;
    // X = t < aE; a negative element takes the ceiling, which is at most aE
    if (x.neg) {
        if (inexact) ml_add_word(X, 1);
        ml_sub(v, ml_resize<L>(X));
    } else {
        ml_add(v, ml_resize<L>(X));
    }
    return v;
}
