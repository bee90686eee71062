// The model encoder: one weight -> its bincode Ratio<BigInt> element, as
// 32-bit words, in integers only. Shared by the K7 kernels (kernels.hip) and
// the host (model_codec_encode / model_codec_words in sdk_bindings.cpp), so it
// compiles as plain C++ like limbs.h and mask_quant.h. The format is the one
// write_dyadic and the encode_range_* functions of message/bincode.cpp write;
// that file stays the independent reference.
//
// A weight is zero or +-m * 2^e with m odd. Every field of its element is a
// whole number of u32 words (a u64 count is two):
//   zero:    sign 1 (NoSign) | count 0 | sign 2 (Plus) | count 1 | 1      7 words
//   e >= 0:  sign 0/2 | count nd | nd digits of m << e | 2 | count 1 | 1  7 + nd
//   e <  0:  sign 0/2 | count nd | nd digits of m | 2 | count dd |
//            dd digits of 2^-e                                            6 + nd + dd
// sign is 0 (Minus) or 2 (Plus), digits are little-endian base 2^32 without
// leading zeros. NaN, the infinities and -0.0 are the zero element.
//
// Nothing here keeps an array: mc_write stores each word as it is made, so the
// kernel that inlines it needs no scratch.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define MC_FN __host__ __device__ __forceinline__
#else
#define MC_FN inline
#endif

// the longest element: the least normal double with a full mantissa,
// (2^53 - 1) / 2^1074, has 2 numerator and 34 denominator digits
#define MC_MAX_WORDS 42

// +-m * 2^e, m odd; m == 0 is the zero element (e and neg are then unused)
struct mc_value {
    uint64_t m;
    int e;
    bool neg;
};

MC_FN mc_value mc_reduced(uint64_t m, int e, bool neg) {
    if (m == 0) return mc_value{0, 0, false};
    const int tz = __builtin_ctzll(m);
    return mc_value{m >> tz, e + tz, neg};
}

MC_FN mc_value mc_decompose(float w) {
    uint32_t bits;
    memcpy(&bits, &w, sizeof bits);
    const uint32_t exp = (bits >> 23) & 0xffu, frac = bits & 0x7fffffu;
    const bool neg = (bits >> 31) != 0;
    if (exp == 0xffu) return mc_value{0, 0, false};              // NaN, +-inf
    if (exp == 0) return mc_reduced(frac, -149, neg);            // zero and subnormals
    return mc_reduced(uint64_t(frac) | (uint64_t(1) << 23), int(exp) - 150, neg);
}

MC_FN mc_value mc_decompose(double w) {
    uint64_t bits;
    memcpy(&bits, &w, sizeof bits);
    const uint64_t exp = (bits >> 52) & 0x7ffu, frac = bits & ((uint64_t(1) << 52) - 1);
    const bool neg = (bits >> 63) != 0;
    if (exp == 0x7ffu) return mc_value{0, 0, false};
    if (exp == 0) return mc_reduced(frac, -1074, neg);
    return mc_reduced(frac | (uint64_t(1) << 52), int(exp) - 1075, neg);
}

// the most negative value has magnitude 2^63 (2^31), which the unsigned
// negation yields
MC_FN mc_value mc_decompose(int64_t w) {
    return mc_reduced(w < 0 ? uint64_t(0) - uint64_t(w) : uint64_t(w), 0, w < 0);
}

MC_FN mc_value mc_decompose(int32_t w) { return mc_decompose(int64_t(w)); }

// digits of the numerator: of m << e (e >= 0), or of m
MC_FN uint32_t mc_numer_digits(const mc_value& v) {
    const int bits = 64 - __builtin_clzll(v.m) + (v.e > 0 ? v.e : 0);
    return uint32_t(bits + 31) >> 5;
}

// the number of u32 words of the element
MC_FN uint32_t mc_words(const mc_value& v) {
    if (v.m == 0) return 7;
    const uint32_t nd = mc_numer_digits(v);
    return v.e >= 0 ? 7 + nd : 6 + nd + (uint32_t(-v.e) >> 5) + 1;
}

// writes the mc_words(v) words of the element at out
MC_FN void mc_write(const mc_value& v, uint32_t* out) {
    if (v.m == 0) {
        out[0] = 1;  // NoSign, no digits
        out[1] = 0;
        out[2] = 0;
        out[3] = 2;  // Plus, one digit: 1
        out[4] = 1;
        out[5] = 0;
        out[6] = 1;
        return;
    }
    const uint32_t nd = mc_numer_digits(v);
    out[0] = v.neg ? 0u : 2u;
    out[1] = nd;
    out[2] = 0;
    out += 3;
    if (v.e >= 0) {
        // m << e: m shifted by e % 32 bits spans up to three digits, above
        // e / 32 zero digits
        const uint32_t zeros = uint32_t(v.e) >> 5, sh = uint32_t(v.e) & 31u;
        const uint64_t lo = v.m << sh;
        const uint32_t hi = sh ? uint32_t(v.m >> (64 - sh)) : 0u;
        for (uint32_t i = 0; i < zeros; ++i) out[i] = 0;
        out[zeros] = uint32_t(lo);
        if (zeros + 1 < nd) out[zeros + 1] = uint32_t(lo >> 32);
        if (zeros + 2 < nd) out[zeros + 2] = hi;
        out += nd;
        out[0] = 2;  // denominator 1
        out[1] = 1;
        out[2] = 0;
        out[3] = 1;
        return;
    }
    out[0] = uint32_t(v.m);
    if (nd == 2) out[1] = uint32_t(v.m >> 32);
    out += nd;
    // denominator 2^k: k / 32 zero digits, then one bit
    const uint32_t k = uint32_t(-v.e), zeros = k >> 5;
    out[0] = 2;
    out[1] = zeros + 1;
    out[2] = 0;
    out += 3;
    for (uint32_t i = 0; i < zeros; ++i) out[i] = 0;
    out[zeros] = uint32_t(1) << (k & 31u);
}

// ---- the inverse: words -> weight (the K7d kernels, model_codec_decode) ----

// The length in words (7..MC_MAX_WORDS) of an element that would start at w,
// from its two count fields alone, or 0: both counts' high words are zero,
// the denominator has a digit, and the element fits MC_MAX_WORDS and the
// `avail` words that exist. Nothing at or past w + avail is read.
MC_FN uint32_t mc_span(const uint32_t* w, uint32_t avail) {
    if (avail < 7) return 0;
    const uint32_t nd = w[1];
    // the denominator's count sits at 4 + nd, its high word at 5 + nd
    if (w[2] != 0 || nd > MC_MAX_WORDS - 7 || nd + 7 > avail) return 0;
    const uint32_t dd = w[4 + nd];
    if (w[5 + nd] != 0 || dd < 1 || dd > MC_MAX_WORDS - 6 - nd) return 0;
    const uint32_t len = 6 + nd + dd;
    return len <= avail ? len : 0;
}

// +-m * 2^e (m odd, non-zero) as a T, or false where no T has that value
MC_FN bool mc_compose(uint64_t m, int e, bool neg, float* out) {
    const int mbits = 64 - __builtin_clzll(m), top = e + mbits - 1;
    if (mbits > 24 || e < -149 || top > 127) return false;
    uint32_t bits = neg ? 0x80000000u : 0u;
    if (top >= -126)
        bits |= (uint32_t(top + 127) << 23) | ((uint32_t(m) << (24 - mbits)) & 0x7fffffu);
    else
        bits |= uint32_t(m) << (e + 149);  // subnormal
    memcpy(out, &bits, sizeof bits);
    return true;
}

MC_FN bool mc_compose(uint64_t m, int e, bool neg, double* out) {
    const int mbits = 64 - __builtin_clzll(m), top = e + mbits - 1;
    if (mbits > 53 || e < -1074 || top > 1023) return false;
    uint64_t bits = neg ? uint64_t(1) << 63 : 0;
    if (top >= -1022)
        bits |= (uint64_t(top + 1023) << 52) | ((m << (53 - mbits)) & ((uint64_t(1) << 52) - 1));
    else
        bits |= m << (e + 1074);
    memcpy(out, &bits, sizeof bits);
    return true;
}

// the magnitude m << e must stay at or below 2^63 (2^31); only the negative
// value reaches it
MC_FN bool mc_compose(uint64_t m, int e, bool neg, int64_t* out) {
    const int mbits = 64 - __builtin_clzll(m);
    if (e < 0 || e + mbits > 64) return false;
    const uint64_t mag = m << e;
    if (mag > (uint64_t(1) << 63) || (!neg && mag == (uint64_t(1) << 63))) return false;
    *out = int64_t(neg ? uint64_t(0) - mag : mag);
    return true;
}

MC_FN bool mc_compose(uint64_t m, int e, bool neg, int32_t* out) {
    const int mbits = 64 - __builtin_clzll(m);
    if (e < 0 || e + mbits > 32) return false;
    const uint64_t mag = m << e;
    if (mag > (uint64_t(1) << 31) || (!neg && mag == (uint64_t(1) << 31))) return false;
    *out = int32_t(uint32_t(neg ? uint64_t(0) - mag : mag));
    return true;
}

// True exactly when the len words at w are the canonical element of some T:
// what mc_write gives for mc_decompose of that value, which *out then is (+0
// for the zero element). Reads w[0..len) only.
template <typename T>
MC_FN bool mc_read(const uint32_t* w, uint32_t len, T* out) {
    if (len < 7 || len > MC_MAX_WORDS) return false;
    const uint32_t sign = w[0], nd = w[1];
    if (w[2] != 0 || nd > len - 7) return false;
    const uint32_t dd = w[4 + nd];
    // a Plus denominator of exactly the remaining words, no leading zero
    if (w[3 + nd] != 2 || w[5 + nd] != 0 || dd != len - 6 - nd) return false;
    const uint32_t* num = w + 3;
    const uint32_t* den = w + 6 + nd;
    const uint32_t dtop = den[dd - 1];
    if (dtop == 0 || (dtop & (dtop - 1)) != 0) return false;  // one bit
    for (uint32_t i = 0; i + 1 < dd; ++i)
        if (den[i] != 0) return false;
    const uint32_t k = 32 * (dd - 1) + uint32_t(__builtin_ctz(dtop));  // denominator 2^k
    if (sign == 1) {  // NoSign: the zero element, 0 / 1
        if (nd != 0 || k != 0) return false;
        *out = T(0);
        return true;
    }
    if ((sign != 0 && sign != 2) || nd == 0 || num[nd - 1] == 0) return false;
    uint64_t m;
    int e;
    if (k == 0) {
        // an integer m << e: zero digits, then m across up to three digits
        uint32_t z = 0;
        while (num[z] == 0) ++z;  // ends: the top digit is not zero
        const uint32_t tz = uint32_t(__builtin_ctz(num[z]));
        const int bits = 32 * int(nd - 1) + 32 - __builtin_clz(num[nd - 1]);
        e = int(32 * z + tz);
        if (bits - e > 64) return false;
        const uint64_t lo = uint64_t(num[z]) | (z + 1 < nd ? uint64_t(num[z + 1]) << 32 : 0);
        const uint64_t hi = z + 2 < nd ? num[z + 2] : 0;
        m = tz ? (lo >> tz) | (hi << (64 - tz)) : lo;
    } else {
        // reduced: an odd numerator of at most two digits
        if (nd > 2 || (num[0] & 1u) == 0) return false;
        m = uint64_t(num[0]) | (nd == 2 ? uint64_t(num[1]) << 32 : 0);
        e = -int(k);
    }
    return mc_compose(m, e, sign == 0, out);
}
