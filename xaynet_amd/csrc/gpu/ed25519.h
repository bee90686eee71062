// Ed25519 verification: the arithmetic the K10 kernels (kernels.hip) and the
// host (ed25519_verify_host and friends in core_bindings.cpp) share, over the
// field of fe25519.h and in its terms (reduced, loose). Everything a
// signature check reads is public, so nothing here is secret; branches and
// indices are still free of data, because 64 lanes run it in step.
//
// The acceptance rules are those of crypto::ed25519_verify, not the stricter
// ones of libsodium: s >= L is rejected; bit 255 of the key is the sign and
// the low 255 bits are y as given (y >= p acts as y mod p); with u = y^2 - 1
// and v = d y^2 + 1 a key is rejected where neither v x^2 = u nor v x^2 = -u,
// and where x = 0 with the sign bit set; keys and R of small order are NOT
// rejected; R is never decompressed: the canonical encoding of s B - k A is
// compared with the signature's first 32 bytes, so a non-canonical R fails.
#pragma once

#include "fe25519.h"

// ------------------------------------------------------- field additions

// loose -> reduced, one carry pass: limbs are below 2^28, so every carry is
// at most 3 (19 * 3 into limb 0, whose own carry then leaves limb 1 at most
// 2^25)
FE_FN fe25519 fe_weak(const fe25519& f) {
    fe25519 o = f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        o.v[i + 1] += o.v[i] >> fe_bits(i);
        o.v[i] &= fe_mask(i);
    }
    o.v[0] += 19u * (o.v[9] >> 25);
    o.v[9] &= fe_mask(9);
    o.v[1] += o.v[0] >> 26;
    o.v[0] &= fe_mask(0);
    return o;
}

// reduced -> loose
FE_FN fe25519 fe_neg(const fe25519& f) { return fe_sub(fe_zero(), f); }

// b where bit is 1, a where it is 0
FE_FN fe25519 fe_select(const fe25519& a, const fe25519& b, uint32_t bit) {
    const uint32_t m = 0u - bit;
    fe25519 o;
#pragma unroll
    for (int i = 0; i < 10; ++i) o.v[i] = a.v[i] ^ (m & (a.v[i] ^ b.v[i]));
    return o;
}

// z^(2^252 - 3) = z^((p - 5) / 8): the chain of fe_invert, cut short
FE_FN fe25519 fe_pow22523(const fe25519& z) {
    const fe25519 z2 = fe_sq(z);
    const fe25519 z9 = fe_mul(z, fe_sq_times(z2, 2));
    const fe25519 z11 = fe_mul(z2, z9);
    const fe25519 e5 = fe_mul(z9, fe_sq(z11));                  // 2^5 - 1
    const fe25519 e10 = fe_mul(fe_sq_times(e5, 5), e5);         // 2^10 - 1
    const fe25519 e20 = fe_mul(fe_sq_times(e10, 10), e10);      // 2^20 - 1
    const fe25519 e40 = fe_mul(fe_sq_times(e20, 20), e20);      // 2^40 - 1
    const fe25519 e50 = fe_mul(fe_sq_times(e40, 10), e10);      // 2^50 - 1
    const fe25519 e100 = fe_mul(fe_sq_times(e50, 50), e50);     // 2^100 - 1
    const fe25519 e200 = fe_mul(fe_sq_times(e100, 100), e100);  // 2^200 - 1
    const fe25519 e250 = fe_mul(fe_sq_times(e200, 50), e50);    // 2^250 - 1
    return fe_mul(fe_sq_times(e250, 2), z);                     // 2^252 - 3
}

// loose -> 1 where the value is 0 mod p
FE_FN uint32_t fe_iszero(const fe25519& f) {
    uint32_t w[8], any = 0;
    fe_tobytes(w, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) any |= w[i];
    return any == 0 ? 1u : 0u;
}

// loose -> the low bit of the canonical value ("x is negative")
FE_FN uint32_t fe_isnegative(const fe25519& f) {
    uint32_t w[8];
    fe_tobytes(w, f);
    return w[0] & 1u;
}

// d = -121665 / 121666 mod p, the curve's constant (RFC 8032, 5.1)
FE_FN fe25519 fe_d() {
    return fe25519{{0x35978a3, 0xd37284, 0x3156ebd, 0x6a0a0e, 0x1c029, 0x179e898, 0x3a03cbb,
                    0x1ce7198, 0x2e2b6ff, 0x1480db3}};
}
// 2 d mod p
FE_FN fe25519 fe_d2() {
    return fe25519{{0x2b2f159, 0x1a6e509, 0x22add7a, 0xd4141d, 0x38052, 0xf3d130, 0x3407977,
                    0x19ce331, 0x1c56dff, 0x901b67}};
}
// sqrt(-1) = 2^((p - 1) / 4) mod p
FE_FN fe25519 fe_sqrtm1() {
    return fe25519{{0x20ea0b0, 0x186c9d2, 0x8f189d, 0x35697f, 0xbd0c60, 0x1fbd7a7, 0x2804c9e,
                    0x1e16569, 0x4fc1d, 0xae0c92}};
}

// ------------------------------- points on -x^2 + y^2 = 1 + d x^2 y^2

// Extended: x = X / Z, y = Y / Z, x y = T / Z. Coordinates are reduced.
struct ge_ext {
    fe25519 X, Y, Z, T;
};
// Completed, what a doubling or an addition leaves: the point is
// (X T : Y Z : Z T : X Y) in extended terms. Coordinates are loose.
struct ge_p1p1 {
    fe25519 X, Y, Z, T;
};
// Cached (Y + X, Y - X, Z, 2 d T) and affine precomputed (y + x, y - x,
// 2 d x y): the second operand of an addition. Reduced in a table; loose after
// ge_signed.
struct ge_cached {
    fe25519 ypx, ymx, z, t2d;
};
struct ge_pre {
    fe25519 ypx, ymx, xy2d;
};

FE_FN ge_ext ge_identity() { return ge_ext{fe_zero(), fe_one(), fe_one(), fe_zero()}; }

// 3 multiplications, T left out (a doubling does not read it), or 4
FE_FN ge_ext ge_complete(const ge_p1p1& p, bool with_t) {
    ge_ext r;
    r.X = fe_mul(p.X, p.T);
    r.Y = fe_mul(p.Y, p.Z);
    r.Z = fe_mul(p.Z, p.T);
    r.T = with_t ? fe_mul(p.X, p.Y) : fe_zero();
    return r;
}

// 2 P from (X : Y : Z), 4 squarings; with ge_complete's 4 multiplications the
// doubling. A = X^2, B = Y^2, C = 2 Z^2, all reduced; B + A and B - A are
// loose. (X + Y)^2 - (B + A) hands fe_sub a loose subtrahend, and so does
// C - (B - A): a weak carry on B + A and on C + A (limbs at most 3 * 2^26,
// loose) makes both operands reduced, the latter taken as (C + A) - B.
FE_FN ge_p1p1 ge_dbl(const ge_ext& p) {
    const fe25519 A = fe_sq(p.X), B = fe_sq(p.Y), ZZ = fe_sq(p.Z);
    const fe25519 S = fe_sq(fe_add(p.X, p.Y));
    ge_p1p1 r;
    r.Y = fe_weak(fe_add(B, A));
    r.Z = fe_sub(B, A);
    r.X = fe_sub(S, r.Y);
    r.T = fe_sub(fe_weak(fe_add(fe_add(ZZ, ZZ), A)), B);
    return r;
}

// P + Q for Q = (ypx, ymx, t2d) over the denominator product zz (reduced):
// Z1 * Z2 for a cached Q, Z1 itself for an affine one. P - Q is the same with
// ypx and ymx swapped and t2d negated (ge_signed). 2 zz + C has limbs of at
// most 3 * 2^26, loose; 2 zz - C would reach 4 * 2^26, so 2 zz gets a weak
// carry first.
FE_FN ge_p1p1 ge_add_core(const ge_ext& p, const fe25519& ypx, const fe25519& ymx,
                          const fe25519& t2d, const fe25519& zz) {
    const fe25519 A = fe_mul(fe_add(p.Y, p.X), ypx);
    const fe25519 B = fe_mul(fe_sub(p.Y, p.X), ymx);
    const fe25519 C = fe_mul(t2d, p.T);
    const fe25519 D = fe_add(zz, zz);
    ge_p1p1 r;
    r.X = fe_sub(A, B);
    r.Y = fe_add(A, B);
    r.Z = fe_add(D, C);
    r.T = fe_sub(fe_weak(D), C);
    return r;
}

FE_FN ge_p1p1 ge_add(const ge_ext& p, const ge_cached& q) {  // 8 multiplications
    return ge_add_core(p, q.ypx, q.ymx, q.t2d, fe_mul(p.Z, q.z));
}
FE_FN ge_p1p1 ge_madd(const ge_ext& p, const ge_pre& q) {  // 7
    return ge_add_core(p, q.ypx, q.ymx, q.xy2d, p.Z);
}

// extended (reduced) -> cached (reduced)
FE_FN ge_cached ge_to_cached(const ge_ext& p) {
    return ge_cached{fe_weak(fe_add(p.Y, p.X)), fe_weak(fe_sub(p.Y, p.X)), p.Z,
                     fe_mul(p.T, fe_d2())};
}

// The table entry of |digit| as the operand of digit: swapped and negated
// where neg is 1, the identity where zero is 1. By mask, never by branch.
FE_FN void ge_signed(fe25519& ypx, fe25519& ymx, fe25519& t2d, uint32_t neg, uint32_t zero) {
    fe_cswap(ypx, ymx, neg);
    t2d = fe_select(t2d, fe_neg(t2d), neg);
    ypx = fe_select(ypx, fe_one(), zero);
    ymx = fe_select(ymx, fe_one(), zero);
    t2d = fe_select(t2d, fe_zero(), zero);
}

// -P, coordinates reduced again
FE_FN ge_ext ge_neg(const ge_ext& p) {
    return ge_ext{fe_weak(fe_neg(p.X)), p.Y, p.Z, fe_weak(fe_neg(p.T))};
}

// 32 key bytes -> the point, 1 where it is one (the rules at the top). Where
// it is none the coordinates are field elements all the same, so a lane goes
// on computing and only its flag says no.
FE_FN uint32_t ge_decompress(ge_ext& p, const uint32_t w[8]) {
    const fe25519 y = fe_frombytes(w);
    const fe25519 y2 = fe_sq(y);
    const fe25519 u = fe_weak(fe_sub(y2, fe_one()));
    const fe25519 v = fe_weak(fe_add(fe_mul(fe_d(), y2), fe_one()));
    const fe25519 v3 = fe_mul(fe_sq(v), v);
    const fe25519 v7 = fe_mul(fe_sq(v3), v);
    fe25519 x = fe_mul(fe_mul(u, v3), fe_pow22523(fe_mul(u, v7)));  // u v^3 (u v^7)^((p-5)/8)
    const fe25519 vx2 = fe_mul(v, fe_sq(x));
    const uint32_t plus = fe_iszero(fe_sub(vx2, u));   // v x^2 = u
    const uint32_t minus = fe_iszero(fe_add(vx2, u));  // v x^2 = -u: x *= sqrt(-1)
    x = fe_select(fe_mul(x, fe_sqrtm1()), x, plus);
    const uint32_t sign = w[7] >> 31;
    const uint32_t flip = fe_isnegative(x) ^ sign;
    const uint32_t ok = (plus | minus) & (1u ^ (fe_iszero(x) & sign));
    p.X = fe_weak(fe_select(x, fe_neg(x), flip));
    p.Y = y;
    p.Z = fe_one();
    p.T = fe_mul(p.X, y);
    return ok;
}

// (X : Y : Z) -> the canonical 32 bytes: y, and the low bit of x on top
FE_FN void ge_compress(uint32_t w[8], const ge_ext& p) {
    const fe25519 zi = fe_invert(p.Z);
    fe_tobytes(w, fe_mul(p.Y, zi));
    w[7] |= fe_isnegative(fe_mul(p.X, zi)) << 31;
}

// ---------------------------------------------------------------- scalars

// L = 2^252 + 27742317777372353535851937790883648493, the group's order
FE_FN constexpr uint32_t sc_l(int i) {
    return i == 0 ? 0x5cf5d3edu : i == 1 ? 0x5812631au : i == 2 ? 0xa2f79cd6u
         : i == 3 ? 0x14def9deu : i == 7 ? 0x10000000u : 0u;
}
// floor(2^512 / L), nine words: Barrett's constant for 32-bit limbs and k = 8
FE_FN constexpr uint32_t sc_mu(int i) {
    return i == 0 ? 0x0a2c131bu : i == 1 ? 0xed9ce5a3u : i == 2 ? 0x086329a7u
         : i == 3 ? 0x2106215du : i == 4 ? 0xffffffebu : i == 8 ? 0xfu : 0xffffffffu;
}

// r - L over nine words (the ninth of L is 0) where that is not negative;
// returns 1 where r < L and r stays
FE_FN uint32_t sc_sub_l(uint32_t r[9]) {
    uint32_t t[9];
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const uint64_t d = uint64_t(r[i]) - (i < 8 ? sc_l(i) : 0u) - borrow;
        t[i] = uint32_t(d);
        borrow = (d >> 32) & 1u;
    }
    const uint32_t keep = 0u - uint32_t(borrow);
#pragma unroll
    for (int i = 0; i < 9; ++i) r[i] = (r[i] & keep) | (t[i] & ~keep);
    return uint32_t(borrow);
}

// s < L, for 32 bytes as little-endian words
FE_FN uint32_t sc_is_canonical(const uint32_t s[8]) {
    uint32_t r[9];
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = s[i];
    r[8] = 0;
    return sc_sub_l(r);
}

// 64 bytes (sixteen little-endian words) -> the value mod L in [0, L).
// Barrett's reduction (Handbook of Applied Cryptography 14.42) with b = 2^32
// and k = 8: q3 = floor(floor(x / b^7) mu / b^9) is the quotient or up to 2
// below it, so x - q3 L, taken mod b^9, is below 3 L and two conditional
// subtractions finish. Row products: a * b + word + carry fits a u64.
FE_FN void sc_reduce512(uint32_t out[8], const uint32_t x[16]) {
    uint32_t q2[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) q2[i] = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const uint64_t t = uint64_t(x[7 + i]) * sc_mu(j) + q2[i + j] + carry;
            q2[i + j] = uint32_t(t);
            carry = t >> 32;
        }
        q2[i + 9] = uint32_t(carry);
    }
    uint32_t r2[9];  // q3 * L mod b^9, q3 = q2[9..17]
#pragma unroll
    for (int i = 0; i < 9; ++i) r2[i] = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (i + j < 9) {
                const uint64_t t = uint64_t(q2[9 + i]) * sc_l(j) + r2[i + j] + carry;
                r2[i + j] = uint32_t(t);
                carry = t >> 32;
            }
        }
        if (i == 0) r2[8] = uint32_t(carry);
    }
    uint32_t r[9];
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const uint64_t d = uint64_t(x[i]) - r2[i] - borrow;
        r[i] = uint32_t(d);
        borrow = (d >> 32) & 1u;
    }
    sc_sub_l(r);
    sc_sub_l(r);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = r[i];
}

// A scalar below 2^253 as 64 signed radix-16 digits, digit i in nibble i of
// the eight words as a 4-bit two's complement: digits 0..62 in [-8, 7], the
// top one in [0, 2], so no overflow digit. A larger scalar gives digits that
// mean nothing but are digits all the same.
FE_FN void sc_recode(uint32_t d[8], const uint32_t s[8]) {
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t n = ((s[w] >> (4 * j)) & 15u) + carry;
            carry = (w == 7 && j == 7) ? 0u : (n + 8u) >> 4;
            o |= (n & 15u) << (4 * j);
        }
        d[w] = o;
    }
}

// The top digit of d as (|digit|, digit < 0), and d moved up one digit, so
// that the window loop indexes nothing by its counter.
FE_FN void sc_next_digit(uint32_t d[8], uint32_t& mag, uint32_t& neg) {
    const uint32_t n = d[7] >> 28;
    neg = n >> 3;
    mag = neg ? 16u - n : n;
#pragma unroll
    for (int i = 7; i > 0; --i) d[i] = (d[i] << 4) | (d[i - 1] >> 28);
    d[0] <<= 4;
}

// ---------------------------------------------------------------- SHA-512

FE_FN uint32_t ed_bswap32(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}

FE_FN void sha512_init(uint64_t h[8]) {
    h[0] = 0x6a09e667f3bcc908ull, h[1] = 0xbb67ae8584caa73bull;
    h[2] = 0x3c6ef372fe94f82bull, h[3] = 0xa54ff53a5f1d36f1ull;
    h[4] = 0x510e527fade682d1ull, h[5] = 0x9b05688c2b3e6c1full;
    h[6] = 0x1f83d9abfb41bd6bull, h[7] = 0x5be0cd19137e2179ull;
}

#define ED_SHA_ROUND(a, b, c, d, e, f, g, h, i)                                                \
    {                                                                                          \
        if (t16) {                                                                             \
            const uint64_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];                       \
            w[i] += (fe_rotr64(w15, 1) ^ fe_rotr64(w15, 8) ^ (w15 >> 7)) + w[(i + 9) & 15] +   \
                    (fe_rotr64(w2, 19) ^ fe_rotr64(w2, 61) ^ (w2 >> 6));                       \
        }                                                                                      \
        const uint64_t t1 = h + (fe_rotr64(e, 14) ^ fe_rotr64(e, 18) ^ fe_rotr64(e, 41)) +     \
                            ((e & f) ^ (~e & g)) + K[t16 + i] + w[i];                          \
        const uint64_t t2 = (fe_rotr64(a, 28) ^ fe_rotr64(a, 34) ^ fe_rotr64(a, 39)) +         \
                            ((a & b) ^ (a & c) ^ (b & c));                                     \
        d += t1;                                                                               \
        h = t1 + t2;                                                                           \
    }

// One block: the sixteen big-endian words w (used up as the schedule's window)
// into the state. The words and the eight working variables stay in registers:
// sixteen rounds are written out, so every index into w is a constant.
FE_FN void sha512_compress(uint64_t st[8], uint64_t w[16]) {
    static constexpr uint64_t K[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
        0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
        0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
        0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
        0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
        0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
        0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
        0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
        0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
        0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
        0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
        0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
        0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
        0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
        0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
        0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
        0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
        0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
        0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
        0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
    uint64_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll 1
    for (int t16 = 0; t16 < 80; t16 += 16) {
        ED_SHA_ROUND(a, b, c, d, e, f, g, h, 0)
        ED_SHA_ROUND(h, a, b, c, d, e, f, g, 1)
        ED_SHA_ROUND(g, h, a, b, c, d, e, f, 2)
        ED_SHA_ROUND(f, g, h, a, b, c, d, e, 3)
        ED_SHA_ROUND(e, f, g, h, a, b, c, d, 4)
        ED_SHA_ROUND(d, e, f, g, h, a, b, c, 5)
        ED_SHA_ROUND(c, d, e, f, g, h, a, b, 6)
        ED_SHA_ROUND(b, c, d, e, f, g, h, a, 7)
        ED_SHA_ROUND(a, b, c, d, e, f, g, h, 8)
        ED_SHA_ROUND(h, a, b, c, d, e, f, g, 9)
        ED_SHA_ROUND(g, h, a, b, c, d, e, f, 10)
        ED_SHA_ROUND(f, g, h, a, b, c, d, e, 11)
        ED_SHA_ROUND(e, f, g, h, a, b, c, d, 12)
        ED_SHA_ROUND(d, e, f, g, h, a, b, c, 13)
        ED_SHA_ROUND(c, d, e, f, g, h, a, b, 14)
        ED_SHA_ROUND(b, c, d, e, f, g, h, a, 15)
    }
    st[0] += a, st[1] += b, st[2] += c, st[3] += d;
    st[4] += e, st[5] += f, st[6] += g, st[7] += h;
}

// blocks of a message of `total` bytes: the 0x80 and the 16-byte length fit
FE_FN uint64_t sha512_blocks(uint64_t total) { return (total + 17 + 127) / 128; }

// Block `block` of a message of `total` bytes, its 128 bytes given as 32
// little-endian words m in memory order -> the sixteen words compress takes.
// Whatever m holds from byte `total` on is dropped, the 0x80 goes in where it
// falls, and the last block ends in the bit length; a block wholly inside the
// message passes through. All by masks: lanes at different lengths agree.
FE_FN void sha512_block_words(uint64_t w[16], const uint32_t m[32], uint64_t block,
                              uint64_t total) {
    const int64_t left0 = int64_t(total) - int64_t(128 * block);  // message bytes from here on
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        uint32_t half[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t left = left0 - 4 * (2 * i + j);
            const uint32_t sh = 8u * uint32_t(left & 3);
            const uint32_t keep = left >= 4 ? 0xffffffffu : left <= 0 ? 0u : (1u << sh) - 1u;
            const uint32_t mark = (left >= 0 && left < 4) ? 0x80u << sh : 0u;
            half[j] = ed_bswap32((m[2 * i + j] & keep) | mark);
        }
        w[i] = uint64_t(half[0]) << 32 | half[1];
    }
    if (block + 1 == sha512_blocks(total)) w[15] = total * 8;  // total < 2^33: w[14] stays 0
}

// The digest's 64 bytes as the sixteen little-endian words sc_reduce512 takes
FE_FN void sha512_digest_words(uint32_t out[16], const uint64_t st[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        out[2 * i] = ed_bswap32(uint32_t(st[i] >> 32));
        out[2 * i + 1] = ed_bswap32(uint32_t(st[i]));
    }
}

// ------------------------------------------------------------ the check

// The multiples 1..8 of P, cached: put(e, c) takes entry e = multiple - 1.
template <class Put>
FE_FN void ge_table8(const ge_ext& p, Put&& put) {
    const ge_cached c1 = ge_to_cached(p);
    put(0, c1);
    ge_ext q = ge_complete(ge_dbl(p), true);
    put(1, ge_to_cached(q));
#pragma unroll 1
    for (int e = 2; e < 8; ++e) {
        q = ge_complete(ge_add(q, c1), true);
        put(e, ge_to_cached(q));
    }
}

// s B + k Q for recoded s and k (both used up), Q's table behind cached(e) and
// B's behind base(e), e = |digit| - 1 in 0..7. 64 windows from the top: four
// doublings, then +-B[|s_i|] and +-Q[|k_i|]. Returns (X : Y : Z); T is not
// kept.
template <class Base, class Cached>
FE_FN ge_ext ge_double_scalarmult(uint32_t sd[8], uint32_t kd[8], Base&& base, Cached&& cached) {
    ge_ext r = ge_identity();
#pragma unroll 1
    for (int i = 0; i < 64; ++i) {
        r = ge_complete(ge_dbl(r), false);
        r = ge_complete(ge_dbl(r), false);
        r = ge_complete(ge_dbl(r), false);
        r = ge_complete(ge_dbl(r), true);
        uint32_t mag, neg;
        sc_next_digit(sd, mag, neg);
        ge_pre b = base(mag == 0 ? 0u : mag - 1u);
        ge_signed(b.ypx, b.ymx, b.xy2d, neg, mag == 0 ? 1u : 0u);
        r = ge_complete(ge_madd(r, b), true);
        sc_next_digit(kd, mag, neg);
        ge_cached q = cached(mag == 0 ? 0u : mag - 1u);
        ge_signed(q.ypx, q.ymx, q.t2d, neg, mag == 0 ? 1u : 0u);
        q.z = fe_select(q.z, fe_one(), mag == 0 ? 1u : 0u);
        r = ge_complete(ge_add(r, q), false);
    }
    return r;
}

// encode(s B - k A) == R and every rule at the top: sig is R || s, pk the key,
// k = SHA-512(R || A || M) mod L. put / cached write and read the table of -A.
template <class Base, class Put, class Cached>
FE_FN uint32_t ed_check(const uint32_t sig[16], const uint32_t pk[8], const uint32_t k[8],
                        Base&& base, Put&& put, Cached&& cached) {
    uint32_t ok = sc_is_canonical(sig + 8);
    ge_ext A;
    ok &= ge_decompress(A, pk);
    ge_table8(ge_neg(A), put);
    uint32_t sd[8], kd[8], enc[8];
    sc_recode(sd, sig + 8);
    sc_recode(kd, k);
    ge_compress(enc, ge_double_scalarmult(sd, kd, base, cached));
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) diff |= enc[i] ^ sig[i];
    return ok & (diff == 0 ? 1u : 0u);
}

// ---------------------------------------------------- host only: B's table

// 1 B .. 8 B as affine precomputed (y + x, y - x, 2 d x y), 30 words an entry:
// computed by the arithmetic above from y = 4 / 5 and the even x. The K10
// launcher uploads these 240 words; the host check reads them in place.
inline const uint32_t* ed_base_table() {
    static const struct Table {
        uint32_t w[240];
        Table() {
            const fe25519 four{{4, 0, 0, 0, 0, 0, 0, 0, 0, 0}}, five{{5, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
            uint32_t yb[8];
            fe_tobytes(yb, fe_mul(four, fe_invert(five)));  // sign bit 0: the even x
            ge_ext b;
            ge_decompress(b, yb);
            ge_table8(b, [&](int e, const ge_cached& c) {
                const fe25519 zi = fe_invert(c.z);  // (Y + X) / Z = y + x, ...
                const fe25519 col[3] = {fe_mul(c.ypx, zi), fe_mul(c.ymx, zi), fe_mul(c.t2d, zi)};
                for (int f = 0; f < 3; ++f)
                    for (int i = 0; i < 10; ++i) w[30 * e + 10 * f + i] = col[f].v[i];
            });
        }
    } table;
    return table.w;
}

// The whole check on the host, as the two kernels divide it: k10_hram's
// hash and reduction, then ed_check over tables in plain arrays.
inline bool ed25519_verify_host(const uint8_t sig[64], const uint8_t* msg, uint64_t len,
                                const uint8_t pk[32]) {
    uint32_t sw[16], pw[8], k[8], digest[16];
    std::memcpy(sw, sig, 64);
    std::memcpy(pw, pk, 32);
    const uint64_t total = len + 64;
    uint64_t st[8], w[16];
    sha512_init(st);
    for (uint64_t b = 0; b < sha512_blocks(total); ++b) {
        uint8_t bytes[128] = {};
        for (uint64_t i = 0; i < 128; ++i) {
            const uint64_t at = 128 * b + i;
            if (at < 32) bytes[i] = sig[at];
            else if (at < 64) bytes[i] = pk[at - 32];
            else if (at < total) bytes[i] = msg[at - 64];
        }
        uint32_t m[32];
        std::memcpy(m, bytes, 128);
        sha512_block_words(w, m, b, total);
        sha512_compress(st, w);
    }
    sha512_digest_words(digest, st);
    sc_reduce512(k, digest);
    const uint32_t* bt = ed_base_table();
    ge_cached table[8];
    auto base = [&](uint32_t e) {
        ge_pre q;
        for (int i = 0; i < 10; ++i) {
            q.ypx.v[i] = bt[30 * e + i];
            q.ymx.v[i] = bt[30 * e + 10 + i];
            q.xy2d.v[i] = bt[30 * e + 20 + i];
        }
        return q;
    };
    return ed_check(sw, pw, k, base, [&](int e, const ge_cached& c) { table[e] = c; },
                    [&](uint32_t e) { return table[e]; }) != 0;
}
