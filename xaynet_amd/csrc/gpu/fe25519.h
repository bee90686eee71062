// X25519 and the sealed-box nonce: the arithmetic the K9 kernels (kernels.hip)
// and the host (x25519_host / seal_nonce_host in core_bindings.cpp) share, so
// it compiles as plain C++ like box_stream.h. No secret-dependent branch or
// index anywhere: the ladder swaps by mask and reads its scalar through a
// shift register, every loop bound is a constant.
//
// No low-order-point rejection: a point of small order gives the all-zero
// shared secret and this code returns it, as crypto::x25519 does and as
// crypto::box_beforenm accepts it. The device path has to produce the bytes
// of the host path, so it must not reject what the host path takes.
//
// Field elements of GF(2^255 - 19) are ten limbs in u32, even limbs 26 bits
// and odd limbs 25 (limb i sits on bit ceil(25.5 * i)). Bounds, in the terms
// used below:
//   reduced: even limbs < 2^26, odd limbs < 2^25, limb 1 < 2^25 + 2^18.
//            What fe_mul, fe_sq, fe_mul121665 and fe_frombytes return.
//   loose:   even limbs <= 3 * 2^26, odd limbs <= 3 * 2^25 + 2^18. What
//            fe_add and fe_sub make of reduced inputs, and what the
//            multiplications take.
// A product of loose inputs: one factor is at most doubled (odd x odd limb) or
// quadrupled (the square's 2 * doubled), the other at most 19-fold, both still
// u32 (19 * 3 * 2^26 < 2^32); a term is below 2^28.6 * 2^31.9 and a limb sums
// at most ten of them, below 2^64.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define FE_FN __host__ __device__ __forceinline__
#else
#define FE_FN inline
#endif

struct fe25519 {
    uint32_t v[10];
};

FE_FN constexpr int fe_bits(int i) { return (i & 1) ? 25 : 26; }
FE_FN constexpr uint32_t fe_mask(int i) { return (1u << fe_bits(i)) - 1u; }
// the bit limb i starts on: 0, 26, 51, 77, 102, 128, 153, 179, 204, 230
FE_FN constexpr int fe_offset(int i) { return (51 * i + 1) / 2; }

FE_FN fe25519 fe_zero() { return fe25519{{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}}; }
FE_FN fe25519 fe_one() { return fe25519{{1, 0, 0, 0, 0, 0, 0, 0, 0, 0}}; }

// reduced + reduced -> loose
FE_FN fe25519 fe_add(const fe25519& a, const fe25519& b) {
    fe25519 o;
#pragma unroll
    for (int i = 0; i < 10; ++i) o.v[i] = a.v[i] + b.v[i];
    return o;
}

// a - b for reduced a, b: a + 2p - b limb by limb, never negative -> loose
FE_FN fe25519 fe_sub(const fe25519& a, const fe25519& b) {
    fe25519 o;
    o.v[0] = a.v[0] + 0x7ffffdau - b.v[0];  // 2 * (2^26 - 19)
#pragma unroll
    for (int i = 1; i < 10; ++i) o.v[i] = a.v[i] + 2u * fe_mask(i) - b.v[i];
    return o;
}

// ten u64 columns (each below 2^63.5) -> reduced
FE_FN fe25519 fe_carry(uint64_t h[10]) {
    fe25519 o;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        h[i + 1] += h[i] >> fe_bits(i);
        o.v[i] = uint32_t(h[i]) & fe_mask(i);
    }
    const uint64_t f = uint64_t(o.v[0]) + 19u * (h[9] >> 25);  // below 2^44
    o.v[9] = uint32_t(h[9]) & fe_mask(9);
    o.v[0] = uint32_t(f) & fe_mask(0);
    o.v[1] += uint32_t(f >> 26);
    return o;
}

// loose * loose -> reduced. f_i * g_j lands on limb (i + j) mod 10, doubled
// where both limbs are odd (25.5-bit steps), times 19 where it wraps.
FE_FN fe25519 fe_mul(const fe25519& f, const fe25519& g) {
    uint32_t g19[10], f2[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        g19[i] = 19u * g.v[i];
        f2[i] = 2u * f.v[i];
    }
    uint64_t h[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const uint32_t a = (i & j & 1) ? f2[i] : f.v[i];
            const uint32_t b = i + j >= 10 ? g19[j] : g.v[j];
            h[(i + j) % 10] += uint64_t(a) * b;
        }
    return fe_carry(h);
}

// loose^2 -> reduced: fe_mul(f, f) with the symmetric terms taken once
FE_FN fe25519 fe_sq(const fe25519& f) {
    uint32_t f19[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) f19[i] = 19u * f.v[i];
    uint64_t h[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int j = i; j < 10; ++j) {
            const uint32_t a = f.v[i] << ((i != j ? 1 : 0) + (i & j & 1));
            const uint32_t b = i + j >= 10 ? f19[j] : f.v[j];
            h[(i + j) % 10] += uint64_t(a) * b;
        }
    return fe_carry(h);
}

// loose * 121665 = (486662 - 2) / 4 -> reduced
FE_FN fe25519 fe_mul121665(const fe25519& f) {
    uint64_t h[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) h[i] = uint64_t(f.v[i]) * 121665u;
    return fe_carry(h);
}

// swap a and b where bit is 1, by mask
FE_FN void fe_cswap(fe25519& a, fe25519& b, uint32_t bit) {
    const uint32_t m = 0u - bit;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t t = m & (a.v[i] ^ b.v[i]);
        a.v[i] ^= t;
        b.v[i] ^= t;
    }
}

// 32 bytes as little-endian words -> reduced. Bit 255 is ignored and a value
// of p or more is taken as it is (RFC 7748: reduced by the arithmetic).
FE_FN fe25519 fe_frombytes(const uint32_t w[8]) {
    fe25519 o;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const int at = fe_offset(i), k = at / 32;
        const uint64_t two = uint64_t(w[k]) | (k < 7 ? uint64_t(w[k < 7 ? k + 1 : 7]) << 32 : 0);
        o.v[i] = uint32_t(two >> (at % 32)) & fe_mask(i);
    }
    return o;
}

// loose -> the canonical 32 bytes: the value mod p, in [0, p)
FE_FN void fe_tobytes(uint32_t w[8], const fe25519& f) {
    uint32_t h[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) h[i] = f.v[i];
    // two carry rounds: the first leaves limb 0 below 2^26 + 2^9, the second
    // every limb under its mask (a second wrap means the rest was all ones
    // and is now zero, so + 19 stays under the mask)
#pragma unroll
    for (int round = 0; round < 2; ++round) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            h[i + 1] += h[i] >> fe_bits(i);
            h[i] &= fe_mask(i);
        }
        h[0] += 19u * (h[9] >> 25);
        h[9] &= fe_mask(9);
    }
    // q = 1 iff h + 19 reaches 2^255, i.e. h >= p; then h + 19 - 2^255 = h - p
    uint32_t q = (h[0] + 19u) >> 26;
#pragma unroll
    for (int i = 1; i < 10; ++i) q = (h[i] + q) >> fe_bits(i);
    h[0] += 19u * q;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        h[i + 1] += h[i] >> fe_bits(i);
        h[i] &= fe_mask(i);
    }
    h[9] &= fe_mask(9);  // drops q * 2^255
    uint64_t acc = 0;
    int have = 0, k = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        acc |= uint64_t(h[i]) << have;
        have += fe_bits(i);
        if (have >= 32) {
            w[k++] = uint32_t(acc);
            acc >>= 32;
            have -= 32;
        }
    }
    w[7] = uint32_t(acc);  // 255 bits: seven whole words and 31 bits
}

FE_FN fe25519 fe_sq_times(fe25519 f, int n) {
#pragma unroll 1
    for (int i = 0; i < n; ++i) f = fe_sq(f);
    return f;
}

// z^(p - 2): 254 squarings and 11 multiplications; 0 for z = 0
FE_FN fe25519 fe_invert(const fe25519& z) {
    const fe25519 z2 = fe_sq(z);
    const fe25519 z9 = fe_mul(z, fe_sq_times(z2, 2));
    const fe25519 z11 = fe_mul(z2, z9);
    const fe25519 e5 = fe_mul(z9, fe_sq(z11));                // 2^5 - 1
    const fe25519 e10 = fe_mul(fe_sq_times(e5, 5), e5);       // 2^10 - 1
    const fe25519 e20 = fe_mul(fe_sq_times(e10, 10), e10);    // 2^20 - 1
    const fe25519 e40 = fe_mul(fe_sq_times(e20, 20), e20);    // 2^40 - 1
    const fe25519 e50 = fe_mul(fe_sq_times(e40, 10), e10);    // 2^50 - 1
    const fe25519 e100 = fe_mul(fe_sq_times(e50, 50), e50);   // 2^100 - 1
    const fe25519 e200 = fe_mul(fe_sq_times(e100, 100), e100);  // 2^200 - 1
    const fe25519 e250 = fe_mul(fe_sq_times(e200, 50), e50);  // 2^250 - 1
    return fe_mul(fe_sq_times(e250, 5), z11);                 // 2^255 - 21
}

// --------------------------------------------------------------- X25519

// out = X25519(scalar, point), RFC 7748: 32 bytes each as little-endian
// words. The scalar is clamped here. Its bits leave through the top of an
// eight-word shift register, so no step indexes by a secret or by the step
// number (a register array stays in registers).
FE_FN void fe_x25519(uint32_t out[8], const uint32_t scalar[8], const uint32_t point[8]) {
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = scalar[i];
    e[0] &= 0xfffffff8u;
    e[7] = (e[7] & 0x7fffffffu) | 0x40000000u;
    const fe25519 x1 = fe_frombytes(point);
    fe25519 x2 = fe_one(), z2 = fe_zero(), x3 = x1, z3 = fe_one();
    uint32_t swap = 0;
#pragma unroll 1
    for (int t = 254; t >= 0; --t) {
        const uint32_t bit = (e[7] >> 30) & 1u;  // bit t of the scalar
#pragma unroll
        for (int i = 7; i > 0; --i) e[i] = (e[i] << 1) | (e[i - 1] >> 31);
        e[0] <<= 1;
        swap ^= bit;
        fe_cswap(x2, x3, swap);
        fe_cswap(z2, z3, swap);
        swap = bit;
        const fe25519 A = fe_add(x2, z2), B = fe_sub(x2, z2);
        const fe25519 C = fe_add(x3, z3), D = fe_sub(x3, z3);
        const fe25519 AA = fe_sq(A), BB = fe_sq(B);
        const fe25519 DA = fe_mul(D, A), CB = fe_mul(C, B);
        const fe25519 E = fe_sub(AA, BB);
        x3 = fe_sq(fe_add(DA, CB));
        z3 = fe_mul(x1, fe_sq(fe_sub(DA, CB)));
        x2 = fe_mul(AA, BB);
        z2 = fe_mul(E, fe_add(AA, fe_mul121665(E)));
    }
    fe_cswap(x2, x3, swap);
    fe_cswap(z2, z3, swap);
    fe_tobytes(out, fe_mul(x2, fe_invert(z2)));
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = 0;
}

// ------------------------------------- BLAKE2b, the sealed-box nonce only

FE_FN uint64_t fe_rotr64(uint64_t x, int c) { return (x >> c) | (x << (64 - c)); }

#define FE_B2_G(a, b, c, d, x, y)       \
    v[a] += v[b] + (x);                 \
    v[d] = fe_rotr64(v[d] ^ v[a], 32);  \
    v[c] += v[d];                       \
    v[b] = fe_rotr64(v[b] ^ v[c], 24);  \
    v[a] += v[b] + (y);                 \
    v[d] = fe_rotr64(v[d] ^ v[a], 16);  \
    v[c] += v[d];                       \
    v[b] = fe_rotr64(v[b] ^ v[c], 63)

// one round, its message schedule spelled out so that m[] stays in registers
#define FE_B2_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
    FE_B2_G(0, 4, 8, 12, m[s0], m[s1]);                                                    \
    FE_B2_G(1, 5, 9, 13, m[s2], m[s3]);                                                    \
    FE_B2_G(2, 6, 10, 14, m[s4], m[s5]);                                                   \
    FE_B2_G(3, 7, 11, 15, m[s6], m[s7]);                                                   \
    FE_B2_G(0, 5, 10, 15, m[s8], m[s9]);                                                   \
    FE_B2_G(1, 6, 11, 12, m[s10], m[s11]);                                                 \
    FE_B2_G(2, 7, 8, 13, m[s12], m[s13]);                                                  \
    FE_B2_G(3, 4, 9, 14, m[s14], m[s15])

// nonce = BLAKE2b(epk || pk) with a 24-byte digest and no key: one block of
// exactly 64 input bytes, the second half of the block zero.
FE_FN void fe_seal_nonce(uint32_t nonce[6], const uint32_t epk[8], const uint32_t pk[8]) {
    const uint64_t iv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                            0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                            0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
    uint64_t m[16], v[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m[i] = uint64_t(epk[2 * i]) | uint64_t(epk[2 * i + 1]) << 32;
        m[4 + i] = uint64_t(pk[2 * i]) | uint64_t(pk[2 * i + 1]) << 32;
        m[8 + i] = m[12 + i] = 0;
    }
    const uint64_t h0 = iv[0] ^ 0x01010000ull ^ 24u;  // digest 24, no key, fanout = depth = 1
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = iv[i];
        v[8 + i] = iv[i];
    }
    v[0] = h0;
    v[12] ^= 64;          // bytes so far
    v[14] = ~v[14];       // the last block
    FE_B2_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    FE_B2_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    FE_B2_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4);
    FE_B2_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8);
    FE_B2_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13);
    FE_B2_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9);
    FE_B2_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11);
    FE_B2_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10);
    FE_B2_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5);
    FE_B2_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0);
    FE_B2_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    FE_B2_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    const uint64_t d0 = h0 ^ v[0] ^ v[8], d1 = iv[1] ^ v[1] ^ v[9], d2 = iv[2] ^ v[2] ^ v[10];
    nonce[0] = uint32_t(d0);
    nonce[1] = uint32_t(d0 >> 32);
    nonce[2] = uint32_t(d1);
    nonce[3] = uint32_t(d1 >> 32);
    nonce[4] = uint32_t(d2);
    nonce[5] = uint32_t(d2 >> 32);
}
