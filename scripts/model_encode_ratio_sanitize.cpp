// Stand-alone sanitizer pass over the rational model encoder's element
// functions (ml_gcd, ml_div_exact_odd in xaynet_amd/csrc/gpu/limbs.h;
// mc_ratio_words / mc_ratio_write in xaynet_amd/csrc/gpu/model_codec.h), the
// source the K7r kernels compile. Host only. Build and run on the CPU, from
// the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ixaynet_amd/csrc scripts/model_encode_ratio_sanitize.cpp \
//       -o build/model_encode_ratio_sanitize
//   build/model_encode_ratio_sanitize
//
// Every element is written into a heap allocation of exactly mc_ratio_words
// words, so a word past the count is an AddressSanitizer error, and every
// shift of the gcd and the division runs under UBSan. Per L = 1..5: the cases
// of tests/test_model_encode_ratio_cpu.py (0, +-1, +-Q, +-3Q, a coprime pair,
// common factors 2^k and odd, a top limb with a zero high half, a one-digit
// and a full-width Q, the largest magnitude) and seeded random pairs of every
// bit length. Checked here without a second implementation: the element
// parses back to num / den with num * Q == mag * den and gcd(num, den) == 1.
// Equality with Fraction is the Python test's part.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpu/model_codec.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 2685821657736338717ull;
}

// a * b on 2L limbs
template <int L>
static limbs<2 * L> mul(const limbs<L>& a, const limbs<L>& b) {
    limbs<2 * L> r = ml_zero<2 * L>();
    for (int j = 0; j < L; ++j) {
        limbs<2 * L> part = ml_resize<2 * L>(ml_mul_word(ml_resize<L + 1>(a), b.w[j]));
        for (int k = 0; k < j; ++k) ml_shl_limb(part);
        ml_add(r, part);
    }
    return r;
}

template <int L>
static bool same(const limbs<L>& a, const limbs<L>& b) {
    for (int j = 0; j < L; ++j)
        if (a.w[j] != b.w[j]) return false;
    return true;
}

// `bits` random bits, the top one set; bits == 0 is zero
template <int L>
static limbs<L> random_limbs(int bits) {
    limbs<L> r = ml_zero<L>();
    if (bits == 0) return r;
    for (int j = 0; j < L; ++j) r.w[j] = rng();
    ml_shr(r, 64 * L - bits);
    limbs<L> top = ml_zero<L>();
    top.w[0] = 1;
    ml_shl(top, bits - 1);
    for (int j = 0; j < L; ++j) r.w[j] |= top.w[j];
    return r;
}

template <int L>
static int check(bool neg, const limbs<L>& mag, const limbs<L>& q) {
    const uint32_t nw = mc_ratio_words<L>(mag, q);
    if (nw < 7 || nw > 6 + 4 * L) return 1;
    uint32_t* w = static_cast<uint32_t*>(std::malloc(4 * nw));
    mc_ratio_write<L>(neg, mag, q, w);
    const uint32_t nd = w[1], dd = w[4 + nd];
    int bad = w[2] != 0 || w[5 + nd] != 0 || w[3 + nd] != 2 || 6 + nd + dd != nw || dd == 0;
    bad |= w[0] != (ml_is_zero(mag) ? 1u : neg ? 0u : 2u);
    bad |= (nd && w[2 + nd] == 0) || w[5 + nd + dd] == 0;  // no leading zero digit
    limbs<L> num = ml_zero<L>(), den = ml_zero<L>();
    for (uint32_t i = 0; i < nd; ++i) num.w[i / 2] |= uint64_t(w[3 + i]) << (32 * (i % 2));
    for (uint32_t i = 0; i < dd; ++i) den.w[i / 2] |= uint64_t(w[6 + nd + i]) << (32 * (i % 2));
    std::free(w);
    limbs<L> one = ml_zero<L>();
    one.w[0] = 1;
    bad |= !same(mul(num, q), mul(mag, den)) || !same(ml_gcd(num, den), one);
    return bad;
}

template <int L>
static int run() {
    int bad = 0;
    limbs<L> one = ml_zero<L>(), full, small = ml_zero<L>();
    one.w[0] = 1;
    small.w[0] = 5040;  // 2^4 * 3^2 * 5 * 7, one digit
    for (int j = 0; j < L; ++j) full.w[j] = ~uint64_t(0);
    full.w[0] -= 5039;  // full width
    const limbs<L> qs[3] = {small, random_limbs<L>(32 * L), full};
    for (const limbs<L>& q : qs) {
        limbs<L> q1 = q, q3 = ml_mul_word(q, 3), half = ml_zero<L>(), big = full;
        ml_add_word(q1, 1);
        half.w[L - 1] = uint64_t(1) << 20;
        half.w[0] |= 1;
        limbs<L> cases[] = {ml_zero<L>(), one, q, q1, ml_mul_word(small, 11), half, big};
        for (const limbs<L>& mag : cases)
            for (int neg = 0; neg < 2; ++neg) bad |= check<L>(neg, mag, q);
        if (ml_bits(q) + 2 <= 64 * L) bad |= check<L>(false, q3, q) | check<L>(true, q3, q);
        for (int k : {3, 33, 70}) {  // multiples of 2^k * 21 on both sides
            if (k + 5 + 32 * L > 64 * L) continue;
            limbs<L> f = ml_zero<L>();
            f.w[0] = 21;
            ml_shl(f, k);
            const limbs<L> a = ml_resize<L>(mul(f, random_limbs<L>(20)));
            const limbs<L> b = ml_resize<L>(mul(f, random_limbs<L>(32 * L - k - 5)));
            bad |= check<L>(false, a, b) | check<L>(true, b, a);
        }
    }
    for (int c = 0; c < 4000; ++c) {
        const int bm = int(rng() % (64 * L + 1)), bq = 1 + int(rng() % (64 * L));
        bad |= check<L>(rng() & 1, random_limbs<L>(bm), random_limbs<L>(bq));
    }
    std::printf("L = %d: %s\n", L, bad ? "a wrong element" : "ok");
    return bad;
}

int main() {
    int bad = run<1>();
    bad |= run<2>();
    bad |= run<3>();
    bad |= run<4>();
    bad |= run<5>();
    std::puts(bad ? "model_encode_ratio_sanitize: FAILED" : "model_encode_ratio_sanitize: OK");
    return bad;
}
