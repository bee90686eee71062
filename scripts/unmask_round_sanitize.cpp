// Stand-alone sanitizer pass over the exact float unmask's element function
// (xaynet_amd/csrc/gpu/unmask_round.h), the source k4_unmask_exact compiles.
// Build and run on the CPU, from the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ixaynet_amd/csrc scripts/unmask_round_sanitize.cpp -o build/unmask_round_sanitize
//   build/unmask_round_sanitize
//
// For float and double and every limb count L = 1..5 it calls ur_round on
// numerators and divisors of every pair of bit lengths 1..64L (so every shift
// count the function forms, the whole-limb ones and 0 and 63 included: an
// out-of-range shift is a UBSan error), on all-ones and single-bit limbs, and
// on seeded random pairs. It checks what needs no second implementation:
// the result is finite, signed as asked, +0 for a zero numerator, and
// monotonic in the numerator. Bit equality with the Fraction reference is
// tests/test_unmask_exact_cpu.py's part.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "gpu/unmask_round.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// an L-limb value of exactly `bits` significant bits (1..64L): random below
// the top bit, or all ones, or the top bit alone
template <int L>
static limbs<L> with_bits(int bits, int kind) {
    limbs<L> v = ml_zero<L>();
    for (int j = 0; j < L; ++j) {
        const int lo = 64 * j;
        if (bits <= lo) break;
        const int here = bits - lo >= 64 ? 64 : bits - lo;
        uint64_t w = kind == 0 ? next_u64() : kind == 1 ? ~uint64_t(0) : 0;
        if (here < 64) w &= (uint64_t(1) << here) - 1;
        if (bits - lo <= 64) w |= uint64_t(1) << (here - 1);  // the top bit
        v.w[j] = w;
    }
    return v;
}

static long failures = 0;
static void fail(const char* what, int L, int bm, int bq) {
    std::fprintf(stderr, "FAIL %s: L=%d bits(mag)=%d bits(q)=%d\n", what, L, bm, bq);
    ++failures;
}

template <typename F, int L>
static long run() {
    long calls = 0;
    const limbs<L> one = with_bits<L>(1, 2);
    for (int bq = 1; bq <= 64 * L; ++bq) {
        for (int kind = 0; kind < 3; ++kind) {
            const limbs<L> q = with_bits<L>(bq, kind);
            if (ur_round<F, L>(false, ml_zero<L>(), q) != F(0) ||
                std::signbit(ur_round<F, L>(true, ml_zero<L>(), q)))
                fail("zero numerator", L, 0, bq);
            F last = F(0);
            for (int bm = 1; bm <= 64 * L; ++bm) {
                const limbs<L> mag = with_bits<L>(bm, kind == 0 ? 0 : 2);  // grows with bm
                const F pos = ur_round<F, L>(false, mag, q);
                const F neg = ur_round<F, L>(true, mag, q);
                calls += 2;
                if (!std::isfinite(pos) || pos < F(0) || neg != -pos || !std::signbit(neg))
                    fail("finite and signed", L, bm, bq);
                if (pos < last) fail("monotonic in the numerator", L, bm, bq);
                last = pos;
            }
        }
    }
    // mag == q is exactly one; mag / 1 of at most p bits is exact
    for (int b = 1; b <= 64 * L; ++b) {
        const limbs<L> v = with_bits<L>(b, 0);
        if (ur_round<F, L>(false, v, v) != F(1)) fail("v / v", L, b, b);
        if (b <= std::numeric_limits<F>::digits) {
            if (ur_round<F, L>(false, v, one) != F(v.w[0])) fail("v / 1", L, b, 1);
        }
        calls += 2;
    }
    for (int i = 0; i < 20000; ++i) {
        const int bm = 1 + int(next_u64() % (64 * L)), bq = 1 + int(next_u64() % (64 * L));
        const F r = ur_round<F, L>(i & 1, with_bits<L>(bm, 0), with_bits<L>(bq, 0));
        ++calls;
        if (!std::isfinite(r) || std::signbit(r) != bool(i & 1)) fail("random pair", L, bm, bq);
    }
    return calls;
}

template <typename F>
static long run_all() {
    return run<F, 1>() + run<F, 2>() + run<F, 3>() + run<F, 4>() + run<F, 5>();
}

int main() {
    const long f = run_all<float>();
    const long d = run_all<double>();
    if (failures) {
        std::fprintf(stderr, "unmask_round_sanitize: %ld failures\n", failures);
        return 1;
    }
    std::printf("unmask_round_sanitize: OK (%ld float and %ld double calls, L = 1..5)\n", f, d);
    return 0;
}
