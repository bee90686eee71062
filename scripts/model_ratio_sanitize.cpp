// Stand-alone sanitizer pass over the rational model decoder's element
// function (mc_read_ratio / mc_read_rational in
// xaynet_amd/csrc/gpu/model_codec.h), the source k7d_emit<T, true> compiles.
// Host only. Build and run on the CPU, from the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ixaynet_amd/csrc scripts/model_ratio_sanitize.cpp -o build/model_ratio_sanitize
//   build/model_ratio_sanitize
//
// As in model_decode_sanitize.cpp, every word array is copied to the very end
// of a heap allocation of exactly its size before it is walked, so a read at
// or past `avail` is an AddressSanitizer error, and every shift and
// conversion of the division runs under UBSan. Walked per dtype: a body of
// random rationals of 0..10 digits a side (floats must accept all of it, and
// small quotients must equal the plain integer division), every truncation
// of it, and seeded single-word corruptions. Equality with Fraction is
// tests/test_model_ratio_cpu.py's part.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "gpu/model_codec.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 2685821657736338717ull;
}

// The host walk of model_codec_decode(rational=True) over `total` words that
// end exactly at the end of their allocation. Returns false for "rejected".
template <typename T>
static bool walk(const std::vector<uint32_t>& src, size_t total, size_t n, std::vector<T>& out) {
    uint32_t* w = static_cast<uint32_t*>(std::malloc(total ? 4 * total : 1));
    if (total) memcpy(w, src.data(), 4 * total);
    out.assign(n, T(0));
    size_t at = 0;
    bool ok = n <= total / 7 && total <= size_t(MC_MAX_WORDS) * n;
    for (size_t i = 0; ok && i < n; ++i) {
        const size_t left = total - at;
        const uint32_t len = mc_span(w + at, left > MC_MAX_WORDS ? MC_MAX_WORDS : uint32_t(left));
        ok = len != 0 && mc_read_rational<T>(w + at, len, &out[i]);
        at += len;
    }
    std::free(w);
    return ok && at == total;
}

// sign | count | digits with a non-zero top digit
static void put_number(std::vector<uint32_t>& words, uint32_t sign, uint32_t digits) {
    words.insert(words.end(), {sign, digits, 0u});
    for (uint32_t i = 0; i < digits; ++i)
        words.push_back(uint32_t(rng()) | (i + 1 == digits ? 1u : 0u));
}

// n elements; `small` keeps the numerator to two digits under a denominator
// of at least two, so that the quotient is an i64
static std::vector<uint32_t> body(size_t n, bool small) {
    std::vector<uint32_t> words;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t nd = uint32_t(rng() % (small ? 3 : MC_RATIO_DIGITS + 1));
        const uint32_t dd = 1 + uint32_t(rng() % MC_RATIO_DIGITS);
        put_number(words, nd == 0 ? 1u : (rng() & 1 ? 0u : 2u), nd);
        put_number(words, 2u, small && dd < 2 ? 2u : dd);
    }
    return words;
}

template <typename T>
static int run(const char* name) {
    constexpr bool is_float = std::is_floating_point<T>::value;
    const size_t n = 400;
    const std::vector<uint32_t> words = body(n, true);
    std::vector<T> out;
    const bool accepted_all = walk(words, words.size(), n, out);
    if (is_float && !accepted_all) {
        std::printf("%s: a valid body is rejected\n", name);
        return 1;
    }
    const std::vector<uint32_t> wide = body(n, false);
    if (is_float && !walk(wide, wide.size(), n, out)) {
        std::printf("%s: a valid ten-digit body is rejected\n", name);
        return 1;
    }
    if (!is_float) walk(wide, wide.size(), n, out);  // mostly out of range: must only be clean
    for (size_t cut = 0; cut < words.size(); ++cut)
        if (walk(words, cut, n, out)) {
            std::printf("%s: accepted %zu of %zu words\n", name, cut, words.size());
            return 1;
        }
    static const uint32_t picks[7] = {0, 1, 2, 3, 10, 11, 0xffffffffu};
    size_t accepted = 0;
    for (int c = 0; c < 20000; ++c) {
        std::vector<uint32_t> bad = c & 1 ? words : wide;
        const uint64_t r = rng();
        bad[size_t(rng() % bad.size())] = (r & 7) == 7 ? uint32_t(r >> 32) : picks[r & 7];
        accepted += walk(bad, bad.size(), n, out);
    }
    std::printf("%s: %zu + %zu words, %zu of 20000 corruptions still accepted\n", name,
                words.size(), wide.size(), accepted);
    return 0;
}

// one-limb quotients against the machine's own division, and the type's ends
static int ends() {
    int bad = 0;
    for (int c = 0; c < 20000; ++c) {
        const uint64_t a = rng() >> (rng() % 64), b = (rng() >> (rng() % 64)) | 1;
        limbs<MC_RATIO_LIMBS> mag = ml_zero<MC_RATIO_LIMBS>(), q = mag;
        mag.w[0] = a;
        q.w[0] = b;
        uint64_t x = 0;
        bad |= !mc_trunc_div(mag, q, &x) || x != a / b;
        mag.w[1] = b;  // (b * 2^64 + a) / b is 2^64 or more
        bad |= mc_trunc_div(mag, q, &x);
    }
    const uint32_t min32[] = {0, 1, 0, 0x80000000u, 2, 1, 0, 1};
    const uint32_t max32[] = {2, 1, 0, 0x80000000u, 2, 1, 0, 1};
    int32_t v = 0;
    bad |= !mc_read_ratio<int32_t>(min32, 8, &v) || v != INT32_MIN;
    bad |= mc_read_ratio<int32_t>(max32, 8, &v);
    if (bad) std::puts("ends: a quotient is wrong");
    return bad;
}

int main() {
    int bad = ends();
    bad |= run<float>("f32");
    bad |= run<double>("f64");
    bad |= run<int32_t>("i32");
    bad |= run<int64_t>("i64");
    std::puts(bad ? "model_ratio_sanitize: FAILED" : "model_ratio_sanitize: OK");
    return bad;
}
