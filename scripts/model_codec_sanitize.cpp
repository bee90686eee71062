// Stand-alone sanitizer pass over the model encoder's element functions
// (xaynet_amd/csrc/gpu/model_codec.h), the source the K7 kernels compile.
// Build and run on the CPU, from the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ixaynet_amd/csrc scripts/model_codec_sanitize.cpp -o build/model_codec_sanitize
//   build/model_codec_sanitize
//
// For each dtype it encodes an edge vector (zeros, NaN, infinities, the
// subnormals, the longest elements, every power of two, full mantissas across
// each 32-bit digit boundary) into a heap buffer of exactly the counted size,
// so a word written past an element's count is an AddressSanitizer error, and
// walks the result back by its length fields. Byte equality with the CPU
// encoder is tests/test_model_codec_cpu.py's part.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "gpu/model_codec.h"

template <typename T>
static T from_bits(uint64_t bits) {
    T v;
    if (sizeof(T) == 4) {
        const uint32_t b = uint32_t(bits);
        memcpy(&v, &b, 4);
    } else {
        memcpy(&v, &bits, 8);
    }
    return v;
}

template <typename T>
static std::vector<T> float_edges() {
    using L = std::numeric_limits<T>;
    const int p = L::digits, emin = L::min_exponent - L::digits, emax = L::max_exponent - 1;
    const uint64_t frac_ones = (uint64_t(1) << (p - 1)) - 1;
    const T full = T(std::ldexp(1.0, p) - 1.0);
    std::vector<T> v = {T(0),       -T(0),         T(1),        T(-1),
                        L::quiet_NaN(), L::infinity(), -L::infinity(), L::max(),
                        L::lowest(), L::min(),      L::denorm_min(), -L::denorm_min()};
    v.push_back(from_bits<T>(frac_ones));                              // greatest subnormal
    v.push_back(from_bits<T>((uint64_t(1) << (p - 1)) | frac_ones));   // least normal, full mantissa
    v.push_back(-from_bits<T>((uint64_t(1) << (p - 1)) | frac_ones));
    for (int k = emin; k <= emax; ++k) v.push_back(T(std::ldexp(1.0, k)));
    for (int k = 0; k <= 70; ++k) v.push_back(T(std::ldexp(double(full), k)));
    for (int k = 1; k <= -emin; ++k) {
        if (k % 32 > 1 && k % 32 != 31) continue;
        v.push_back(T(std::ldexp(3.0, -k)));
        v.push_back(-T(std::ldexp(double(full), -k)));
    }
    v.push_back(T(std::ldexp(double(full), emax - p + 1)));  // the type's max again
    return v;
}

template <typename T>
static std::vector<T> int_edges() {
    using L = std::numeric_limits<T>;
    std::vector<T> v = {0, 1, -1, L::max(), L::min(), T(L::max() - 1), T(L::min() + 1)};
    for (int k = 0; k < L::digits; ++k) {
        v.push_back(T(T(1) << k));
        v.push_back(T(-(T(1) << k)));
        const int64_t m = int64_t(0x7fffffff);
        if (k + 31 <= L::digits) {
            v.push_back(T(m << k));
            v.push_back(T(-(m << k)));
        }
    }
    return v;
}

template <typename T>
static int run(const char* name, const std::vector<T>& in) {
    size_t total = 0;
    uint32_t longest = 0;
    for (T x : in) {
        const uint32_t n = mc_words(mc_decompose(x));
        if (n < 7 || n > MC_MAX_WORDS) {
            std::printf("%s: element of %u words\n", name, n);
            return 1;
        }
        longest = n > longest ? n : longest;
        total += n;
    }
    // exactly sized, on the heap: one word too many is out of bounds
    uint32_t* out = static_cast<uint32_t*>(std::malloc(4 * total));
    for (size_t i = 0; i < total; ++i) out[i] = 0xdeadbeefu;
    size_t at = 0;
    for (T x : in) {
        const mc_value v = mc_decompose(x);
        mc_write(v, out + at);
        at += mc_words(v);
    }
    // walk it back: sign | count u64 | digits, twice per element
    size_t rd = 0;
    for (size_t i = 0; i < in.size(); ++i) {
        const size_t start = rd;
        for (int part = 0; part < 2; ++part) {
            const uint32_t sign = out[rd], lo = out[rd + 1], hi = out[rd + 2];
            if (sign > 2 || hi != 0 || (part == 1 && (sign != 2 || lo == 0))) {
                std::printf("%s: bad field in element %zu\n", name, i);
                return 1;
            }
            rd += 3 + lo;
            if (lo && out[rd - 1] == 0) {
                std::printf("%s: leading zero digit in element %zu\n", name, i);
                return 1;
            }
        }
        if (rd - start != mc_words(mc_decompose(in[i]))) {
            std::printf("%s: element %zu is not its counted length\n", name, i);
            return 1;
        }
    }
    uint64_t h = 1469598103934665603ull;  // FNV-1a of the words
    for (size_t i = 0; i < total; ++i) {
        if (out[i] == 0xdeadbeefu) {
            std::printf("%s: word %zu not written\n", name, i);
            return 1;
        }
        h = (h ^ out[i]) * 1099511628211ull;
    }
    std::free(out);
    std::printf("%s: %zu elements, %zu words, longest %u, fnv %016llx\n", name, in.size(), total,
                longest, (unsigned long long)h);
    return rd == total ? 0 : 1;
}

int main() {
    int bad = 0;
    bad |= run("f32", float_edges<float>());
    bad |= run("f64", float_edges<double>());
    bad |= run("i32", int_edges<int32_t>());
    bad |= run("i64", int_edges<int64_t>());
    std::puts(bad ? "model_codec_sanitize: FAILED" : "model_codec_sanitize: OK");
    return bad;
}
