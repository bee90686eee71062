// Stand-alone sanitizer pass over the model decoder's element functions
// (mc_span / mc_read in xaynet_amd/csrc/gpu/model_codec.h), the source the K7d
// kernels compile. Host only. Build and run on the CPU, from the repository
// root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ixaynet_amd/csrc scripts/model_decode_sanitize.cpp -o build/model_decode_sanitize
//   build/model_decode_sanitize
//
// Every word array is copied to the very end of a heap allocation of exactly
// its size before it is walked, so a read at or past `avail` is an
// AddressSanitizer error. Walked are: valid bodies per dtype (which must
// decode to their inputs bit for bit), every truncation of them, and seeded
// single-word corruptions (whatever is still accepted must re-encode to the
// same words). Equality with the CPU decoder is tests/test_model_decode_cpu.py's
// part.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "gpu/model_codec.h"

// The host walk of model_codec_decode over `total` words that end exactly at
// the end of their allocation. Returns false for "rejected".
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
        // also with everything that is left as `avail`, as the kernels' LDS tile gives it
        const uint32_t wide = mc_span(w + at, uint32_t(left > 4096 ? 4096 : left));
        if (len != wide) {
            std::puts("mc_span depends on avail beyond the element");
            std::exit(1);
        }
        ok = len != 0 && mc_read<T>(w + at, len, &out[i]);
        at += len;
    }
    std::free(w);
    return ok && at == total;
}

template <typename T>
static std::vector<uint32_t> encode(const std::vector<T>& in) {
    std::vector<uint32_t> words;
    for (T x : in) {
        const mc_value v = mc_decompose(x);
        const size_t at = words.size();
        words.resize(at + mc_words(v));
        mc_write(v, words.data() + at);
    }
    return words;
}

template <typename T>
static bool same_bits(T a, T b) {
    return memcmp(&a, &b, sizeof a) == 0;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 2685821657736338717ull;
}

template <typename T>
static std::vector<T> float_inputs() {
    using L = std::numeric_limits<T>;
    const int p = L::digits, emin = L::min_exponent - L::digits, emax = L::max_exponent - 1;
    const T full = T(std::ldexp(1.0, p) - 1.0);
    std::vector<T> v = {T(0), T(1), T(-1), T(0.5), L::max(), L::lowest(), L::min(),
                        L::denorm_min(), -L::denorm_min()};
    for (int k = emin; k <= emax; k += 3) v.push_back(T(std::ldexp(1.0, k)));
    for (int k = emin; k <= emax - p + 1; k += 5) v.push_back(-T(std::ldexp(double(full), k)));
    for (int k = -80; k <= 80; ++k) v.push_back(T(std::ldexp(3.0, k)));
    return v;
}

template <typename T>
static std::vector<T> int_inputs() {
    using L = std::numeric_limits<T>;
    std::vector<T> v = {0, 1, -1, L::max(), L::min(), T(L::max() - 1), T(L::min() + 1)};
    for (int k = 0; k < L::digits; ++k) {
        v.push_back(T(T(1) << k));
        v.push_back(T(-(T(1) << k)));
        v.push_back(T((T(1) << k) | 1));
    }
    return v;
}

template <typename T>
static int run(const char* name, const std::vector<T>& in) {
    const std::vector<uint32_t> words = encode(in);
    std::vector<T> out;
    if (!walk(words, words.size(), in.size(), out)) {
        std::printf("%s: the valid body is rejected\n", name);
        return 1;
    }
    for (size_t i = 0; i < in.size(); ++i)
        if (!same_bits(out[i], in[i])) {
            std::printf("%s: element %zu does not decode to its input\n", name, i);
            return 1;
        }
    // every truncation: the walk ends at the cut, never behind it
    for (size_t cut = 0; cut < words.size(); ++cut)
        if (walk(words, cut, in.size(), out)) {
            std::printf("%s: accepted %zu of %zu words\n", name, cut, words.size());
            return 1;
        }
    // one word overwritten: accepted only where it is the encoding of the result
    static const uint32_t picks[7] = {0, 1, 2, 3, 35, 36, 0xffffffffu};
    size_t accepted = 0;
    for (int c = 0; c < 20000; ++c) {
        std::vector<uint32_t> bad = words;
        const uint64_t r = rng();
        bad[size_t(rng() % bad.size())] = (r & 7) == 7 ? uint32_t(r >> 32) : picks[r & 7];
        if (!walk(bad, bad.size(), in.size(), out)) continue;
        ++accepted;
        if (encode(out) != bad) {
            std::printf("%s: accepted a body that is not the encoding of its values\n", name);
            return 1;
        }
    }
    std::printf("%s: %zu elements, %zu words, %zu of 20000 corruptions still canonical\n", name,
                in.size(), words.size(), accepted);
    return 0;
}

int main() {
    int bad = 0;
    bad |= run("f32", float_inputs<float>());
    bad |= run("f64", float_inputs<double>());
    bad |= run("i32", int_inputs<int32_t>());
    bad |= run("i64", int_inputs<int64_t>());
    std::puts(bad ? "model_decode_sanitize: FAILED" : "model_decode_sanitize: OK");
    return bad;
}
