// Stand-alone sanitizer pass over the K10 arithmetic
// (xaynet_amd/csrc/gpu/ed25519.h), the source the k10 kernels compile.
// Build and run on the CPU, from the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ixaynet_amd/csrc scripts/ed25519_sanitize.cpp -o build/ed25519_sanitize
//   build/ed25519_sanitize
//
// It runs ed25519_verify_host over the RFC 8032 7.1 vectors 1 to 3, each also
// with one bit flipped in R, in s, in the key and (where there is one) in the
// message; over s = L, L - 1, 0 and 2^256 - 1; over the keys 1 (the identity),
// p + 1, 1 with the sign bit and p - 1 with the signature (identity, 0), which
// is valid under the identity whatever the message; and over that signature's
// R re-encoded as p + 1. It checks sc_reduce512 at 0, L - 1, L and 2^512 - 1.
// Equality with the integer reference on the whole case list is the test's
// part (tests/test_ed25519_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpu/ed25519.h"

static int failures = 0;

static std::vector<uint8_t> from_hex(const char* hex) {
    std::vector<uint8_t> out;
    for (size_t i = 0; hex[i] && hex[i + 1]; i += 2) {
        unsigned v;
        std::sscanf(hex + i, "%2x", &v);
        out.push_back(uint8_t(v));
    }
    return out;
}

static void expect(bool got, bool want, const char* what, int n) {
    if (got != want) {
        std::printf("FAIL %s (%d)\n", what, n);
        ++failures;
    }
}

static bool verify(const std::vector<uint8_t>& sig, const std::vector<uint8_t>& msg,
                   const std::vector<uint8_t>& pk) {
    // exact-size heap copies: a read past any of the three is a finding
    std::vector<uint8_t> g(sig), m(msg), k(pk);
    return ed25519_verify_host(g.data(), m.data(), m.size(), k.data());
}

static std::vector<uint8_t> le32(const uint32_t w[8]) {
    std::vector<uint8_t> out(32);
    std::memcpy(out.data(), w, 32);
    return out;
}

int main() {
    const char* rfc[3][3] = {
        {"d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a", "",
         "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e06522490155"
         "5fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b"},
        {"3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c", "72",
         "92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da"
         "085ac1e43e15996e458f3613d0f11d8c387b2eaeb4302aeeb00d291612bb0c00"},
        {"fc51cd8e6218a1a38da47ed00230f0580816ed13ba3303ac5deb911548908025", "af82",
         "6291d657deec24024827e69c3abe01a30ce548a284743a445e3680d7db5ac3ac"
         "18ff9b538d16f290ae67f760984dc6594a7c15e9716ed28dc027beceea1ec40a"}};
    for (int v = 0; v < 3; ++v) {
        const auto pk = from_hex(rfc[v][0]), msg = from_hex(rfc[v][1]), sig = from_hex(rfc[v][2]);
        expect(verify(sig, msg, pk), true, "RFC 8032 7.1 vector", v + 1);
        auto bad = sig;
        bad[3] ^= 0x10;
        expect(verify(bad, msg, pk), false, "a bit of R", v + 1);
        bad = sig;
        bad[45] ^= 0x02;
        expect(verify(bad, msg, pk), false, "a bit of s", v + 1);
        auto key = pk;
        key[17] ^= 0x40;
        expect(verify(sig, msg, key), false, "a bit of the key", v + 1);
        auto other = msg;
        other.push_back(0);
        expect(verify(sig, other, pk), false, "a longer message", v + 1);
        if (!msg.empty()) {
            other = msg;
            other[0] ^= 1;
            expect(verify(sig, other, pk), false, "a bit of the message", v + 1);
        }
        // a long message: 40 blocks, the schedule and the padding under the sanitizer
        other.assign(5000, uint8_t(v));
        expect(verify(sig, other, pk), false, "a 5000-byte message", v + 1);
    }

    uint32_t L[8], w[8];
    for (int i = 0; i < 8; ++i) L[i] = sc_l(i);
    const auto pk = from_hex(rfc[0][0]);
    auto sig = from_hex(rfc[0][2]);
    const uint32_t edge[4][8] = {
        {L[0], L[1], L[2], L[3], L[4], L[5], L[6], L[7]},
        {L[0] - 1, L[1], L[2], L[3], L[4], L[5], L[6], L[7]},
        {0, 0, 0, 0, 0, 0, 0, 0},
        {~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u}};
    for (int e = 0; e < 4; ++e) {
        std::memcpy(sig.data() + 32, edge[e], 32);
        expect(verify(sig, {}, pk), false, "an edge value of s", e);
        expect(sc_is_canonical(edge[e]) != 0, e == 1 || e == 2, "sc_is_canonical", e);
    }

    // (identity, 0) under the keys of the edge list
    const uint32_t p1[8] = {0xffffffeeu, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, 0x7fffffffu};  // p + 1
    const uint32_t pm1[8] = {0xffffffecu, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, 0x7fffffffu};  // p - 1
    const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0}, one_sign[8] = {1, 0, 0, 0, 0, 0, 0, 1u << 31};
    std::vector<uint8_t> ident_sig(64, 0);
    ident_sig[0] = 1;
    const std::vector<uint8_t> any = {'a', 'n', 'y'};
    expect(verify(ident_sig, any, le32(one)), true, "the identity as key", 0);
    expect(verify(ident_sig, any, le32(p1)), true, "p + 1 as key", 0);
    expect(verify(ident_sig, any, le32(one_sign)), false, "x = 0 with the sign bit", 0);
    // order 2: k A is the identity or A, so (identity, 0) holds for even k only; run it, no verdict
    verify(ident_sig, any, le32(pm1));
    std::memcpy(ident_sig.data(), p1, 32);
    expect(verify(ident_sig, any, le32(one)), false, "R as y + p", 0);

    uint32_t x[16] = {};
    sc_reduce512(w, x);
    expect(std::memcmp(w, edge[2], 32) == 0, true, "0 mod L", 0);
    std::memcpy(x, edge[1], 32);
    sc_reduce512(w, x);
    expect(std::memcmp(w, edge[1], 32) == 0, true, "L - 1 mod L", 0);
    std::memcpy(x, edge[0], 32);
    sc_reduce512(w, x);
    expect(std::memcmp(w, edge[2], 32) == 0, true, "L mod L", 0);
    for (int i = 0; i < 16; ++i) x[i] = ~0u;
    sc_reduce512(w, x);
    expect(sc_is_canonical(w) != 0, true, "2^512 - 1 mod L is below L", 0);

    if (failures) return 1;
    std::printf("ed25519_sanitize: OK\n");
    return 0;
}
