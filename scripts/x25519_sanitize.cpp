// Stand-alone sanitizer pass over the K9 arithmetic
// (xaynet_amd/csrc/gpu/fe25519.h), the source the k9 kernels compile.
// Build and run on the CPU, from the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ixaynet_amd/csrc scripts/x25519_sanitize.cpp -o build/x25519_sanitize
//   build/x25519_sanitize
//
// It runs fe_x25519 over the edge points of tests/test_x25519_cpu.py (0, 1,
// p - 1, p, p + 1, the two points of order 8, 2, 9, p - 2, 2^255 - 20,
// 2^255 - 1, 2^256 - 1, 9 with bit 255 set), each under the all-zero, the
// all-ones and a random scalar, and checks what needs no second
// implementation: the RFC 7748 5.2 vectors and the first iteration, that u and
// u + p agree, that bit 255 of u is ignored, that every point of small order
// gives zero, that the output is below p, and that a Diffie-Hellman pair
// agrees. It runs fe_seal_nonce on one fixed input against its known BLAKE2b
// digest. Byte equality with the integer reference on every pair is the
// test's part.
#include <cstdio>
#include <cstdlib>

#include "gpu/fe25519.h"

static int failures = 0;

static void from_hex(uint32_t w[8], const char* hex) {
    uint8_t b[32];
    for (int i = 0; i < 32; ++i) {
        unsigned v;
        std::sscanf(hex + 2 * i, "%2x", &v);
        b[i] = uint8_t(v);
    }
    std::memcpy(w, b, 32);
}

static void expect(const uint32_t got[8], const uint32_t want[8], const char* what) {
    if (std::memcmp(got, want, 32) != 0) {
        std::printf("FAIL %s\n", what);
        ++failures;
    }
}

// p + d as words (d may be negative)
static void p_plus(uint32_t w[8], int d) {
    for (int i = 0; i < 8; ++i) w[i] = 0xffffffffu;
    w[7] = 0x7fffffffu;
    w[0] = uint32_t(int64_t(0xffffffedu) + d);  // |d| < 19: no borrow below p + 19
    if (d >= 19) {                              // p + d = 2^255 + (d - 19)
        for (int i = 0; i < 8; ++i) w[i] = 0;
        w[0] = uint32_t(d - 19);
        w[7] = 0x80000000u;
    }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return uint32_t((z ^ (z >> 31)) >> 16);
}

int main() {
    uint32_t k[8], u[8], out[8], want[8];

    from_hex(k, "a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4");
    from_hex(u, "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c");
    from_hex(want, "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552");
    fe_x25519(out, k, u);
    expect(out, want, "RFC 7748 5.2 vector 1");
    from_hex(k, "4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d");
    from_hex(u, "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493");
    from_hex(want, "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957");
    fe_x25519(out, k, u);
    expect(out, want, "RFC 7748 5.2 vector 2");
    const uint32_t nine[8] = {9, 0, 0, 0, 0, 0, 0, 0};
    from_hex(want, "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079");
    fe_x25519(out, nine, nine);
    expect(out, want, "RFC 7748 5.2 iteration 1");

    // the edge points
    uint32_t pts[14][8] = {};
    pts[1][0] = 1;
    p_plus(pts[2], -1);
    p_plus(pts[3], 0);
    p_plus(pts[4], 1);
    from_hex(pts[5], "e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800");
    from_hex(pts[6], "5f9c95bca3508c24b1d0b1559c83ef5b04445cc4581c8e86d8224eddd09f1157");
    pts[7][0] = 2;
    pts[8][0] = 9;
    p_plus(pts[9], -2);
    p_plus(pts[10], -1);  // 2^255 - 20
    p_plus(pts[11], 18);  // 2^255 - 1
    for (int i = 0; i < 8; ++i) pts[12][i] = 0xffffffffu;  // 2^256 - 1
    pts[13][0] = 9;
    pts[13][7] = 0x80000000u;
    uint32_t scalars[3][8];
    for (int i = 0; i < 8; ++i) {
        scalars[0][i] = 0;
        scalars[1][i] = 0xffffffffu;
        scalars[2][i] = next_u32() << 16 | next_u32();
    }
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t res[14][8];
    for (int s = 0; s < 3; ++s) {
        for (int p = 0; p < 14; ++p) {
            fe_x25519(res[p], scalars[s], pts[p]);
            // canonical: below p = 2^255 - 19
            bool top = (res[p][7] >> 31) != 0;
            bool all = res[p][7] == 0x7fffffffu && res[p][0] >= 0xffffffedu;
            for (int i = 1; i < 7; ++i) all = all && res[p][i] == 0xffffffffu;
            if (top || all) {
                std::printf("FAIL output of point %d not below p\n", p);
                ++failures;
            }
        }
        expect(res[3], res[0], "u = p against u = 0");
        expect(res[4], res[1], "u = p + 1 against u = 1");
        expect(res[13], res[8], "bit 255 of u");
        for (int p = 0; p < 7; ++p) expect(res[p], zero, "a point of small order");
    }

    // Diffie-Hellman on random keys
    for (int round = 0; round < 4; ++round) {
        uint32_t a[8], b[8], pa[8], pb[8], sa[8], sb[8];
        for (int i = 0; i < 8; ++i) {
            a[i] = next_u32() << 16 | next_u32();
            b[i] = next_u32() << 16 | next_u32();
        }
        fe_x25519(pa, a, nine);
        fe_x25519(pb, b, nine);
        fe_x25519(sa, a, pb);
        fe_x25519(sb, b, pa);
        expect(sa, sb, "Diffie-Hellman");
    }

    // BLAKE2b-24 of bytes 0..63, digest from any BLAKE2b implementation
    uint32_t epk[8], pk[8], nonce[6];
    uint8_t in[64], digest[32] = {};
    for (int i = 0; i < 64; ++i) in[i] = uint8_t(i);
    std::memcpy(epk, in, 32);
    std::memcpy(pk, in + 32, 32);
    fe_seal_nonce(nonce, epk, pk);
    uint32_t dw[8];
    from_hex(dw, "aa054507b4916837a6d2b35b1ce7c525facdb7868ed55a8a0000000000000000");
    std::memcpy(digest, dw, 32);
    if (std::memcmp(nonce, digest, 24) != 0) {
        std::printf("FAIL seal nonce\n");
        ++failures;
    }

    if (failures) return 1;
    std::printf("x25519_sanitize: OK\n");
    return 0;
}
