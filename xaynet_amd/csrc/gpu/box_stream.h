// XSalsa20-Poly1305 (NaCl secretbox) cut into independent tiles: the
// arithmetic the K8 kernels (kernels.hip) and the host (box_stream_host in
// core_bindings.cpp) share, so it compiles as plain C++ like limbs.h. No
// secret-dependent branch or index anywhere: every branch below is on a
// length, a tile number or a lane number, all public.
//
// Stream coordinates. Keystream byte x of a box belongs to message byte
// x - 32: the first 32 keystream bytes are the one-time Poly1305 key. The
// stream is cut into 16-byte slots (slot q holds Poly1305 block q - 2; 32 is a
// multiple of 16, so a 64-byte Salsa block is four whole slots) and into tiles
// of B Salsa blocks = S = 4B slots (B = 256 on the GPU: 16 KiB). Tile 0
// carries the two key slots and S - 2 blocks, every later full tile S.
//
// A tile works on S *positions*. Position `pos` holds slot pos - shift of the
// tile, shift = S - used, so the last valid slot of a short tile sits on the
// last position and the empty positions lead: a zero in front of a Poly1305
// message changes nothing, a zero behind it would. Position pos belongs to
// lane pos % B in pass pos / B. A lane runs Horner by r^B over its four
// passes; lanes fold pairwise, level m by r^(2^m); the root times r is the
// tile partial
//   P_t = sum_j c_j * r^(nb_t - j + 1),  j = 1..nb_t,
// the tile's nb_t blocks right-aligned to exponent 1. A box's tag is then
//   H = (sum_{t < T-1} P_t * (r^S)^(T-2-t)) * r^(nb_last) + P_(T-1)
// finished as Poly1305 finishes: the first sum by BS_FINISH_LANES lanes
// striding over the tiles (right-aligned the same way) and one more tree.
//
// Field elements are five 26-bit limbs in u32. bs_mulmod takes any h (limbs
// below 2^32) and r limbs below 2^26 + 2^15 (what it leaves itself): five
// products of 2^32 * 5 * 2^26.01 stay below 2^63. A tree of depth d adds d + 2
// reduced elements between two multiplications, far from 2^32.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define BS_FN __host__ __device__ __forceinline__
#else
#define BS_FN inline
#endif

#define BS_POWERS 11        // r^(2^m), m = 0..10: tiles of up to 2^10 slots
#define BS_FINISH_LANES 64  // lanes striding over a box's tile partials

enum { BS_OPEN = 0, BS_SEAL = 1, BS_MAC = 2 };

// ------------------------------------------------------------- Salsa20/20

BS_FN uint32_t bs_rotl(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }

#define BS_QR(a, b, c, d)          \
    x[b] ^= bs_rotl(x[a] + x[d], 7);  \
    x[c] ^= bs_rotl(x[b] + x[a], 9);  \
    x[d] ^= bs_rotl(x[c] + x[b], 13); \
    x[a] ^= bs_rotl(x[d] + x[c], 18)

// The 20 rounds on x in place, without the feed-forward.
BS_FN void bs_salsa_rounds(uint32_t x[16]) {
#pragma unroll 1
    for (int round = 0; round < 10; ++round) {
        BS_QR(0, 4, 8, 12);
        BS_QR(5, 9, 13, 1);
        BS_QR(10, 14, 2, 6);
        BS_QR(15, 3, 7, 11);
        BS_QR(0, 1, 2, 3);
        BS_QR(5, 6, 7, 4);
        BS_QR(10, 11, 8, 9);
        BS_QR(15, 12, 13, 14);
    }
}

// sigma, the key words k[8] and the four words in[4] of the nonce/counter row
BS_FN void bs_salsa_state(uint32_t st[16], const uint32_t k[8], const uint32_t in[4]) {
    st[0] = 0x61707865;
    st[5] = 0x3320646e;
    st[10] = 0x79622d32;
    st[15] = 0x6b206574;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        st[1 + i] = k[i];
        st[11 + i] = k[4 + i];
        st[6 + i] = in[i];
    }
}

// Salsa20 block `counter` of the stream of (key, nonce8): 16 keystream words
BS_FN void bs_salsa_block(uint32_t out[16], const uint32_t key[8], const uint32_t nonce8[2],
                          uint64_t counter) {
    const uint32_t in[4] = {nonce8[0], nonce8[1], uint32_t(counter), uint32_t(counter >> 32)};
    uint32_t st[16];
    bs_salsa_state(st, key, in);
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = st[i];
    bs_salsa_rounds(out);
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] += st[i];
}

// subkey = HSalsa20(key, nonce16): the XSalsa20 key of nonce words 4..5
BS_FN void bs_hsalsa(uint32_t subkey[8], const uint32_t key[8], const uint32_t nonce16[4]) {
    uint32_t x[16];
    bs_salsa_state(x, key, nonce16);
    bs_salsa_rounds(x);
    subkey[0] = x[0];
    subkey[1] = x[5];
    subkey[2] = x[10];
    subkey[3] = x[15];
    subkey[4] = x[6];
    subkey[5] = x[7];
    subkey[6] = x[8];
    subkey[7] = x[9];
}

// --------------------------------------------------- Poly1305, 5 x 26 bits

struct bs_fe {
    uint32_t v[5];
};

BS_FN bs_fe bs_fe_zero() { return bs_fe{{0, 0, 0, 0, 0}}; }
BS_FN bs_fe bs_fe_one() { return bs_fe{{1, 0, 0, 0, 0}}; }

// 128 bits as limbs, `top` on bit 128
BS_FN bs_fe bs_fe_from_words(const uint32_t w[4], uint32_t top) {
    const uint32_t m = 0x3ffffff;
    bs_fe h;
    h.v[0] = w[0] & m;
    h.v[1] = ((w[0] >> 26) | (w[1] << 6)) & m;
    h.v[2] = ((w[1] >> 20) | (w[2] << 12)) & m;
    h.v[3] = ((w[2] >> 14) | (w[3] << 18)) & m;
    h.v[4] = (w[3] >> 8) | (top << 24);
    return h;
}

// r of the one-time key: its first 16 bytes, clamped
BS_FN bs_fe bs_clamp_r(const uint32_t w[4]) {
    const uint32_t c[4] = {w[0] & 0x0fffffff, w[1] & 0x0ffffffc, w[2] & 0x0ffffffc,
                           w[3] & 0x0ffffffc};
    return bs_fe_from_words(c, 0);
}

// how many of the first `bytes` (0..16) bytes of a block lie in its word i
BS_FN uint32_t bs_word_bytes(uint32_t bytes, int i) {
    const uint32_t lo = 4u * uint32_t(i);
    return bytes <= lo ? 0u : (bytes - lo >= 4u ? 4u : bytes - lo);
}

// zero all but the first `bytes` (0..16) bytes of w
BS_FN void bs_keep_bytes(uint32_t w[4], uint32_t bytes) {
    for (int i = 0; i < 4; ++i) {
        const uint32_t have = bs_word_bytes(bytes, i);
        w[i] &= have == 4 ? 0xffffffffu : (1u << (8 * have)) - 1u;
    }
}

// The Poly1305 block of the first `bytes` (1..16) bytes of w, the rest of w
// being zero (bs_keep_bytes): a full block gets the 2^128 pad bit, a short
// one 0x01 behind its last byte. bytes == 0: no block, zero.
BS_FN bs_fe bs_block(const uint32_t w[4], uint32_t bytes) {
    uint32_t p[4];
    for (int i = 0; i < 4; ++i) {
        const uint32_t have = bs_word_bytes(bytes, i);
        const bool pad_here = bytes != 0 && have < 4 && bytes >= 4u * uint32_t(i);
        p[i] = w[i] | (pad_here ? 1u << (8 * have) : 0u);
    }
    return bs_fe_from_words(p, bytes == 16 ? 1u : 0u);
}

BS_FN bs_fe bs_add(bs_fe a, const bs_fe& b) {
    for (int i = 0; i < 5; ++i) a.v[i] += b.v[i];
    return a;
}

// h * r mod 2^130 - 5, partially reduced: limbs below 2^26, limb 1 below
// 2^26 + 2^15. u32 x u32 -> u64 partial products, the wrap folded as 5 * r.
BS_FN bs_fe bs_mulmod(const bs_fe& h, const bs_fe& r) {
    const uint64_t h0 = h.v[0], h1 = h.v[1], h2 = h.v[2], h3 = h.v[3], h4 = h.v[4];
    const uint32_t r0 = r.v[0], r1 = r.v[1], r2 = r.v[2], r3 = r.v[3], r4 = r.v[4];
    const uint32_t s1 = r1 * 5, s2 = r2 * 5, s3 = r3 * 5, s4 = r4 * 5;
    uint64_t d0 = h0 * r0 + h1 * s4 + h2 * s3 + h3 * s2 + h4 * s1;
    uint64_t d1 = h0 * r1 + h1 * r0 + h2 * s4 + h3 * s3 + h4 * s2;
    uint64_t d2 = h0 * r2 + h1 * r1 + h2 * r0 + h3 * s4 + h4 * s3;
    uint64_t d3 = h0 * r3 + h1 * r2 + h2 * r1 + h3 * r0 + h4 * s4;
    uint64_t d4 = h0 * r4 + h1 * r3 + h2 * r2 + h3 * r1 + h4 * r0;
    const uint32_t m = 0x3ffffff;
    bs_fe o;
    d1 += d0 >> 26;
    d2 += d1 >> 26;
    d3 += d2 >> 26;
    d4 += d3 >> 26;
    o.v[2] = uint32_t(d2) & m;
    o.v[3] = uint32_t(d3) & m;
    o.v[4] = uint32_t(d4) & m;
    const uint64_t f = (uint64_t(uint32_t(d0) & m)) + (d4 >> 26) * 5;  // below 2^41
    o.v[0] = uint32_t(f) & m;
    o.v[1] = (uint32_t(d1) & m) + uint32_t(f >> 26);
    return o;
}

// acc * pow + add: one Horner step of a lane, one level of a tree
BS_FN bs_fe bs_step(const bs_fe& acc, const bs_fe& pow, const bs_fe& add) {
    return bs_add(bs_mulmod(acc, pow), add);
}

// r^e for e < 2^BS_POWERS from the stored r^(2^m)
BS_FN bs_fe bs_power(const bs_fe pw[BS_POWERS], uint32_t e) {
    bs_fe x = bs_fe_one();
    for (int m = 0; m < BS_POWERS; ++m)
        if ((e >> m) & 1) x = bs_mulmod(x, pw[m]);
    return x;
}

// The tag: h reduced fully (h >= 2^130 - 5 included), plus s mod 2^128.
BS_FN void bs_finish(uint32_t tag[4], const bs_fe& h, const uint32_t s[4]) {
    const uint32_t m = 0x3ffffff;
    uint32_t h0 = h.v[0], h1 = h.v[1], h2 = h.v[2], h3 = h.v[3], h4 = h.v[4];
    uint32_t c;
    // two carry rounds: limbs come in below 2^32, go out below 2^26
    for (int k = 0; k < 2; ++k) {
        c = h0 >> 26; h0 &= m; h1 += c;
        c = h1 >> 26; h1 &= m; h2 += c;
        c = h2 >> 26; h2 &= m; h3 += c;
        c = h3 >> 26; h3 &= m; h4 += c;
        c = h4 >> 26; h4 &= m; h0 += c * 5;
    }
    c = h0 >> 26; h0 &= m; h1 += c;
    // g = h + 5 - 2^130; its sign picks h or g
    uint32_t g0 = h0 + 5;
    c = g0 >> 26; g0 &= m;
    uint32_t g1 = h1 + c;
    c = g1 >> 26; g1 &= m;
    uint32_t g2 = h2 + c;
    c = g2 >> 26; g2 &= m;
    uint32_t g3 = h3 + c;
    c = g3 >> 26; g3 &= m;
    const uint32_t g4 = h4 + c - (1u << 26);
    const uint32_t take_g = (g4 >> 31) - 1;  // all ones iff g >= 0, i.e. h >= p
    h0 = (h0 & ~take_g) | (g0 & take_g);
    h1 = (h1 & ~take_g) | (g1 & take_g);
    h2 = (h2 & ~take_g) | (g2 & take_g);
    h3 = (h3 & ~take_g) | (g3 & take_g);
    h4 = (h4 & ~take_g) | (g4 & take_g);
    // h mod 2^128 as four words, plus s
    const uint32_t w0 = h0 | (h1 << 26);
    const uint32_t w1 = (h1 >> 6) | (h2 << 20);
    const uint32_t w2 = (h2 >> 12) | (h3 << 14);
    const uint32_t w3 = (h3 >> 18) | (h4 << 8);
    uint64_t f = uint64_t(w0) + s[0];
    tag[0] = uint32_t(f);
    f = uint64_t(w1) + s[1] + (f >> 32);
    tag[1] = uint32_t(f);
    f = uint64_t(w2) + s[2] + (f >> 32);
    tag[2] = uint32_t(f);
    f = uint64_t(w3) + s[3] + (f >> 32);
    tag[3] = uint32_t(f);
}

// 16 bytes equal? No exit on the first difference.
BS_FN bool bs_equal16(const uint32_t a[4], const uint32_t b[4]) {
    return ((a[0] ^ b[0]) | (a[1] ^ b[1]) | (a[2] ^ b[2]) | (a[3] ^ b[3])) == 0;
}

// ------------------------------------------------- per-box key material

// What k8_box_keys leaves for the other kernels: one row per box.
struct bs_box_keys {
    uint32_t subkey[8];      // XSalsa20 subkey (unused by the MAC alone)
    uint32_t s[4];           // the tag's additive half
    bs_fe pw[BS_POWERS];     // r^(2^m)
    uint32_t pad[1];         // rows stay 16-byte multiples: 272 bytes
};

BS_FN void bs_powers(bs_fe pw[BS_POWERS], const bs_fe& r) {
    pw[0] = r;
    for (int m = 1; m < BS_POWERS; ++m) pw[m] = bs_mulmod(pw[m - 1], pw[m - 1]);
}

// A box's row from (key, nonce24): HSalsa20, keystream block 0, clamp, powers.
BS_FN void bs_box_keys_derive(bs_box_keys& row, const uint32_t key[8], const uint32_t nonce[6]) {
    bs_hsalsa(row.subkey, key, nonce);
    uint32_t ks[16];
    bs_salsa_block(ks, row.subkey, nonce + 4, 0);
    for (int i = 0; i < 4; ++i) row.s[i] = ks[4 + i];
    bs_powers(row.pw, bs_clamp_r(ks));
    row.pad[0] = 0;
}

// The MAC alone: the 32 bytes are the one-time key itself.
BS_FN void bs_mac_keys_derive(bs_box_keys& row, const uint32_t key[8]) {
    for (int i = 0; i < 8; ++i) row.subkey[i] = 0;
    for (int i = 0; i < 4; ++i) row.s[i] = key[4 + i];
    bs_powers(row.pw, bs_clamp_r(key));
    row.pad[0] = 0;
}

// --------------------------------------------------------- tile geometry

// slots of a box of `len` message bytes, the two key slots included
BS_FN uint64_t bs_slots(uint64_t len) { return 2 + (len + 15) / 16; }
// its tiles of S slots: at least one, so that every box has a partial
BS_FN uint64_t bs_tiles(uint64_t len, uint32_t S) { return (bs_slots(len) + S - 1) / S; }

struct bs_tile_geo {
    uint32_t used;   // slots of the tile that the box reaches: 1..S
    uint32_t shift;  // S - used: position pos holds slot pos - shift
    uint32_t nb;     // Poly1305 blocks among them: used, less tile 0's two
};

BS_FN bs_tile_geo bs_geo(uint64_t len, uint64_t tile, uint32_t S) {
    const uint64_t left = bs_slots(len) - tile * S;
    bs_tile_geo g;
    g.used = left < S ? uint32_t(left) : S;
    g.shift = S - g.used;
    g.nb = g.used - (tile == 0 ? 2u : 0u);
    return g;
}

// Message bytes that position `pos` of `tile` holds (0: an empty position or
// a key slot), and where they start: *off, a multiple of 16.
BS_FN uint32_t bs_position(uint64_t len, uint64_t tile, uint32_t S, const bs_tile_geo& g,
                           uint32_t pos, uint64_t* off) {
    *off = 0;
    if (pos < g.shift) return 0;
    const uint64_t slot = tile * S + (pos - g.shift);
    if (slot < 2) return 0;
    *off = (slot - 2) * 16;
    const uint64_t left = len - *off;  // slot < bs_slots(len): at least 1
    return left < 16 ? uint32_t(left) : 16u;
}

// Where slot `q` of a tile lies in its LDS image, in 16-byte units: thread t
// stores slots 4t..4t+3 one store instruction each, so without the swizzle
// sixteen lanes of one store would share four 16-byte bank groups. Readers
// walk consecutive slots and stay conflict-free either way.
BS_FN uint32_t bs_swizzle(uint32_t q) { return q ^ ((q >> 4) & 3u); }

// ------------------------------------------------------------- the host

// One box on the host, lane for lane what the K8 kernels do with tiles of B
// Salsa blocks (a power of two, 1..256). key: 32 bytes; nonce: 24 (unused by
// BS_MAC, whose key is the one-time key). in/out: len bytes (out unused by
// BS_MAC). tag: read by BS_OPEN, written by the other two. False iff an open
// failed; out is then zeros.
inline bool bs_host_box(int mode, uint32_t B, const uint8_t* key, const uint8_t* nonce,
                        const uint8_t* in, uint8_t* out, uint64_t len, uint8_t tag[16]) {
    const uint32_t S = 4 * B;
    uint32_t k[8], n[6] = {0, 0, 0, 0, 0, 0};
    std::memcpy(k, key, 32);
    if (mode != BS_MAC) std::memcpy(n, nonce, 24);
    bs_box_keys row;
    if (mode == BS_MAC)
        bs_mac_keys_derive(row, k);
    else
        bs_box_keys_derive(row, k, n);
    int logB = 0;
    while ((1u << logB) < B) ++logB;
    const uint64_t T = bs_tiles(len, S);
    std::vector<bs_fe> partial(T);
    std::vector<uint32_t> lds(size_t(S) * 4);
    std::vector<bs_fe> acc(B);
    for (uint64_t tile = 0; tile < T; ++tile) {
        const bs_tile_geo g = bs_geo(len, tile, S);
        if (mode != BS_MAC)
            for (uint32_t t = 0; t < B; ++t) {  // thread t: Salsa block tile*B + t
                uint32_t ks[16];
                bs_salsa_block(ks, row.subkey, n + 4, tile * B + t);
                for (uint32_t j = 0; j < 4; ++j)
                    std::memcpy(&lds[size_t(bs_swizzle(4 * t + j)) * 4], ks + 4 * j, 16);
            }
        for (uint32_t l = 0; l < B; ++l) {  // lane l: four passes, Horner by r^B
            acc[l] = bs_fe_zero();
            for (uint32_t p = 0; p < 4; ++p) {
                const uint32_t pos = p * B + l;
                uint64_t off;
                const uint32_t bytes = bs_position(len, tile, S, g, pos, &off);
                uint32_t w[4] = {0, 0, 0, 0}, c[4];
                if (bytes) std::memcpy(w, in + off, bytes);
                for (int i = 0; i < 4; ++i) c[i] = w[i];
                if (mode != BS_MAC && bytes) {
                    const uint32_t* ks = &lds[size_t(bs_swizzle(pos - g.shift)) * 4];
                    uint32_t x[4];
                    for (int i = 0; i < 4; ++i) x[i] = w[i] ^ ks[i];
                    bs_keep_bytes(x, bytes);
                    std::memcpy(out + off, x, bytes);
                    if (mode == BS_SEAL)
                        for (int i = 0; i < 4; ++i) c[i] = x[i];
                }
                acc[l] = bs_step(acc[l], row.pw[logB], bs_block(c, bytes));
            }
        }
        for (int m = 0; m < logB; ++m)  // the tree, level m by r^(2^m)
            for (uint32_t l = 0; l + (1u << m) < B; l += 2u << m)
                acc[l] = bs_step(acc[l], row.pw[m], acc[l + (1u << m)]);
        partial[tile] = bs_mulmod(acc[0], row.pw[0]);
    }
    // finish: lanes stride over tiles 0..T-2 by (r^S)^LANES, then a tree
    const uint64_t N = T - 1;
    bs_fe xp[7];  // (r^S)^(2^m)
    xp[0] = row.pw[logB + 2];
    for (int m = 1; m < 7; ++m) xp[m] = bs_mulmod(xp[m - 1], xp[m - 1]);
    const uint64_t lead = (BS_FINISH_LANES - N % BS_FINISH_LANES) % BS_FINISH_LANES;
    bs_fe lane[BS_FINISH_LANES];
    for (uint32_t l = 0; l < BS_FINISH_LANES; ++l) {
        lane[l] = bs_fe_zero();
        for (uint64_t u = l; u < N + lead; u += BS_FINISH_LANES)
            lane[l] = bs_step(lane[l], xp[6], u >= lead ? partial[u - lead] : bs_fe_zero());
    }
    for (int m = 0; m < 6; ++m)
        for (uint32_t l = 0; l + (1u << m) < BS_FINISH_LANES; l += 2u << m)
            lane[l] = bs_step(lane[l], xp[m], lane[l + (1u << m)]);
    const bs_fe h =
        bs_step(lane[0], bs_power(row.pw, bs_geo(len, T - 1, S).nb), partial[T - 1]);
    uint32_t t[4], given[4];
    bs_finish(t, h, row.s);
    if (mode != BS_OPEN) {
        std::memcpy(tag, t, 16);
        return true;
    }
    std::memcpy(given, tag, 16);
    const bool ok = bs_equal16(t, given);
    if (!ok) std::memset(out, 0, len);
    return ok;
}
