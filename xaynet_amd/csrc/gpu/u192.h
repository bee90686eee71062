// 192-bit window arithmetic of the u128-order finalize kernels (K2
// canonicalize / recode, K4 unmask): digit planes -> one u192 -> value mod
// order. Shared by the kernels (kernels.hip) and the host instantiation that
// the CPU tests run (mask_bindings.cpp, _core.mask.planes_mod), so it compiles
// as plain C++ too.
#pragma once

#include "limbs.h"

struct u192 {
    uint64_t w[3];  // little-endian
};

ML_FN void u192_shl1(u192& a) {
    a.w[2] = (a.w[2] << 1) | (a.w[1] >> 63);
    a.w[1] = (a.w[1] << 1) | (a.w[0] >> 63);
    a.w[0] <<= 1;
}

ML_FN bool u192_geq(const u192& a, const u192& b) {
    if (a.w[2] != b.w[2]) return a.w[2] > b.w[2];
    if (a.w[1] != b.w[1]) return a.w[1] > b.w[1];
    return a.w[0] >= b.w[0];
}

ML_FN void u192_sub(u192& a, const u192& b) {
    unsigned __int128 d0 = (unsigned __int128)a.w[0] - b.w[0];
    unsigned __int128 d1 = (unsigned __int128)a.w[1] - b.w[1] - ((d0 >> 64) ? 1 : 0);
    a.w[0] = uint64_t(d0);
    a.w[2] = a.w[2] - b.w[2] - ((d1 >> 64) ? 1 : 0);
    a.w[1] = uint64_t(d1);
}

// value (below 2^191: the launchers check the plane shape) mod order (u128,
// > 2^64): classic binary shift-subtract, one iteration per bit that the
// value is longer than the order.
ML_FN unsigned __int128 u192_mod_u128(u192 v, unsigned __int128 order) {
    u192 m{{uint64_t(order), uint64_t(order >> 64), 0}};
    int shift = 0;
    // grow m while (m << 1) <= v (m stays below 2^191 by the loop guard)
    while (!(m.w[2] >> 62)) {
        u192 m2 = m;
        u192_shl1(m2);
        if (!u192_geq(v, m2)) break;  // m2 > v
        m = m2;
        ++shift;
    }
    for (; shift >= 0; --shift) {
        if (u192_geq(v, m)) u192_sub(v, m);
        m.w[0] = (m.w[0] >> 1) | (m.w[1] << 63);
        m.w[1] = (m.w[1] >> 1) | (m.w[2] << 63);
        m.w[2] >>= 1;
    }
    return ((unsigned __int128)v.w[1] << 64) | v.w[0];
}

// Recombine `n_planes` digit planes (plane stride `len`) into one u192:
// v = sum_d plane[d][i] << (digit_bits * d), built top-down as
// v = (v << digit_bits) + plane[d][i] with carry. digit_bits is 1..63; the
// planes hold plain integer SUMS of digits, so a plane entry may be anything
// below 2^64. The launchers refuse plane shapes whose total could leave the
// u192_mod_u128 window: (n_planes - 1) * digit_bits + 64 <= 191.
// DB is the compile-time digit width (32 for the accumulator), 0 = runtime.
template <int DB>
ML_FN u192 u192_from_planes(const uint64_t* __restrict__ planes, uint64_t len, uint64_t i,
                            int n_planes, int digit_bits) {
    const int s = DB ? DB : digit_bits;
    u192 v{{0, 0, 0}};
    for (int d = n_planes - 1; d >= 0; --d) {
        v.w[2] = (v.w[2] << s) | (v.w[1] >> (64 - s));
        v.w[1] = (v.w[1] << s) | (v.w[0] >> (64 - s));
        v.w[0] = (v.w[0] << s);
        unsigned __int128 t = (unsigned __int128)v.w[0] + planes[uint64_t(d) * len + i];
        v.w[0] = uint64_t(t);
        if (t >> 64) {  // carry
            if (++v.w[1] == 0) ++v.w[2];
        }
    }
    return v;
}

// Digit j (digit_bits wide) of a u128 value; digits may straddle the lo/hi
// word boundary. Shifts of 128 or more (k * digit_bits may overshoot) are 0.
ML_FN uint64_t u128_digit(unsigned __int128 v, int j, int digit_bits) {
    int sh = digit_bits * j;
    if (sh >= 128) return 0;
    return uint64_t(v >> sh) & ((uint64_t(1) << digit_bits) - 1);
}
