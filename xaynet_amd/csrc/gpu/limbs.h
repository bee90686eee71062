// Fixed-width multi-limb integers for group orders in [2^64, 2^320): N
// little-endian u64 limbs, N a compile-time constant. Shared by the kernels
// (kernels.hip) and the host code that prepares their constants
// (hip_bindings.cpp), so it compiles as plain C++ too.
//
// Every loop has compile-time bounds and every limb index is a constant after
// unrolling: the limbs stay in registers. Nothing here indexes a limb array
// by a run-time value — whole-limb moves by a run-time count are written as
// N conditional one-limb steps.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define ML_FN __host__ __device__ __forceinline__
#else
#define ML_FN inline
#endif

#define ML_MAX_LIMBS 5

// Multi-limb constants (orders, exp_shift, offsets) cross the launcher ABI by
// value in this struct; limbs beyond the value's width are zero.
struct xhip_limbs {
    uint64_t w[ML_MAX_LIMBS];
};

template <int N>
struct limbs {
    uint64_t w[N];
};

template <int N>
ML_FN limbs<N> ml_zero() {
    limbs<N> r;
#pragma unroll
    for (int j = 0; j < N; ++j) r.w[j] = 0;
    return r;
}

// low N limbs of a launcher constant
template <int N>
ML_FN limbs<N> ml_from(const xhip_limbs& c) {
    static_assert(N <= ML_MAX_LIMBS, "a launcher constant has ML_MAX_LIMBS limbs");
    limbs<N> r;
#pragma unroll
    for (int j = 0; j < N; ++j) r.w[j] = c.w[j];
    return r;
}

// zero-extend or truncate to M limbs
template <int M, int N>
ML_FN limbs<M> ml_resize(const limbs<N>& a) {
    constexpr int K = M < N ? M : N;
    limbs<M> r;
#pragma unroll
    for (int j = 0; j < K; ++j) r.w[j] = a.w[j];
#pragma unroll
    for (int j = K; j < M; ++j) r.w[j] = 0;
    return r;
}

template <int N>
ML_FN bool ml_is_zero(const limbs<N>& a) {
    uint64_t any = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) any |= a.w[j];
    return any == 0;
}

// a >= b
template <int N>
ML_FN bool ml_geq(const limbs<N>& a, const limbs<N>& b) {
    uint64_t borrow = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        uint64_t d = a.w[j] - b.w[j];
        borrow = uint64_t(a.w[j] < b.w[j]) | uint64_t(d < borrow);
    }
    return borrow == 0;
}

// a -= b; returns the borrow out of the top limb
template <int N>
ML_FN uint64_t ml_sub(limbs<N>& a, const limbs<N>& b) {
    uint64_t borrow = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        uint64_t d = a.w[j] - b.w[j];
        uint64_t out = uint64_t(a.w[j] < b.w[j]) | uint64_t(d < borrow);
        a.w[j] = d - borrow;
        borrow = out;
    }
    return borrow;
}

// a += b; returns the carry out of the top limb
template <int N>
ML_FN uint64_t ml_add(limbs<N>& a, const limbs<N>& b) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        uint64_t s = a.w[j] + b.w[j];
        uint64_t out = uint64_t(s < b.w[j]);
        s += carry;
        out |= uint64_t(s < carry);
        a.w[j] = s;
        carry = out;
    }
    return carry;
}

// a += x (one word); returns the carry out
template <int N>
ML_FN uint64_t ml_add_word(limbs<N>& a, uint64_t x) {
    uint64_t carry = x;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        uint64_t s = a.w[j] + carry;
        carry = uint64_t(s < carry);
        a.w[j] = s;
    }
    return carry;
}

// a <<= s, s in 1..63 (bits shifted out of the top limb are dropped)
template <int N>
ML_FN void ml_shl_bits(limbs<N>& a, int s) {
#pragma unroll
    for (int j = N - 1; j > 0; --j) a.w[j] = (a.w[j] << s) | (a.w[j - 1] >> (64 - s));
    a.w[0] <<= s;
}

// a >>= s, s in 1..63
template <int N>
ML_FN void ml_shr_bits(limbs<N>& a, int s) {
#pragma unroll
    for (int j = 0; j < N - 1; ++j) a.w[j] = (a.w[j] >> s) | (a.w[j + 1] << (64 - s));
    a.w[N - 1] >>= s;
}

// a <<= 64 (one whole limb)
template <int N>
ML_FN void ml_shl_limb(limbs<N>& a) {
#pragma unroll
    for (int j = N - 1; j > 0; --j) a.w[j] = a.w[j - 1];
    a.w[0] = 0;
}

// a >>= 64; returns the limb shifted out
template <int N>
ML_FN uint64_t ml_shr_limb(limbs<N>& a) {
    uint64_t out = a.w[0];
#pragma unroll
    for (int j = 0; j < N - 1; ++j) a.w[j] = a.w[j + 1];
    a.w[N - 1] = 0;
    return out;
}

// a <<= s for any s in 0 .. 64*N-1 (the caller knows the result fits)
template <int N>
ML_FN void ml_shl(limbs<N>& a, int s) {
#pragma unroll
    for (int k = 0; k < N - 1; ++k) {
        if (s >= 64) {
            ml_shl_limb(a);
            s -= 64;
        }
    }
    if (s) ml_shl_bits(a, s);
}

// a >>= s for any s >= 0; returns whether any 1 bit was shifted out
template <int N>
ML_FN bool ml_shr_sticky(limbs<N>& a, int s) {
    uint64_t lost = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (s >= 64) {
            lost |= ml_shr_limb(a);
            s -= 64;
        }
    }
    if (s >= 64) {  // s was >= 64*N: everything is gone
        lost |= uint64_t(!ml_is_zero(a));
        a = ml_zero<N>();
        return lost != 0;
    }
    if (s) {
        lost |= a.w[0] << (64 - s);
        ml_shr_bits(a, s);
    }
    return lost != 0;
}

// v mod order by binary shift-subtract over an L+1-limb window (the wide
// analog of u192_mod_u128). v must be below 2^(64*(L+1) - 1); the loop count
// is the bit-length difference of v and order, a handful for the sums of a
// round.
template <int L>
ML_FN limbs<L> ml_mod(limbs<L + 1> v, const limbs<L>& order) {
    limbs<L + 1> m = ml_resize<L + 1>(order);
    int shift = 0;
    // grow m while (m << 1) <= v; the guard keeps m below 2^(64*(L+1) - 1)
    while (!(m.w[L] >> 62)) {
        limbs<L + 1> m2 = m;
        ml_shl_bits(m2, 1);
        if (!ml_geq(v, m2)) break;
        m = m2;
        ++shift;
    }
    for (; shift >= 0; --shift) {
        if (ml_geq(v, m)) ml_sub(v, m);
        ml_shr_bits(m, 1);
    }
    return ml_resize<L>(v);
}

// a = (a + b) mod order for canonical a, b (< order): the sum is below
// 2*order, so one conditional subtraction; a carry out of the top limb means
// the wrapped difference is already the residue.
template <int L>
ML_FN void ml_mod_add(limbs<L>& a, const limbs<L>& b, const limbs<L>& order) {
    uint64_t carry = ml_add(a, b);
    if (carry || ml_geq(a, order)) ml_sub(a, order);
}

// (a - b) mod order for canonical a, b
template <int L>
ML_FN limbs<L> ml_mod_sub(limbs<L> a, const limbs<L>& b, const limbs<L>& order) {
    if (ml_sub(a, b)) ml_add(a, order);  // went negative: wraps back into [0, order)
    return a;
}

// a = a / d, returns a % d (d != 0): schoolbook division by one word, top limb
// first. Written as N rounds on the TOP limb with a whole-limb rotate between
// them, so the loop need not unroll around the 128-by-64-bit division.
template <int N>
ML_FN uint64_t ml_divrem_word(limbs<N>& a, uint64_t d) {
    uint64_t rem = 0;
#pragma unroll 1
    for (int k = 0; k < N; ++k) {
        unsigned __int128 cur = ((unsigned __int128)rem << 64) | a.w[N - 1];
        uint64_t q = uint64_t(cur / d);  // rem < d, so the quotient fits a word
        rem = uint64_t(cur - (unsigned __int128)q * d);
        ml_shl_limb(a);
        a.w[0] = q;
    }
    return rem;
}

// a * x (one word), result in N limbs (the caller knows it fits)
template <int N>
ML_FN limbs<N> ml_mul_word(const limbs<N>& a, uint64_t x) {
    limbs<N> r;
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        unsigned __int128 p = (unsigned __int128)a.w[j] * x + carry;
        r.w[j] = uint64_t(p);
        carry = uint64_t(p >> 64);
    }
    return r;
}

// Nearest double (ties to even) of a: ONE rounding, whatever the width. The
// value is normalised so its top limb is non-zero and its top bit set; the 64
// leading bits with everything below OR-ed into bit 0 (a sticky bit, far
// below the 53-bit rounding position) round exactly like the full integer.
template <int N>
ML_FN double ml_to_double(limbs<N> a) {
    if (ml_is_zero(a)) return 0.0;
    int moved = 0;  // bits shifted up
#pragma unroll
    for (int k = 0; k < N - 1; ++k) {
        if (a.w[N - 1] == 0) {
            ml_shl_limb(a);
            moved += 64;
        }
    }
    int s = __builtin_clzll(a.w[N - 1]);
    if (s) ml_shl_bits(a, s);
    moved += s;
    uint64_t sticky = 0;
#pragma unroll
    for (int j = 0; j < N - 1; ++j) sticky |= a.w[j];
    uint64_t top = a.w[N - 1] | uint64_t(sticky != 0);
    return ldexp(double(top), 64 * (N - 1) - moved);
}

// Digit planes -> the integer they spell, v = sum_d plane[d][i] << (s * d),
// built top-down as v = (v << s) + plane[d][i]. Planes hold plain SUMS of
// digits, so an entry may exceed 2^s; s is 1..63.
template <int N>
ML_FN limbs<N> ml_from_planes(const uint64_t* planes, uint64_t len, uint64_t i, int n_planes,
                              int s) {
    limbs<N> v = ml_zero<N>();
    for (int d = n_planes - 1; d >= 0; --d) {
        ml_shl_bits(v, s);
        ml_add_word(v, planes[uint64_t(d) * len + i]);
    }
    return v;
}

// floor(|y| * E) for a finite double y, exactly: |y| = m * 2^e with a 53-bit
// integer mantissa m, so the product is (m * E) shifted by e. `inexact`
// reports whether the floor dropped a fraction (ceil = floor + 1 then). The
// caller knows |y| * E fits N limbs, and so does 2^53 * E.
template <int N>
ML_FN limbs<N> ml_quantize(double y, const limbs<N>& E, bool& inexact) {
    inexact = false;
    y = fabs(y);
    if (y == 0.0) return ml_zero<N>();
    int e;
    double m = frexp(y, &e);                         // y = m * 2^e, m in [0.5, 1)
    uint64_t mi = uint64_t(m * 9007199254740992.0);  // m * 2^53, exact
    limbs<N> prod = ml_mul_word(E, mi);
    int shift = 53 - e;
    if (shift >= 0)
        inexact = ml_shr_sticky(prod, shift);
    else
        ml_shl(prod, -shift);
    return prod;
}
