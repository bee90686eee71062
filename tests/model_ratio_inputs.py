"""Shared inputs of the rational model-decode tests (test_model_ratio_cpu.py,
test_gpu_model_ratio.py): bodies packed from (numerator, denominator) pairs and
their reference, Fraction rounded once (unmask_exact_inputs.round_exact) or
truncated toward zero. Everything is generated; nothing is read."""
import random
from fractions import Fraction
from functools import lru_cache

import numpy as np

from model_decode_inputs import ZERO, ONE, body_of  # noqa: F401
from unmask_exact_inputs import round_exact

T24, T53, TOP = 2**24 + 1, 2**53 + 1, 2**320 - 1  # p + 1-bit ties, ten digits of ones
# every pair is a value of the float types; an integer type rejects those whose
# truncated quotient it does not hold
VALUES = [(0, 7), (1, 3), (-1, 3), (7, 2), (-7, 2)]
# unreduced ties at p + 1 bits and the integers on either side
VALUES += [(3 * t + d, 3) for t in (T24, T53) for d in (0, -1, 1)]
# m + 1/2 over 6: m even stays, m odd goes up
VALUES += [(3 * (2 * m + 1), 6) for m in (2**23 + 2, 2**23 + 1, 2**52 + 2, 2**52 + 1)]
# the f32 subnormal grid, below half its unit (+0 and -0), saturation, 10 / 10 digits
VALUES += [(1, 3 << 148), (1, 3 << 151), (-1, 3 << 151), (TOP, 1), (-TOP, 1),
           (TOP, 2**319 + 1), (-TOP, TOP - 2)]
# the ends of the integer types, over 1 and unreduced over 3, and one past them
VALUES += [(k * v, k) for v in (2**31 - 1, 1 - 2**31, -2**31, 2**63 - 1, 1 - 2**63, -2**63,
                                2**31, 2**63) for k in (1, 3)]
VALUES += [(-(3 * 2**31 + 2), 3), (3 * 2**63 + 2, 3)]  # truncate to -2^31, to +2^63

# words no mode takes
BAD = {
    "eleven-digit numerator": (2, 11, 0, *([1] * 11), 2, 1, 0, 3),
    "eleven-digit denominator": (2, 1, 0, 1, 2, 11, 0, *([1] * 11)),
    "Minus denominator": (2, 1, 0, 1, 0, 1, 0, 3),
    "leading zero digit": (2, 2, 0, 1, 0, 2, 1, 0, 3),
    "leading zero digit below": (2, 1, 0, 1, 2, 2, 0, 3, 0),
    "NoSign with a digit": (1, 1, 0, 1, 2, 1, 0, 3),
    "Plus without digits": (2, 0, 0, 2, 1, 0, 3),
}


def _digits(x):
    return [x >> s & 0xFFFFFFFF for s in range(0, x.bit_length(), 32)]


def element(num, den):
    n, d = _digits(abs(num)), _digits(den)
    return (1 if num == 0 else 2 if num > 0 else 0, len(n), 0, *n, 2, len(d), 0, *d)


def reference(name, num, den):
    """The value of num / den as dtype `name`, or None where it has none."""
    if name.startswith("float"):
        return round_exact(Fraction(num, den), np.dtype(name).type)
    t = abs(num) // den * (1 if num > 0 else -1)
    info = np.iinfo(name)
    return np.dtype(name).type(t) if info.min <= t <= info.max else None


def split(name, pairs=VALUES):
    """(body of the pairs `name` holds, their reference; the pairs it rejects)."""
    refs = [reference(name, *p) for p in pairs]
    held = [element(*p) for p, r in zip(pairs, refs) if r is not None]
    want = np.array([r for r in refs if r is not None], dtype=name)
    return body_of(held), want, [p for p, r in zip(pairs, refs) if r is None]


def check(got, want, what):
    """Bit for bit: -0.0 is not +0.0."""
    assert got is not None and got.dtype == want.dtype and got.shape == want.shape, what
    uint = np.uint32 if want.dtype.itemsize == 4 else np.uint64
    bad = np.nonzero(got.view(uint) != want.view(uint))[0]
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def random_pairs(n, seed, max_digits=3, quotient_bits=None):
    """n pairs of up to max_digits digits a side; quotient_bits bounds |num / den|."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        den = rng.getrandbits(rng.randrange(1, 32 * max_digits + 1)) | 1
        top = 32 * max_digits if quotient_bits is None else \
            min(32 * max_digits, den.bit_length() - 1 + quotient_bits)
        out.append((rng.choice((1, -1)) * rng.getrandbits(rng.randrange(0, top + 1)), den))
    return out


@lru_cache(maxsize=None)
def block_edges(bw):
    """A few thousand pairs: a 10 / 10-digit element (26 words, the longest the
    mode takes) that starts in the last word of the first block, 7-word zeros on
    both sides of the second block edge, 8-word fillers and random pairs."""
    def filler(words):  # 7a + 8b
        b = words % 7
        return [(0, 1)] * ((words - 8 * b) // 7) + [(5, 3)] * b

    pairs = filler(bw - 1) + [(-TOP, TOP - 2)] + filler(2 * bw - 7 - (bw - 1 + 26)) + [(0, 1)] * 2
    starts = np.cumsum([0] + [len(element(*p)) for p in pairs])
    assert bw - 1 in starts and 2 * bw - 7 in starts and 2 * bw in starts
    return tuple(pairs + random_pairs(2500, 16))
