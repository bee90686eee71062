"""Shared inputs of the model-decoder tests (test_model_decode_cpu.py,
test_gpu_model_decode.py): hand-built bodies that a strict decoder rejects,
and seeded single-word corruptions of valid bodies. Everything is generated;
nothing is read."""
import struct
from functools import lru_cache

import numpy as np

import model_codec_inputs as mci

# elements as u32 words: sign | u64 count | digits, numerator then denominator
ZERO = (1, 0, 0, 2, 1, 0, 1)
ONE = (2, 1, 0, 1, 2, 1, 0, 1)
HALF = (2, 1, 0, 1, 2, 1, 0, 2)
INT_MIN32 = (0, 1, 0, 2**31, 2, 1, 0, 1)

ALL = frozenset(mci.DTYPES)
# label -> (words of X, the dtypes that must reject the body zero, X, one)
BAD_ELEMENTS = {
    "1/3": ((2, 1, 0, 1, 2, 1, 0, 3), ALL),
    "1/2 as an integer": (HALF, frozenset({"int32", "int64"})),
    "unreduced 2/2": ((2, 1, 0, 2, 2, 1, 0, 2), ALL),
    "leading zero digit": ((2, 2, 0, 1, 0, 2, 1, 0, 1), ALL),
    "2^24 + 1": ((2, 1, 0, 2**24 + 1, 2, 1, 0, 1), frozenset({"float32"})),
    "denominator sign 0": ((2, 1, 0, 1, 0, 1, 0, 1), ALL),
    "numerator sign 3": ((3, 1, 0, 1, 2, 1, 0, 1), ALL),
    "high count word 1": ((2, 1, 1, 1, 2, 1, 0, 1), ALL),
    "+2^31": ((2, 1, 0, 2**31, 2, 1, 0, 1), frozenset({"int32"})),
}


def body_of(elements, n=None, head=1):
    """head byte | u64 n (the element count unless given) | the elements' words."""
    words = [w for el in elements for w in el]
    n = len(elements) if n is None else n
    return struct.pack("<BQ", head, n) + np.array(words, dtype="<u4").tobytes()


def element_bodies(name):
    """label -> (body zero, X, one; whether `name` must reject it)."""
    return {label: (body_of([ZERO, x, ONE]), name in dtypes)
            for label, (x, dtypes) in BAD_ELEMENTS.items()}


def framing_bodies(name):
    """The valid body zero, X, one (X = 1/2, or -2^31 for the integer types)
    and label -> a body with a defect of length, count or head."""
    els = [ZERO, HALF if name.startswith("float") else INT_MIN32, ONE]
    good = body_of(els)
    bad = {
        "last word missing": good[:-4],
        "one zero word more": good + bytes(4),
        "n + 1": body_of(els, n=4),
        "n - 1": body_of(els, n=2),
        "head 00": body_of(els, head=0),
        "head 02": body_of(els, head=2),
        "one byte more": good + b"\0",
        "two bytes less": good[:-2],
        "shorter than a head": good[:5],
    }
    return good, bad


@lru_cache(maxsize=None)
def mixed_vector(name, n, seed=77):
    """n elements drawn from the edge and random vectors: every element length."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([mci.edges(name), mci.random_vector(name)])
    v = pool[rng.integers(0, len(pool), n)]
    v.setflags(write=False)
    return v


def corruptions(body, cases, seed):
    """`cases` copies of `body`, each with one random element word overwritten
    by a value from {0, 1, 2, 3, 35, 36, 2^32 - 1, random}."""
    rng = np.random.default_rng(seed)
    words = (len(body) - 9) // 4
    for _ in range(cases):
        at = int(rng.integers(0, words))
        pick = int(rng.integers(0, 8))
        value = (0, 1, 2, 3, 35, 36, 2**32 - 1, int(rng.integers(0, 2**32)))[pick]
        out = bytearray(body)
        out[9 + 4 * at: 13 + 4 * at] = struct.pack("<I", value)
        yield bytes(out)
