"""Shared inputs of the model-encoder tests (test_model_codec_cpu.py,
test_gpu_model_codec.py): per dtype an edge vector, a seeded random vector and
a heavy-tail mix. Everything is generated from seeds; nothing is read."""
from functools import lru_cache

import numpy as np

DTYPES = ("float32", "float64", "int32", "int64")
# mask::DataType codes
DTYPE_CODE = {"float32": 0, "float64": 1, "int32": 2, "int64": 3}

# (mantissa bits, exponent of the least subnormal, exponent of the top power of two)
_FLOAT_SHAPE = {"float32": (24, -149, 127), "float64": (53, -1074, 1023)}
_UINT = {"float32": np.uint32, "float64": np.uint64}


def _from_bits(name, bits):
    return np.array(bits, dtype=_UINT[name]).view(name)


def _ldexp(name, mant, exps):
    """mant * 2^e for every e, in `name`; exact wherever the value fits."""
    with np.errstate(over="ignore", under="ignore"):
        v = np.ldexp(np.float64(mant), np.asarray(list(exps), dtype=np.int64))
        return v.astype(name)


def _float_edges(name):
    p, emin, emax = _FLOAT_SHAPE[name]
    info = np.finfo(name)
    frac_bits = p - 1
    frac_ones = (1 << frac_bits) - 1
    full = (1 << p) - 1  # a full odd mantissa
    parts = [
        np.array([0.0, -0.0, 1.0, -1.0, np.nan, np.inf, -np.inf], dtype=name),
        # least and greatest subnormal, least normal with a full mantissa, tiny
        _from_bits(name, [1, frac_ones, (1 << frac_bits) | frac_ones, 1 << frac_bits]),
        -_from_bits(name, [1, frac_ones, (1 << frac_bits) | frac_ones]),
        np.array([info.max, info.min, info.tiny, info.eps], dtype=name),
        np.array([-2.0**31, 2.0**31 - 1, -2.0**63, 2.0**63 - 1], dtype=name),  # INT_MIN, INT_MAX
        # 2^k for every k the type reaches
        _ldexp(name, 1.0, range(emin, emax + 1)),
        -_ldexp(name, 1.0, range(emin, emax + 1, 7)),
        # a full odd mantissa shifted across each 32-bit digit boundary
        _ldexp(name, float(full), range(0, 71)),
        -_ldexp(name, float(full), range(0, 71, 3)),
        _ldexp(name, 3.0, range(0, 71)),
    ]
    # denominators 2^k at k = 31, 0, 1 (mod 32), under a small and a full mantissa
    ks = [k for k in range(1, -emin + 1) if k % 32 in (31, 0, 1)]
    parts += [_ldexp(name, 1.0, [-k for k in ks]),
              _ldexp(name, 3.0, [-k for k in ks if k < -emin]),
              -_ldexp(name, 5.0, [-k for k in ks if k < -emin - 1]),
              _ldexp(name, float(full), [-k for k in ks if k <= -emin]),
              _ldexp(name, float(full), [-k for k in range(p - 2, p + 40)])]
    return np.concatenate(parts)


def _int_edges(name):
    info = np.iinfo(name)
    bits = info.bits
    vals = [0, 1, -1, info.max, info.min, info.max - 1, info.min + 1,
            -(2**31), 2**31 - 1, -(2**31) + 1]
    vals += [2**k for k in range(bits - 1)] + [-(2**k) for k in range(bits)]
    vals += [(2**31 - 1) * 2**k for k in range(bits) if (2**31 - 1) * 2**k <= info.max]
    vals += [-(2**31 - 1) * 2**k for k in range(bits) if (2**31 - 1) * 2**k <= info.max]
    vals += [3 * 2**k for k in range(bits - 2)]
    return np.array([v for v in vals if info.min <= v <= info.max], dtype=name)


@lru_cache(maxsize=None)
def edges(name):
    v = _float_edges(name) if name in _FLOAT_SHAPE else _int_edges(name)
    v.setflags(write=False)
    return v


@lru_cache(maxsize=None)
def random_vector(name, n=6000, seed=1105):
    rng = np.random.default_rng(seed)
    if name in _FLOAT_SHAPE:
        # weights in (-1, 1), plus raw bit patterns: every exponent, NaNs too
        unit = rng.uniform(-1, 1, n // 2).astype(name)
        raw = rng.integers(0, 2 ** (8 * np.dtype(name).itemsize), n - n // 2,
                           dtype=np.uint64).astype(_UINT[name]).view(name)
        v = np.concatenate([unit, raw])
    else:
        info = np.iinfo(name)
        small = rng.integers(-1000, 1000, n // 2).astype(name)
        wide = rng.integers(info.min, info.max, n - n // 2, dtype=np.int64,
                            endpoint=True).astype(name)
        v = np.concatenate([small, wide])
    rng.shuffle(v)
    v.setflags(write=False)
    return v


@lru_cache(maxsize=None)
def heavy_tail(name, n=8192, seed=2207):
    """Runs of zeros (7 words), of the type's longest elements and of typical
    weights, with run lengths from 1 to a few blocks: block totals differ
    widely."""
    rng = np.random.default_rng(seed)
    if name in _FLOAT_SHAPE:
        p, _, _ = _FLOAT_SHAPE[name]
        frac_bits = p - 1
        longest = np.concatenate([
            _from_bits(name, [(1 << frac_bits) | ((1 << frac_bits) - 1)]),  # 42 / 12 words
            np.array([np.finfo(name).max], dtype=name)])
        typical = rng.uniform(-1, 1, 4096).astype(name)
    else:
        info = np.iinfo(name)
        longest = np.array([info.max, info.min + 1], dtype=name)
        typical = rng.integers(-1000, 1000, 4096).astype(name)
    out = np.zeros(n, dtype=name)
    at = 0
    while at < n:
        run = int(rng.choice([1, 3, 64, 255, 257, 700]))
        kind = rng.integers(0, 3)
        if kind == 1:
            out[at:at + run] = np.resize(longest, run)[: n - at]
        elif kind == 2:
            out[at:at + run] = rng.choice(typical, run)[: n - at]
        at += run
    out.setflags(write=False)
    return out


def vectors(name):
    """name -> {label: vector}"""
    return {"edges": edges(name), "random": random_vector(name), "heavy": heavy_tail(name)}


def tiled(vec, n):
    """`vec` repeated (or cut) to n elements."""
    return np.resize(vec, n)
