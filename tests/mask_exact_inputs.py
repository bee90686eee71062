"""Inputs shared by the exact-masking tests (test_mask_exact_cpu.py,
test_gpu_mask_exact.py): the config matrix, weight vectors full of edge cases,
the scalars, and the oracle values everything is compared with."""
from fractions import Fraction
from functools import lru_cache

import numpy as np

from xaynet_amd import _core

mk = _core.mask

N = 1031  # four blocks of 256 threads and a tail of 7
SEED = bytes(range(7, 39))

# (group, dtype, bound, model)
CONFIGS = [
    (1, 0, 0, 6),
    (1, 0, 2, 6),
    (1, 0, 6, 3),     # 65-bit order, the smallest wide one
    (1, 1, 0, 3),
    (1, 1, 4, 9),
    (1, 2, 0, 6),
    (1, 3, 0, 6),
    (1, 3, 6, 6),
    (1, 2, 255, 3),   # L = 2
    (1, 3, 255, 12),  # L = 3
    (1, 0, 255, 3),   # L = 5
]

# the uniform part of a float vector spans +-scale, past the clamp bound
FLOAT_SCALES = {
    (1, 0, 0, 6): 1.0,
    (1, 0, 2, 6): 150.0,
    (1, 0, 6, 3): 2e6,
    (1, 1, 0, 3): 1.0,
    (1, 1, 4, 9): 2e4,
    (1, 0, 255, 3): 1e30,
}

SCALARS = [(1, 1), (1, 3), (2, 7), (1, 1024), (3, 2), (5, 1), (7, 2**40),
           (2**62 - 1, 2**61 + 1), (1, 2**62 + 3)]
GPU_SCALARS = [(1, 1), (1, 3), (2, 7), (3, 2)]

NP_DTYPES = {0: np.float32, 1: np.float64, 2: np.int32, 3: np.int64}

# add_shift by bound; a Bmax bound is the data type's own extreme
ADD_SHIFTS = {0: 1, 2: 100, 4: 10**4, 6: 10**6}
BMAX_ADD_SHIFTS = {0: (2**24 - 1) << 104, 2: 2**31, 3: 2**63}


def add_shift(cfg_args) -> int:
    _, dtype, bound, _ = cfg_args
    return BMAX_ADD_SHIFTS[dtype] if bound == 255 else ADD_SHIFTS[bound]


def clamped_scalar(cfg_args, num: int, den: int):
    """num/den clamped to the unit config's add_shift (the tests use the vect
    config for the unit too), in lowest terms."""
    s = min(Fraction(num, den), Fraction(add_shift(cfg_args)))
    return s.numerator, s.denominator


def pair_of(cfg_args):
    c = mk.MaskConfig(*cfg_args)
    return mk.MaskConfigPair(c, c)


def weights(cfg_args, n: int = N) -> np.ndarray:
    """n elements of the config's dtype: edge cases first, then seeded
    uniform values that reach past the clamp bound."""
    _, dtype, bound, _ = cfg_args
    np_dt = NP_DTYPES[dtype]
    rng = np.random.default_rng(1000 * dtype + bound)
    if dtype in (0, 1):
        fi = np.finfo(np_dt)
        one = np_dt(1)
        pos = [0.0, 1.0, np.nextafter(one, np_dt(0)), np.nextafter(one, np_dt(2)),
               fi.tiny, fi.smallest_subnormal, fi.max, np.inf,
               1e-10, 0.5e-10, 3e-10, 1.0 / 3.0, 3.0]
        head = [s * np_dt(x) for x in pos for s in (1, -1)] + [np.nan]
        scale = FLOAT_SCALES[cfg_args]
        rest = rng.uniform(-scale, scale, n - len(head))
        w = np.concatenate([np.array(head, dtype=np_dt), rest.astype(np_dt)])
    else:
        ii = np.iinfo(np_dt)
        head = [0, 1, -1, ii.max, ii.min]
        if bound == 255:
            rest = rng.integers(ii.min, ii.max, n - len(head), dtype=np_dt, endpoint=True)
        else:
            rest = rng.integers(-2 * 10**6, 2 * 10**6, n - len(head), endpoint=True)
        w = np.concatenate([np.array(head, dtype=np_dt), rest.astype(np_dt)])
    assert w.dtype == np_dt and w.shape == (n,)
    return w


@lru_cache(maxsize=None)
def oracle(cfg_args, num: int, den: int):
    """The rational masker's update for weights(cfg_args) and scalar num/den,
    computed once per case and shared."""
    return mk.mask_model_oracle(SEED, mk.Scalar(num, den), weights(cfg_args), pair_of(cfg_args))


@lru_cache(maxsize=None)
def mask_elements(cfg_args):
    m = mk.derive_mask(SEED, N, pair_of(cfg_args))
    return [int(m.element(i)) for i in range(N)]


def oracle_values(cfg_args, num: int, den: int):
    """What the oracle quantised each element to: (wire element - mask
    element) mod order."""
    order = int(mk.MaskConfig(*cfg_args).order)
    obj = oracle(cfg_args, num, den)
    return [(int(obj.element(i)) - m) % order for i, m in enumerate(mask_elements(cfg_args))]
