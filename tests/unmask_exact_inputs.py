"""Inputs and the reference of the exact float unmask (exact=True).

Shared by tests/test_unmask_exact_cpu.py (the element function on the host,
CpuPlaneAggregator, two gloo ranks) and tests/test_gpu_unmask_exact.py (the
k4_unmask_exact kernels). A plain module, no fixtures.

The reference is the rational the coordinator publishes, Fraction(d, Q) with

    t = (planes mod order - mask) mod order
    d = t - C,            C = nb * add_shift * exp_shift
    Q = exp_shift * scalar_sum = n1 - nb * add_1 * exp_1   (same config twice)

rounded ONCE to the output type by `round_exact`: nearest, ties to even, on
the subnormal grid below the normal range, saturated at the largest finite
value. It is unmask_edges.round_once with those two ends added, and works on
integers alone (one divmod), not as the element function under test does.

Rounds are crafted straight from (Q, [d_i]) for any config the engines cover,
Bmax included: t_i = C + d_i, a random canonical mask, planes lifted by
multiples of the order as unmask_edges.forge lifts them, and the masked unit
sum chosen so that _unmask_scalars derives exactly Q.
"""
import functools
import random
from fractions import Fraction

import numpy as np
import torch

import unmask_edges as ue
from unmask_edges import mk

N = ue.N      # 1027: four full 256-thread workgroups and a tail of 3
CUT = ue.CUT  # the two column shards

# exp_shift, add_shift of the Bmax configs per mask::DataType, kept apart from
# the engine's own table (test_reference_is_the_oracle pins the F32 pair)
BMAX_SHIFTS = {0: (10**45, (2**24 - 1) << 104), 2: (10**10, 2**31), 3: (10**10, 2**63)}

# np type -> (precision, log2 of the smallest subnormal, largest finite value)
FORMATS = {
    np.float32: (24, -149, (2**24 - 1) << 104),
    np.float64: (53, -1074, (2**53 - 1) << 971),
}
DTYPE_CODE = {np.float32: 0, np.float64: 1}


def shifts(cfg_args):
    """(add_shift, exp_shift) as integers, Bmax included."""
    _, dtype, bound, _ = cfg_args
    if bound == 255:
        exp, add = BMAX_SHIFTS[dtype]
        return add, exp
    return ue.shifts(cfg_args)


# ------------------------------------------------------------------ reference


def round_exact(q: Fraction, np_type):
    """q rounded once to np_type: nearest, ties to even; subnormal grid at the
    bottom, saturation at +-max at the top; a negative q that rounds to zero
    keeps its sign, q == 0 is +0."""
    p, min_unit, top = FORMATS[np_type]
    if q == 0:
        return np_type(0.0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()  # floor(log2 a) or one above
    if a < Fraction(2) ** e:
        e -= 1
    unit = max(e - (p - 1), min_unit)  # log2 of the last place
    scaled = a / Fraction(2) ** unit
    m, rest = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rest
    if twice > scaled.denominator or (twice == scaled.denominator and m & 1):
        m += 1
    value = min(Fraction(m) * Fraction(2) ** unit, Fraction(top))
    out = float(value)  # exact: at most 53 bits, in range
    assert Fraction(out) == value
    return np_type(-out if q < 0 else out)


def bits(arr):
    """Floats as their integer bit patterns (so -0.0 != +0.0 and no NaN rule)."""
    arr = np.ascontiguousarray(arr)
    return arr.view(np.uint32 if arr.dtype == np.float32 else np.uint64)


# --------------------------------------------------------------- numerators


def _split_pow2(q):
    k = (q & -q).bit_length() - 1
    return k, q >> k


def crafted_numerators(q, np_type, lo, hi, n, rng):
    """n numerators d in [lo, hi] (lo < 0 < hi) for the divisor q = 2^k * odd:
    exact ties at p bits with an even and with an odd lower neighbour (d =
    (2m + 1) * odd * 2^j: d / q = (2m + 1) * 2^(j - k) with p + 1 significant
    bits), the integers next to each tie, exactly representable quotients
    (m * odd * 2^j), 0, +-1, both ends of the range, bit lengths 1, bitlen(q)
    and the longest the range holds, f32 edges where the range reaches them,
    and random ones. Returns (numerators, indices of the exact ties)."""
    p, min_unit, top = FORMATS[np_type]
    k, odd = _split_pow2(q)
    ds, ties = [], []

    def put(d, tie=False):
        if lo <= d <= hi and len(ds) < n:
            if tie:
                ties.append(len(ds))
            ds.append(d)
            return True
        return False

    for d in (0, 1, -1, lo, hi, lo + 1, hi - 1):
        put(d)
    room = hi.bit_length() - odd.bit_length() - (p + 1)  # shifts a tie can take
    for i in range(24):
        for parity in (0, 1):
            m = rng.randrange(2 ** (p - 1), 2 ** p) & ~1 | parity
            j = rng.randrange(0, max(room, 0) + 1)
            tie = (2 * m + 1) * odd << j
            for sign in (1, -1):
                if put(sign * tie, tie=True):
                    put(sign * tie - 1)
                    put(sign * tie + 1)
    # the all-ones mantissa: the tie rounds up into the next binade
    put((2 ** (p + 1) - 1) * odd, tie=True)
    for i in range(24):  # exactly representable
        m = rng.randrange(1, 2 ** p)
        j = rng.randrange(0, max(hi.bit_length() - odd.bit_length() - p, 0) + 1)
        put(m * odd << j)
        put(-(m * odd << j))
    for length in (1, q.bit_length(), hi.bit_length() - 1, hi.bit_length()):
        for _ in range(4):
            if length >= 1:
                d = rng.randrange(2 ** (length - 1), 2 ** length)
                put(d)
                put(-d)
    # quotients at powers of two that the format's ends name: q * 2^x and its
    # neighbours, where the range reaches them (f32 under a wide config)
    for x in (-126, -127, -149, -150, -151, 127, 128):
        for mul in (1, 3, 2 ** p - 1, 2 ** (p + 1) - 1):  # ones: carries
            base = Fraction(q * mul) * Fraction(2) ** x
            if base.denominator == 1 and base.numerator >= 2:
                # f32: half the smallest subnormal ties to zero, 3 halves to 2 units
                is_tie = p == 24 and x == -150 and mul in (1, 3)
                for sign in (1, -1):
                    put(sign * base.numerator, tie=is_tie)
                    put(sign * (base.numerator - 1))
                    put(sign * (base.numerator + 1))
    # above the largest finite value
    over = Fraction(top) * q
    if over.denominator == 1:
        half_ulp = q << (103 if p == 24 else 970)  # of the largest finite value, times q
        for d in (over.numerator, over.numerator + 1, over.numerator + half_ulp,
                  2 * over.numerator):
            put(d)
            put(-d)
    while len(ds) < n:
        length = rng.randrange(1, max(hi.bit_length(), 2))
        d = rng.randrange(2 ** (length - 1), 2 ** length)
        put(d if rng.random() < 0.5 else -d)
    return ds, ties


# -------------------------------------------------------------------- rounds


@functools.lru_cache(maxsize=None)
def craft(cfg_args, q, np_type, nb=3, n=N):
    """One crafted round for the config (vector and unit part alike) whose
    exact divisor is q, with np_type output. Computed once per key and shared
    read-only. Keys as unmask_edges.forge, so its tensor helpers apply."""
    cfg = mk.MaskConfig(*cfg_args)
    order = int(cfg.order)
    add, exp = shifts(cfg_args)
    c = nb * add * exp
    assert 2 * c < order and 0 < q and q + c < order, "q is outside what the unit sum can spell"
    rng = random.Random(repr((cfg_args, q, np_type.__name__, nb, n)))
    d, ties = crafted_numerators(q, np_type, -c, min(c, order - c - 1), n, rng)
    assert len(d) == n and len(ties) >= 32, f"{len(ties)} exact ties"
    t = [c + v for v in d]
    assert all(0 <= v < order for v in t)
    quotients = [Fraction(v, q) for v in d]
    p = FORMATS[np_type][0]
    for i in ties:  # a tie: p + 1 significant bits exactly, or half the smallest subnormal
        x = abs(quotients[i])
        assert x.denominator & (x.denominator - 1) == 0
        significant = _split_pow2(x.numerator)[1].bit_length()
        assert significant == p + 1 or x in (Fraction(1, 2 ** 150), Fraction(3, 2 ** 150))

    mask = [rng.randrange(order) for _ in range(n)]
    mask[0], mask[-1] = 0, order - 1
    masked = [(v + m) % order for v, m in zip(t, mask)]
    # the plane forms carry j * order on top, so the in-kernel mod has work
    lifted = [v + (i % nb) * order for i, v in enumerate(masked)]
    n1 = q + c  # exp_shift * (n1 - nb * add_1 * exp_1) / exp_1 == q
    mask_unit = rng.randrange(order)
    return {
        "vect_cfg": cfg, "unit_cfg": cfg, "nb": nb, "n": n, "order": order,
        "add": add, "exp": exp, "q": q, "offset": c, "d": d, "ties": ties,
        "t": t, "n1": n1, "quotients": quotients,
        "mask": mask, "masked": masked, "lifted": lifted,
        "mask_unit": mask_unit, "unit_acc": (n1 + mask_unit) % order,
        "np_type": np_type, "dtype": DTYPE_CODE[np_type],
        "ref": np.array([round_exact(x, np_type) for x in quotients], dtype=np_type),
    }


F32, F64 = np.float32, np.float64

# (config, divisor, output type): L = 1, 2, 2, 3 and 5 limbs. Divisors are
# 2^k and 2^k * odd with room for p + 1-bit ties under nb * add_shift *
# exp_shift, and large enough that the default path's double scalar_sum is
# not zero. F32/Bmax/M3: 10^45 is scalar sum 1; under 2^100 the largest
# numerators pass f32 max; 2^270 and 3 * 2^268 put the quotients on the
# subnormal grid and at half its unit.
CRAFTED = [
    ((1, 0, 4, 3), 2**20, F32),            # Prime/F32/B4/M3, L = 1
    ((1, 0, 4, 3), 3 * 5**5 * 2**9, F32),
    ((1, 1, 0, 3), 2**45, F64),            # Prime/F64/B0/M3, L = 2
    ((1, 1, 0, 3), 3 * 2**40, F64),
    ((1, 1, 4, 9), 2**60, F64),            # Prime/F64/B4/M9, L = 2
    ((1, 1, 4, 9), 5 * 2**58, F64),
    ((1, 1, 4, 9), 2**60, F32),
    ((1, 1, 4, 9), 5**7 * 2**50, F32),
    ((1, 3, 255, 12), 2**40, F32),         # Prime/I64/Bmax/M12, L = 3
    ((1, 3, 255, 12), 10**10, F32),
    ((1, 0, 255, 3), 10**45, F32),         # Prime/F32/Bmax/M3, L = 5
    ((1, 0, 255, 3), 2**100, F32),
    ((1, 0, 255, 3), 2**270, F32),
    ((1, 0, 255, 3), 3 * 2**268, F32),
]
LIMBS = {(1, 0, 4, 3): 1, (1, 1, 0, 3): 2, (1, 1, 4, 9): 2, (1, 3, 255, 12): 3, (1, 0, 255, 3): 5}


def crafted_id(entry):
    cfg, q, np_type = entry
    k, odd = _split_pow2(q)
    return "cfg" + "".join(f"-{a}" for a in cfg) + f"-q2^{k}x{odd}-{np_type.__name__}"


def forged(case):
    """A float case of unmask_edges.FLOAT_CASES as a round with the keys the
    forms helper takes: its reference is already the once-rounded quotient."""
    cfg, scalars = case
    rnd = dict(ue.forge(cfg, cfg, scalars))
    rnd["dtype"] = DTYPE_CODE[rnd["np_type"]]
    c = rnd["nb"] * rnd["add"] * rnd["exp"]
    rnd["q"], rnd["offset"] = rnd["n1"] - c, c  # the same config twice
    # the reference of that module and this one are the same rounding
    again = np.array([round_exact(x, rnd["np_type"]) for x in rnd["quotients"]],
                     dtype=rnd["np_type"])
    assert (bits(again) == bits(rnd["ref"])).all()
    return rnd


def assert_double_steps_miss(rnd, share):
    """The condition that keeps the forged test from passing vacuously: the
    emulated double steps of the default kernels differ from the reference in
    at least `share` of the elements."""
    emu = ue.emulate_kernel_doubles(rnd)
    differ = int((bits(emu) != bits(rnd["ref"])).sum())
    assert differ >= share * rnd["n"], f"only {differ} of {rnd['n']} differ"
    return differ


# --------------------------------------------------------------- entry forms


def unmask_forms(eng, case, exact=True, dtype=None):
    """The round through every unmask entry form of `eng` (either engine),
    like unmask_edges.unmask_forms, with the exact flag: {form: numpy result}.
    dtype defaults to the round's output type."""
    from xaynet_amd.parallel import compact_digits

    dtype = case["dtype"] if dtype is None else dtype
    nb, mu, n = case["nb"], case["mask_unit"], case["n"]
    eng.unit_acc = case["unit_acc"]
    mask = ue.values_tensor(eng, case["mask"])
    planes = ue.planes_tensor(eng, case["lifted"], eng.n_digits, 32)
    eng.acc.copy_(planes)
    outs = {
        "unmask": eng.unmask(mask, mu, nb_models=nb, dtype=dtype, exact=exact),
        "unmask_planes": eng.unmask_planes(planes, mask, mu, nb, dtype, exact=exact),
    }
    shard_bits = 32
    if eng.wide:
        k, shard_bits = compact_digits(case["order"], 2)
        planes = ue.planes_tensor(eng, case["lifted"], k, shard_bits)
        outs["compact_planes"] = eng.unmask_planes(planes, mask, mu, nb, dtype,
                                                   digit_bits=shard_bits, exact=exact)
    else:
        vals = torch.from_numpy(np.array(case["lifted"], dtype=np.uint64).view(np.int64))
        outs["unmask_values"] = eng.unmask_values(vals.to(eng.device), mask, mu, nb, dtype,
                                                  exact=exact)
    parts = [eng.unmask_planes(planes[:, lo:hi].contiguous(), mask[..., lo:hi], mu, nb, dtype,
                               digit_bits=shard_bits, exact=exact)
             for lo, hi in ((0, CUT), (CUT, n))]
    outs["shards"] = torch.cat(parts)
    return {name: out.cpu().numpy() for name, out in outs.items()}


def assert_bits_equal(out, ref, what):
    assert out.dtype == ref.dtype, what
    bad = np.nonzero(bits(out) != bits(ref))[0]
    assert bad.size == 0, (f"{what}: {bad.size} differ, first {bad[:5]}: got {out[bad[:5]]} "
                           f"want {ref[bad[:5]]}")


# ------------------------------------------------- pairs for the element function


def random_pairs(n_limbs, count, seed):
    """(mag, q) of every bit length up to 64 * n_limbs, the full limb width
    included, for _core.mask.unmask_round at `n_limbs` limbs."""
    rng = random.Random(seed)
    top = 64 * n_limbs
    pairs = []
    for i in range(count):
        bm = top if i % 16 == 0 else rng.randrange(1, top + 1)
        bq = top if i % 16 == 1 else rng.randrange(1, top + 1)
        pairs.append((rng.randrange(2 ** (bm - 1), 2 ** bm), rng.randrange(2 ** (bq - 1), 2 ** bq)))
    pairs += [(0, 1), (0, 2 ** top - 1), (1, 1), (2 ** top - 1, 1), (1, 2 ** top - 1),
              (2 ** top - 1, 2 ** top - 1), (2 ** (top - 1), 2 ** (top - 1) + 1)]
    return pairs
