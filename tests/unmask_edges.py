"""Crafted unmask inputs and the exact reference they are checked against.

Shared by tests/test_unmask_edges_cpu.py (CpuPlaneAggregator) and
tests/test_gpu_unmask_edges.py (the K4 kernels). A plain module, no fixtures.

The reference is the unmask of the protocol on fractions.Fraction:

    t_i   = sum_j trunc((clamp(s_j * w_ji, +-add_shift) + add_shift) * exp_shift)
    n1    = sum_j trunc((s_j + add_1) * exp_1)
    out_i = (t_i / exp_shift - nb * add_shift) / (n1 / exp_1 - nb * add_1)

truncated toward zero for integer models, rounded once for float models.

Inputs are built, not searched for. With scalar s_j = num_j / den_j and a weight
w >= 0, participant j's term is floor(w * num_j * E / den_j) - which equals
w * floor(num_j * E / den_j) exactly while w * ((num_j * E) mod den_j) < den_j.
A column that gives every participant such a weight w therefore has the exact
quotient w; with equal scalars 1/k, c participants carrying w and the others 0
have the exact quotient c * w / k wherever k divides c * w. These columns fill
every third element, so the exact-integer quotients (where a double result one
ulp low truncates to the integer below) are at least a quarter of the vector.
"""
import functools
import random
from fractions import Fraction

import numpy as np
import torch

from xaynet_amd import _core

mk = _core.mask

N = 1027   # four full 256-thread workgroups and a tail of 3
CUT = 513  # the two column shards: [0, 513) and [513, 1027)

# exp_shift per mask::DataType and add_shift per bound (B0, B2, B4, B6), kept
# apart from the engine's own table; test_reference_is_the_oracle pins them
EXP_SHIFT = {0: 10**10, 1: 10**20, 2: 10**10, 3: 10**10}
ADD_SHIFT = {0: 1, 2: 100, 4: 10**4, 6: 10**6}
NP_DTYPES = {0: np.float32, 1: np.float64, 2: np.int32, 3: np.int64}

# Equal weights w for k participants of scalar 1/k and exp_shift 10^10 whose
# quotient is exactly w and which were suspected of coming out as w - 1 from
# the double steps: (bound, k) -> weights. The double kernels did return w - 1
# for B4/k=3/w=2 and B6/k=11/w=10 (and 20, 31 for the inexact 21, 32 there);
# the others came out right on the GPU, as they do in a numpy emulation.
EXACT_EQUAL_WEIGHTS = {
    (4, 3): (2,),
    (4, 6): (1,),
    (2, 9): (1, 3, 6, 8),
    (2, 11): (1, 2, 6, 7),
    (4, 9): (1, 2, 3, 8),
    (6, 11): (10,),
}


def shifts(cfg_args):
    """(add_shift, exp_shift) of a (group, dtype, bound, model) config."""
    _, dtype, bound, _ = cfg_args
    return ADD_SHIFT[bound], EXP_SHIFT[dtype]


# ------------------------------------------------------------------ reference


def shifted(value: Fraction, add: int, exp: int) -> int:
    """trunc((clamp(value, +-add) + add) * exp), the masked-domain integer."""
    value = max(-add, min(add, value))
    return int((value + add) * exp)  # int() of a Fraction truncates toward zero


def reference_sums(columns, scalars, add, exp):
    """t_i for every column of per-participant weights."""
    return [sum(shifted(s * Fraction(w), add, exp) for s, w in zip(scalars, col))
            for col in columns]


def reference_quotients(t, n1, nb, add, exp, add1, exp1):
    divisor = Fraction(n1, exp1) - nb * add1
    return [(Fraction(v, exp) - nb * add) / divisor for v in t]


def round_once(q: Fraction, np_type):
    """q rounded to the nearest np_type value (ties to even), one rounding."""
    if np_type is np.float64:
        return np.float64(q.numerator / q.denominator)  # int / int rounds once
    x = np.float32(q.numerator / q.denominator)
    cands = {x, np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))}
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - q),
                                     int(np.float32(c).view(np.uint32)) & 1))


# -------------------------------------------------------------------- columns


def _exact_columns(scalars, add, exp):
    """Columns with an exact integer quotient by construction (module
    docstring): all participants carry a remainder-free w, or - equal scalars
    only - c of them do and k divides c * w."""
    k = len(scalars)
    free = [w for w in range(0, min(add, 16) + 1)
            if all(w * ((s.numerator * exp) % s.denominator) < s.denominator for s in scalars)]
    cols = [(w,) * k for w in free]
    if len(set(scalars)) == 1:
        for c in range(1, k):
            for w in free:
                if w and (c * w) % k == 0:
                    cols.append((w,) * c + (0,) * (k - c))
                    cols.append((0,) * (k - c) + (w,) * c)
    return cols


def _edge_columns(k, add, rng):
    """The named edges: every weight of EXACT_EQUAL_WEIGHTS (0..12), the
    clamp bound itself, weights +-1 around the multiples of k up to 3k (as one
    participant's weight, as every participant's, and as the column sum), and
    columns that clamp."""
    cols = []
    for w in range(0, 13):
        cols += [(w,) * k, (-w,) * k]
    cols += [(add,) * k, (-add,) * k, (add,) + (0,) * (k - 1), (-add,) + (add,) * (k - 1)]
    for m in (1, 2, 3):
        for delta in (-1, 0, 1):
            w = m * k + delta
            for sign in (1, -1):
                cols.append((sign * w,) * k)                      # every participant
                cols.append((sign * w,) + (0,) * (k - 1))         # one participant
                cols.append((0,) * (k - 1) + (sign * w,))
                cols.append((sign * (m + delta),) + (sign * m,) * (k - 1))  # the column sum
    over = k * add + 1  # |w / k| > add_shift for every scalar >= 1/k
    cols += [(over,) * k, (-over,) * k,
             (over,) + tuple(rng.randint(-add, add) for _ in range(k - 1)),
             (-over,) + tuple(rng.randint(-add, add) for _ in range(k - 1))]
    return cols


def integer_columns(scalars, add, exp, n, rng):
    k = len(scalars)
    exact = _exact_columns(scalars, add, exp)
    edges = _edge_columns(k, add, rng)
    cols = []
    for i in range(n):
        if i % 3 == 0:
            cols.append(exact[(i // 3) % len(exact)])
        elif edges:
            cols.append(edges.pop(0))
        else:
            cols.append(tuple(rng.randint(-add, add) for _ in range(k)))
    return cols


def float_columns(k, add, n, rng, np_type):
    """Weights +-add_shift, 0, +-1e-9 and random, as values of the model's
    float type."""
    special = [float(add), -float(add), 0.0, 1e-9, -1e-9]
    cols = [(v,) * k for v in special] + [(v,) + (0.0,) * (k - 1) for v in special]
    while len(cols) < n:
        cols.append(tuple(rng.choice(special) if rng.random() < 0.25
                          else rng.uniform(-add, add) for _ in range(k)))
    return [tuple(float(np_type(w)) for w in col) for col in cols]


# ---------------------------------------------------------------------- cases


@functools.lru_cache(maxsize=None)
def forge(vect_args, unit_args, scalars, n=N):
    """One crafted round: `scalars` is a tuple of (num, den), one participant
    each. Computed once per key and shared read-only by the tests."""
    vect_cfg, unit_cfg = mk.MaskConfig(*vect_args), mk.MaskConfig(*unit_args)
    order, unit_order = int(vect_cfg.order), int(unit_cfg.order)
    add, exp = shifts(vect_args)
    add1, exp1 = shifts(unit_args)
    fr = tuple(Fraction(a, b) for a, b in scalars)
    nb = len(fr)
    rng = random.Random(repr((vect_args, unit_args, scalars, n)))
    is_float = vect_args[1] in (0, 1)
    np_type = NP_DTYPES[vect_args[1]]
    if is_float:
        columns = float_columns(nb, add, n, rng, np_type)
    else:
        columns = integer_columns(fr, add, exp, n, rng)

    t = reference_sums(columns, fr, add, exp)
    n1 = sum(shifted(s, add1, exp1) for s in fr)
    quotients = reference_quotients(t, n1, nb, add, exp, add1, exp1)

    mask = [rng.randrange(order) for _ in range(n)]
    mask[0], mask[-1] = 0, order - 1
    masked = [(v + m) % order for v, m in zip(t, mask)]
    # the plane forms carry j * order on top, so the in-kernel mod has work
    lifted = [v + (i % nb) * order for i, v in enumerate(masked)]
    mask_unit = rng.randrange(unit_order)
    return {
        "vect_cfg": vect_cfg, "unit_cfg": unit_cfg, "nb": nb, "n": n, "order": order,
        "add": add, "exp": exp, "add1": add1, "exp1": exp1, "scalars": fr,
        "columns": columns, "t": t, "n1": n1, "quotients": quotients,
        "mask": mask, "masked": masked, "lifted": lifted,
        "mask_unit": mask_unit, "unit_acc": (n1 + mask_unit) % unit_order,
        "np_type": np_type,
        "exact": np.array([q.denominator == 1 for q in quotients]),
        "ref": (np.array([round_once(q, np_type) for q in quotients], dtype=np_type) if is_float
                else np.array([int(q) for q in quotients], dtype=np.int64).astype(np_type)),
    }


def equal_scalars(k):
    return ((1, k),) * k


# ------------------------------------------------------------ float outputs


def float_bound(case):
    """|out - ref| <= spacing_out(ref) + 2u((7A + 3 A1 |ref|)/S + |ref|) with
    u = 2^-53, A = nb * add_shift, A1 = nb * add_1 and S the exact scalar sum:
    y takes three roundings at magnitude <= 2A, y - A one, scalar_sum two at
    magnitude <= 2 A1, the quotient one; the factor 2 covers second order."""
    u = 2.0 ** -53
    nb = case["nb"]
    a, a1 = nb * case["add"], nb * case["add1"]
    s = float(Fraction(case["n1"], case["exp1"]) - a1)
    ref = np.array([float(abs(q)) for q in case["quotients"]])
    return np.spacing(np.abs(case["ref"])).astype(np.float64) + \
        2 * u * ((7 * a + 3 * a1 * ref) / s + ref)


def emulate_kernel_doubles(case):
    """The K4 double steps in numpy float64, cast to the model's type."""
    exp = case["exp"]
    q = np.array([float(v // exp) for v in case["t"]])
    r = np.array([float(v % exp) for v in case["t"]])
    y = q + r / np.float64(exp)
    scalar_sum = case["n1"] / float(case["exp1"]) - case["nb"] * float(case["add1"])
    out = (y - np.float64(case["nb"] * case["add"])) / np.float64(scalar_sum)
    return out.astype(case["np_type"])


# --------------------------------------------------------------- entry forms


def values_tensor(eng, ints):
    """Python ints -> the engine's canonical value tensor ([n] or [2, n])."""
    rows = [np.array([(v >> (64 * j)) & (2**64 - 1) for v in ints], dtype=np.uint64)
            for j in range(eng.n_limbs if eng.wide else 1)]
    arr = np.stack(rows) if eng.wide else rows[0]
    return torch.from_numpy(arr.view(np.int64)).to(eng.device)


def planes_tensor(eng, ints, k, digit_bits):
    """[k, n] planes of digit_bits-wide digits; the top plane takes whatever
    is left (plane entries are sums, they may exceed 2^digit_bits)."""
    low = (1 << digit_bits) - 1
    rows = [[(v >> (digit_bits * d)) & low for v in ints] for d in range(k - 1)]
    rows.append([v >> (digit_bits * (k - 1)) for v in ints])
    assert max(rows[-1]) < 2**63
    return torch.tensor(rows, dtype=torch.int64).to(eng.device)


def unmask_forms(eng, case, dtype=None):
    """The crafted round through every unmask entry form of `eng` (either
    engine): {form: numpy result}."""
    from xaynet_amd.parallel import compact_digits

    nb, mu, n = case["nb"], case["mask_unit"], case["n"]
    eng.unit_acc = case["unit_acc"]
    mask = values_tensor(eng, case["mask"])
    planes = planes_tensor(eng, case["lifted"], eng.n_digits, 32)
    eng.acc.copy_(planes)
    outs = {
        "unmask": eng.unmask(mask, mu, nb_models=nb, dtype=dtype),
        "unmask_planes": eng.unmask_planes(planes, mask, mu, nb, dtype),
    }
    shard_bits = 32
    if eng.wide:
        k, shard_bits = compact_digits(case["order"], 2)
        planes = planes_tensor(eng, case["lifted"], k, shard_bits)
        outs["compact_planes"] = eng.unmask_planes(planes, mask, mu, nb, dtype,
                                                   digit_bits=shard_bits)
    else:
        vals = torch.from_numpy(np.array(case["lifted"], dtype=np.uint64).view(np.int64))
        outs["unmask_values"] = eng.unmask_values(vals.to(eng.device), mask, mu, nb, dtype)
    parts = [eng.unmask_planes(planes[:, lo:hi].contiguous(), mask[..., lo:hi], mu, nb, dtype,
                               digit_bits=shard_bits)
             for lo, hi in ((0, CUT), (CUT, n))]
    outs["shards"] = torch.cat(parts)
    return {name: out.cpu().numpy() for name, out in outs.items()}


# ------------------------------------------------------------------- matrices

# (vect config, ids): B0, B2, B4 at M3 are u64 orders, B6/M3 is bpn 9 (lo/hi);
# an Integer, a Prime and a Power2 group; i32 and i64
INTEGER_CONFIGS = [
    (0, 2, 0, 3),  # Integer/I32/B0/M3
    (1, 3, 2, 3),  # Prime/I64/B2/M3
    (2, 2, 4, 3),  # Power2/I32/B4/M3
    (1, 3, 6, 3),  # Prime/I64/B6/M3, wide
]
PARTICIPANTS = [3, 6, 9, 11, 4]  # 4: the control, scalar_sum is exactly 1.0
INTEGER_CASES = [(cfg, equal_scalars(k)) for cfg in INTEGER_CONFIGS for k in PARTICIPANTS]
INTEGER_CASES += [((2, 2, 4, 3), ((1, 3), (1, 5), (1, 7))),
                  ((1, 3, 6, 3), ((1, 3), (1, 5), (1, 7)))]

# an I32 vector config with an F64 unit config: exp_shift differs, the
# divisor exp_shift * scalar_sum is no integer
NO_DIVISOR_CASE = ((1, 2, 2, 3), (1, 1, 2, 3), equal_scalars(3))

FLOAT_CASES = [
    ((1, 0, 4, 3), equal_scalars(3)),   # Prime/F32/B4/M3: a u64 order
    ((1, 1, 4, 9), equal_scalars(3)),   # Prime/F64/B4/M9: wide, exp_shift 10^20
]


def case_id(case):
    cfg, scalars = case
    dens = "_".join(str(d) for _, d in scalars) if len(set(scalars)) > 1 else f"k{len(scalars)}"
    return "cfg" + "".join(f"-{a}" for a in cfg) + "-" + dens
