"""Digit planes at full headroom, and the exact reference they are checked against.

Shared by tests/test_plane_headroom_cpu.py (the host instantiation of the
finalize arithmetic, _core.mask.planes_mod, and CpuPlaneAggregator) and
tests/test_gpu_plane_headroom.py (the K2 / K4 kernels). A plain module, no
fixtures. The reference is Python integers only:

    value_i = sum_d planes[d][i] << (digit_bits * d)   mod order

The planes of a round hold sums of at most a few updates, entries below 2^36,
where the recombination never carries between limbs. `respell` writes the same
residues with plane entries as large as the layout allows:

  * 32-bit planes, TOP_DOC = (2^31 - 1)(2^32 - 1): entries up to
    2^31 * (2^32 - 1), what 2^31 updates of 32-bit digits sum to;
  * 32-bit planes, TOP_MAX = 2^64 - 2^32: entries up to 2^64 - 1, all a plane
    entry can hold (the launchers' own contract);
  * compact planes of w-bit digits, TOP_I64(w) = 2^63 - 2^w: entries below
    2^63, the bound of the int64 collective that sums them.

Every case starts with the ripple columns (`ripple_columns`): elements whose
planes spell an exact power of two through a carry that runs up every limb.
Their masks are chosen so that they, too, are elements of the round.
"""
import functools
import random

import numpy as np
import pytest
import torch

import unmask_edges as ue
from unmask_edges import mk

N_ROUND = 259  # one 256-thread workgroup and a tail of 3, after the ripple columns
CUT = 130      # the two column shards: [0, 130) and [130, n)
K = 3          # participants of a round, scalar 1/3 each

TOP_DOC = (2**31 - 1) * (2**32 - 1)
TOP_MAX = 2**64 - 2**32
TOPS32 = {"doc": TOP_DOC, "max": TOP_MAX}


def top_i64(w):
    return 2**63 - 2**w


# (group, dtype, bound, model): order bits / 32-bit planes / limbs
CONFIGS = [
    (0, 2, 0, 3),     # Integer/I32/B0/M3    45 / 2 / 1
    (1, 0, 4, 3),     # Prime/F32/B4/M3      58 / 2 / 1
    (1, 3, 6, 3),     # Prime/I64/B6/M3      65 / 3 / 2
    (1, 1, 4, 9),     # Prime/F64/B4/M9     111 / 4 / 2
    (1, 1, 6, 12),    # Prime/F64/B6/M12    128 / 4 / 2
    (1, 2, 255, 3),   # Prime/I32/Bmax/M3    76 / 3 / 2
    (2, 3, 255, 9),   # Pow2/I64/Bmax/M9    2^128 itself / 4 / 3
    (1, 3, 255, 12),  # Prime/I64/Bmax/M12  138 / 5 / 3
    (1, 0, 255, 3),   # Prime/F32/Bmax/M3   289 / 10 / 5
    (2, 0, 255, 12),  # Pow2/F32/Bmax/M12   320 / 10 / 5
]
# what the comments above claim, asserted by test_config_table
CONFIG_SHAPES = {
    (0, 2, 0, 3): (45, 2, 1), (1, 0, 4, 3): (58, 2, 1), (1, 3, 6, 3): (65, 3, 2),
    (1, 1, 4, 9): (111, 4, 2), (1, 1, 6, 12): (128, 4, 2), (1, 2, 255, 3): (76, 3, 2),
    (2, 3, 255, 9): (129, 4, 3), (1, 3, 255, 12): (138, 5, 3), (1, 0, 255, 3): (289, 10, 5),
    (2, 0, 255, 12): (320, 10, 5),
}


def cfg_id(cfg):
    return "cfg" + "".join(f"-{a}" for a in cfg)


def shape_of(cfg_args):
    """(order, 32-bit planes, limbs) of a config."""
    cfg = mk.MaskConfig(*cfg_args)
    order = int(cfg.order)
    return order, (cfg.bytes_per_number + 3) // 4, (order.bit_length() + 63) // 64


def forms(cfg_args):
    """The plane forms of a config as (k, digit_bits, top name): the 32-bit
    accumulator planes at both tops and, for wide orders, the compact planes
    of a 2- and an 8-rank world."""
    from xaynet_amd.parallel import compact_digits

    order, n_digits, n_limbs = shape_of(cfg_args)
    out = [(n_digits, 32, "doc"), (n_digits, 32, "max")]
    if n_limbs > 1:
        out += [(k, w, "i64") for k, w in sorted({compact_digits(order, 2),
                                                  compact_digits(order, 8)})]
    return out


def top_of(w, top_name):
    return top_i64(w) if top_name == "i64" else TOPS32[top_name]


CASES = [(cfg, form) for cfg in CONFIGS for form in forms(cfg)]


def case_id(case):
    cfg, (k, w, top_name) = case
    return f"{cfg_id(cfg)}-{k}x{w}-{top_name}"


# ------------------------------------------------------------------ reference


def spelled(planes, digit_bits):
    """[k][n] plane entries -> the integers they spell (not reduced)."""
    return [sum(int(p[i]) << (digit_bits * d) for d, p in enumerate(planes))
            for i in range(len(planes[0]))]


def digits_of(value, k, digit_bits):
    """k digits of digit_bits bits; the top one takes whatever is left."""
    low = (1 << digit_bits) - 1
    return [(value >> (digit_bits * d)) & low for d in range(k - 1)] + \
        [value >> (digit_bits * (k - 1))]


def window_bits(n_limbs):
    return 64 * (n_limbs + 1) - 1


def window_ok(k, digit_bits, n_limbs):
    """The rule of the launchers, kept apart from the engines' own copy."""
    return (k - 1) * digit_bits + 64 <= window_bits(n_limbs)


# -------------------------------------------------------------------- columns


def respell(ints, order, k, digit_bits, top, rng):
    """[k][n] plane entries that spell a value congruent to ints[i] mod order
    with entries up to `top` (+ a digit): noise q_d from {0, top, uniform},
    then the digits of r = (ints[i] - sum q_d << (digit_bits d)) mod order on
    top of the noise."""
    planes = [[0] * len(ints) for _ in range(k)]
    for i, want in enumerate(ints):
        noise = [rng.choice((0, top, rng.randint(0, top))) for _ in range(k)]
        if i % 7 == 0:
            noise = [top] * k  # every plane full
        v = sum(q << (digit_bits * d) for d, q in enumerate(noise))
        for d, digit in enumerate(digits_of((want - v) % order, k, digit_bits)):
            planes[d][i] = noise[d] + digit
    return planes


def ripple_columns(k, digit_bits, top, n_limbs):
    """Columns (k entries each) and what they spell. For m = 1 .. k-1: plane 0
    = 2^w and planes 1..m = 2^w - 1, the rest 0, spell exactly 2^(w(m+1)): the
    carry of the last addition runs through every bit above w. For w = 32 and
    m = 2j - 1 that is 2^(64j), a carry out of limb 0 through limbs 1..j-1
    into limb j. Then each of them with `top` in the planes above m, a column
    of zeros, and one of all planes equal to `top`. With entries up to 2^64 -
    1 (TOP_MAX) also [2^32, 2^64 - 1, 2^64 - 2^32, ...], which spell
    2^(32(m+2)) from m + 1 planes: the limb-1-is-all-ones ripple into limb 2
    with three planes only."""
    w = digit_bits
    cols = []
    for m in range(1, k):
        base = [2**w] + [2**w - 1] * m + [0] * (k - 1 - m)
        cols.append((base, 2**(w * (m + 1))))
        noisy = base[:m + 1] + [top] * (k - 1 - m)
        cols.append((noisy, 2**(w * (m + 1)) + sum(top << (w * d) for d in range(m + 1, k))))
    cols.append(([0] * k, 0))
    cols.append(([top] * k, sum(top << (w * d) for d in range(k))))
    if top == TOP_MAX:
        for m in range(2, k):
            if 32 * (m + 2) < window_bits(n_limbs):
                col = [2**32, 2**64 - 1] + [2**64 - 2**32] * (m - 1) + [0] * (k - 1 - m)
                cols.append((col, 2**(32 * (m + 2))))
    for col, value in cols:
        assert sum(p << (w * d) for d, p in enumerate(col)) == value
        assert max(col) < 2**64 and value < 2**window_bits(n_limbs)
    return cols


# --------------------------------------------------------------------- rounds


def _bmax_weights(cfg, length, rng):
    if cfg.dtype == 2:
        return rng.integers(-2**31, 2**31, length).astype(np.int32)
    if cfg.dtype == 3:
        return rng.integers(-2**50, 2**50 + 1, length).astype(np.int64)
    # magnitudes 1e-3 .. 1e30, both signs, the same decade in every update
    decade = 10.0 ** np.random.default_rng(length).uniform(-3, 30, length)
    return (rng.choice([-1.0, 1.0], length) * rng.uniform(0.5, 1.0, length) * decade).astype(
        np.float32)


@functools.lru_cache(maxsize=None)
def _bmax_round(cfg_args, n):
    """K CPU-masked updates of scalar 1/K and the oracle's unmask of them."""
    cfg = mk.MaskConfig(*cfg_args)
    pair = mk.MaskConfigPair(cfg, cfg)
    order, bpn = int(cfg.order), cfg.bytes_per_number
    rng = np.random.default_rng(12)
    agg, mask_agg = mk.Aggregation(pair, n), mk.Aggregation(pair, n)
    unit_acc = 0
    for _ in range(K):
        seed = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        masked = mk.mask_model(seed, mk.Scalar(1, K), _bmax_weights(cfg, n, rng), pair)
        agg.aggregate(masked)
        mask_agg.aggregate(mk.derive_mask(seed, n, pair))
        unit_acc = (unit_acc + int(masked.unit_value)) % order
    masked = [int(agg.object.element(i)) for i in range(n)]
    mask = [int(mask_agg.object.element(i)) for i in range(n)]
    return {
        "t": [(a - b) % order for a, b in zip(masked, mask)],
        "mask_unit": int(mask_agg.object.unit_value), "unit_acc": unit_acc,
        "ref": np.asarray(agg.unmask(mask_agg.object)), "forged": None,
    }


@functools.lru_cache(maxsize=None)
def _round(cfg_args, n):
    """t = (masked - mask) mod order of n elements with the scalars and the
    reference model: unmask_edges.forge for B0..B6, the oracle for Bmax."""
    if cfg_args[2] == 255:
        return _bmax_round(cfg_args, n)
    rnd = ue.forge(cfg_args, cfg_args, ue.equal_scalars(K), n=n)
    return {"t": rnd["t"], "mask_unit": rnd["mask_unit"], "unit_acc": rnd["unit_acc"],
            "ref": rnd["ref"], "forged": rnd}


@functools.lru_cache(maxsize=None)
def case(cfg_args, form):
    """One round in one plane form at full headroom. Computed once per key and
    shared read-only by the tests.

    planes  [k][n] Python ints below 2^64, n = ripple columns + N_ROUND
    plain   the same residues in small entries (digits of `masked`)
    masked  what the planes spell, mod order; mask, mask_unit, unit_acc, nb
    ref     the model (unmask_edges reference or the oracle)"""
    k, w, top_name = form
    order, n_digits, n_limbs = shape_of(cfg_args)
    top = top_of(w, top_name)
    assert window_ok(k, w, n_limbs)
    ripple = ripple_columns(k, w, top, n_limbs)
    n = len(ripple) + N_ROUND
    rnd = _round(cfg_args, n)
    rng = random.Random(repr((cfg_args, form)))
    mask = [rng.randrange(order) for _ in range(n)]
    mask[len(ripple)], mask[-1] = 0, order - 1
    for i, (_, value) in enumerate(ripple):  # the ripple columns are elements of the round
        mask[i] = (value - rnd["t"][i]) % order
    masked = [(t + m) % order for t, m in zip(rnd["t"], mask)]
    planes = respell(masked, order, k, w, top, rng)
    for i, (col, _) in enumerate(ripple):
        for d in range(k):
            planes[d][i] = col[d]
    return {
        "cfg_args": cfg_args, "cfg": mk.MaskConfig(*cfg_args), "form": form, "order": order,
        "n_limbs": n_limbs, "n_digits": n_digits, "k": k, "digit_bits": w, "top": top, "n": n,
        "n_ripple": len(ripple), "planes": planes, "plain": [list(r) for r in zip(
            *(digits_of(v, k, w) for v in masked))],
        "masked": masked, "mask": mask, "mask_unit": rnd["mask_unit"],
        "unit_acc": rnd["unit_acc"], "nb": K, "ref": rnd["ref"], "forged": rnd["forged"],
        "is_float": cfg_args[1] in (0, 1),
    }


# -------------------------------------------------------- top of the window

# Plane forms whose shape meets the window rule with equality, (k - 1) w + 64
# = 64 (L + 1) - 1, per limb count: only these can spell every integer below
# the 2^(64(L+1) - 1) that the reduction takes (the top plane holds the 64 bits
# that are left). No caller uses them; the launchers accept them, and only
# values in the top half of the window make the divisor of the shift-subtract
# loop grow to its last step. 127, 191 are prime: one-bit digits.
EDGE_FORMS = {1: (2, 63), 2: (128, 1), 3: (192, 1), 5: (12, 29)}


@functools.lru_cache(maxsize=None)
def edge_case(cfg_args):
    """Values in [2^(W-1), 2^W), W the window's bits: 2^W - 1, 2^(W-1) and its
    predecessor, the order shifted up to W bits (and one less), 130 values
    above that multiple and 130 anywhere in the top half."""
    order, _, n_limbs = shape_of(cfg_args)
    k, w = EDGE_FORMS[n_limbs]
    bits = window_bits(n_limbs)
    assert (k - 1) * w + 64 == bits and window_ok(k, w, n_limbs)
    rng = random.Random(repr(("edge", cfg_args)))
    lifted = order << (bits - order.bit_length())
    values = [2**bits - 1, 2**(bits - 1), 2**(bits - 1) - 1, lifted, lifted - 1]
    values += [lifted + rng.randrange(min(order, 2**bits - lifted)) for _ in range(130)]
    values += [rng.randrange(2**(bits - 1), 2**bits) for _ in range(130)]
    planes = [list(r) for r in zip(*(digits_of(v, k, w) for v in values))]
    assert max(max(row) for row in planes) < 2**64 and spelled(planes, w) == values
    return {"cfg": mk.MaskConfig(*cfg_args), "order": order, "n_limbs": n_limbs, "k": k,
            "digit_bits": w, "n": len(values), "values": values, "planes": planes,
            "lifted": lifted, "want": [v % order for v in values]}


# ---------------------------------------------------------- tensors and checks


def planes_array(planes):
    """[k][n] Python ints below 2^64 -> uint64 array."""
    return np.array(planes, dtype=np.uint64)


def planes_tensor(eng, planes):
    """-> the engine's int64 plane tensor (entries above 2^63 wrap, as the
    kernels read them back)."""
    return torch.from_numpy(planes_array(planes).view(np.int64)).to(eng.device)


def values_tensor(eng, ints):
    return ue.values_tensor(eng, ints)


def values_ints(eng, t):
    """The engine's canonical value tensor -> Python ints."""
    rows = t.cpu().numpy().view(np.uint64).reshape(-1, t.shape[-1])
    return [sum(int(rows[j][i]) << (64 * j) for j in range(rows.shape[0]))
            for i in range(rows.shape[1])]


def plane_ints(t):
    """A plane tensor -> [k][n] Python ints (unsigned)."""
    return [[int(x) for x in row] for row in t.cpu().numpy().view(np.uint64)]


def first_diff(got, want):
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    return f"{len(bad)} wrong, first at {bad[:5]}" if bad or len(got) != len(want) else ""


def engine_for(cls, c):
    eng = cls(c["cfg"], c["cfg"], c["n"])
    eng.unit_acc = c["unit_acc"]
    return eng


def assert_model(c, out, what):
    """Integer models are the reference exactly. Float models keep the bound
    the existing tests hold them to: unmask_edges.float_bound for B0..B6, one
    spacing of the oracle's value for Bmax."""
    ref = c["ref"]
    assert out.dtype == ref.dtype and out.shape == ref.shape, what
    if not c["is_float"]:
        bad = np.nonzero(out != ref)[0]
        assert bad.size == 0, f"{what}: {bad.size} wrong, first {bad[:5]}"
        return
    assert np.isfinite(out).all(), what
    err = np.abs(out.astype(np.float64) - ref.astype(np.float64))
    if c["forged"] is not None:
        bound = ue.float_bound(c["forged"])
    else:
        bound = np.spacing(np.abs(ref)).astype(np.float64)
    assert (err <= bound).all(), f"{what}: {np.max(err / bound):.3f} of the bound"


def lifted_values(c):
    """masked + m * order with the largest m that stays below 2^64 (u64
    orders: the input of unmask_values)."""
    return [v + ((2**64 - 1 - v) // c["order"]) * c["order"] for v in c["masked"]]


def unmask_forms(eng, c, planes):
    """The round through every unmask entry form of `eng` (either engine) on
    the given plane tensor: {form: numpy model}."""
    nb, mu, n, w = c["nb"], c["mask_unit"], c["n"], c["digit_bits"]
    mask = values_tensor(eng, c["mask"])
    outs = {"unmask_planes": eng.unmask_planes(planes, mask, mu, nb, digit_bits=w)}
    if w == 32:
        eng.acc.copy_(planes)
        outs["unmask"] = eng.unmask(mask, mu, nb_models=nb)
    parts = [eng.unmask_planes(planes[:, lo:hi].contiguous(), mask[..., lo:hi], mu, nb,
                               digit_bits=w) for lo, hi in ((0, CUT), (CUT, n))]
    outs["shards"] = torch.cat(parts)
    return {name: out.cpu().numpy() for name, out in outs.items()}


# --------------------------------------------------------------- window check


def raises_unchanged(call, out):
    """call() raises ValueError and has not written to `out`."""
    before = out.clone()
    with pytest.raises(ValueError):
        call()
    assert torch.equal(out, before)


def check_window(eng):
    """Both engines: plane shapes that could spell 2^191 or more are refused
    by every reader, with the output untouched; the shapes in use pass."""
    from xaynet_amd.parallel import compact_digits

    n = eng.length
    dev = eng.device
    assert eng.order_int.bit_length() == 128 and eng.n_limbs == 2
    mask = eng.new_values(zero=True)
    out = eng.new_values().fill_(7)
    for k, w in ((5, 32), (4, 63), (129, 1)):
        assert not eng.plane_window_ok(k, w)
        planes = torch.full((k, n), 1, dtype=torch.int64, device=dev)
        raises_unchanged(lambda: eng.planes_to_values(planes, out, digit_bits=w), out)
        raises_unchanged(lambda: eng.unmask_planes(planes, mask, 0, 1, digit_bits=w), planes)
    shapes = {(4, 32), (3, 63), (128, 1)} | {compact_digits(eng.order_int, world)
                                              for world in range(1, 9)}
    for k, w in sorted(shapes):
        assert eng.plane_window_ok(k, w)
        planes = torch.full((k, n), 1, dtype=torch.int64, device=dev)
        eng.planes_to_values(planes, out, digit_bits=w)
        want = sum(1 << (w * d) for d in range(k)) % eng.order_int
        assert values_ints(eng, out) == [want] * n, (k, w)
