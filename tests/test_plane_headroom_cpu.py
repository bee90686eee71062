"""The finalize arithmetic at full digit-plane headroom, on the host.

_core.mask.planes_mod runs the kernels' own recombination and reduction
(gpu/limbs.h, gpu/u192.h) compiled for the host; CpuPlaneAggregator gives the
round's reference through every entry form. Both against Python integers on
the inputs of tests/plane_headroom.py - the CPU twin of
tests/test_gpu_plane_headroom.py, which pins inputs and reference before a GPU
sees them. Also here: the window check of both engines' plane readers (CPU
side) and the 2^31-update bound of an accumulator."""
import numpy as np
import pytest
import torch

import plane_headroom as ph
from plane_headroom import mk

from xaynet_amd.ops.base import MAX_UPDATES_PER_ACCUMULATOR
from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator
from xaynet_amd.parallel import compact_digits


@pytest.mark.parametrize("cfg", ph.CONFIGS, ids=ph.cfg_id)
def test_config_table(cfg):
    """The configs are the shapes the module says they are, and every form
    lies inside its window."""
    order, n_digits, n_limbs = ph.shape_of(cfg)
    assert (order.bit_length(), n_digits, n_limbs) == ph.CONFIG_SHAPES[cfg]
    eng = CpuPlaneAggregator(mk.MaskConfig(*cfg), mk.MaskConfig(*cfg), 1)
    assert (eng.n_digits, eng.n_limbs) == (n_digits, n_limbs)
    for k, w, _ in ph.forms(cfg):
        assert ph.window_ok(k, w, n_limbs) and eng.plane_window_ok(k, w)
        assert k * w >= order.bit_length() or order == 1 << (k * w)


def test_all_widths_present():
    assert {ph.shape_of(cfg)[2] for cfg in ph.CONFIGS} == {1, 2, 3, 5}


@pytest.mark.parametrize("case", ph.CASES, ids=ph.case_id)
def test_inputs_reach_the_headroom(case):
    """The condition on the inputs, on the reference alone: the planes spell
    the round's residues, the entries reach the top, the totals reach into
    the window's last limb, and the ripple columns are exact powers of two."""
    c = ph.case(*case)
    k, w, top_name = c["form"]
    values = ph.spelled(c["planes"], w)
    assert [v % c["order"] for v in values] == c["masked"]
    assert [v % c["order"] for v in ph.spelled(c["plain"], w)] == c["masked"]
    biggest = max(max(row) for row in c["planes"])
    assert c["top"] <= biggest < (2**63 if top_name == "i64" else 2**64)
    assert max(values) < 2**ph.window_bits(c["n_limbs"])
    assert max(values).bit_length() >= c["top"].bit_length() + w * (k - 1)
    # steps of the grow-and-subtract loops: 30 and more on the accumulator
    # planes; compact digits leave 63 - w bits to the int64 collective
    steps = max(values).bit_length() - c["order"].bit_length()
    assert steps >= (30 if w == 32 else 63 - w)
    for m in range(1, k):
        assert values[2 * (m - 1)] == 2**(w * (m + 1))
    print(f"{ph.case_id(case)}: largest entry {biggest.bit_length()} bits, "
          f"largest total {max(values).bit_length()} bits, order "
          f"{c['order'].bit_length()} bits")


def _paths(c):
    paths = [("ml", False)]
    if c["n_limbs"] == 2:
        paths += [("u192", False)] + ([("u192", True)] if c["digit_bits"] == 32 else [])
    return paths


@pytest.mark.parametrize("case", ph.CASES, ids=ph.case_id)
def test_planes_mod_is_the_python_sum(case):
    """ml_mod<L>(ml_from_planes<L+1>) and, for two-limb orders,
    u192_mod_u128(u192_from_planes<32 | 0>) on every element."""
    c = ph.case(*case)
    w = c["digit_bits"]
    arr = ph.planes_array(c["planes"])
    for path, runtime in _paths(c):
        got = mk.planes_mod(arr, c["order"], w, path, runtime_shift=runtime)
        for i in range(c["n_ripple"]):  # one by one
            assert got[i] == c["masked"][i], (
                f"{path} runtime={runtime}: ripple column {i} "
                f"{[hex(p[i]) for p in c['planes']]}: got {got[i]:#x} want {c['masked'][i]:#x}")
        assert got == c["masked"], f"{path} runtime={runtime}: {ph.first_diff(got, c['masked'])}"
        plain = mk.planes_mod(ph.planes_array(c["plain"]), c["order"], w, path,
                              runtime_shift=runtime)
        assert plain == c["masked"], f"{path} plain: {ph.first_diff(plain, c['masked'])}"


@pytest.mark.parametrize("cfg", ph.CONFIGS, ids=ph.cfg_id)
def test_top_of_the_window(cfg):
    """Values in the top half of the reduction window, where the divisor of
    the shift-subtract loop has to grow to its last step: ml_mod at every
    width, u192_mod_u128 for the two-limb orders, and the CPU plane."""
    c = ph.edge_case(cfg)
    assert min(c["values"]).bit_length() == ph.window_bits(c["n_limbs"]) - 1
    assert max(c["values"]) == 2**ph.window_bits(c["n_limbs"]) - 1
    assert sum(v >= c["lifted"] for v in c["values"]) >= 130
    arr = ph.planes_array(c["planes"])
    for path in ("ml", "u192") if c["n_limbs"] == 2 else ("ml",):
        got = mk.planes_mod(arr, c["order"], c["digit_bits"], path)
        assert got == c["want"], f"{path}: {ph.first_diff(got, c['want'])}"
    if c["n_limbs"] > 1:  # u64 orders bring their 32-bit planes only
        eng = CpuPlaneAggregator(c["cfg"], c["cfg"], c["n"])
        out = eng.new_values()
        eng.planes_to_values(ph.planes_tensor(eng, c["planes"]), out, digit_bits=c["digit_bits"])
        assert ph.values_ints(eng, out) == c["want"]


def test_planes_mod_refuses_shapes_outside_the_window():
    order = ph.shape_of((1, 1, 6, 12))[0]
    for path in ("ml", "u192"):
        for k, w in ((5, 32), (4, 63), (0, 32)):
            with pytest.raises(ValueError):
                mk.planes_mod(np.zeros((k, 3), dtype=np.uint64), order, w, path)
        assert mk.planes_mod(np.zeros((4, 3), dtype=np.uint64), order, 32, path) == [0, 0, 0]
    with pytest.raises(ValueError):
        mk.planes_mod(np.zeros((2, 3), dtype=np.uint64), 2**45 + 1, 32, "u192")  # one limb
    with pytest.raises(ValueError):
        mk.planes_mod(np.zeros((2, 3), dtype=np.int64), 2**45 + 1, 32, "ml")  # not uint64


@pytest.mark.parametrize("case", ph.CASES, ids=ph.case_id)
def test_cpu_engine_round(case):
    """CpuPlaneAggregator on the respelled planes: planes_to_values,
    recode_planes and every unmask form give the reference."""
    c = ph.case(*case)
    w = c["digit_bits"]
    eng = ph.engine_for(CpuPlaneAggregator, c)
    planes = ph.planes_tensor(eng, c["planes"])

    out = eng.new_values()
    eng.planes_to_values(planes, out, digit_bits=w)
    assert not ph.first_diff(ph.values_ints(eng, out), c["masked"])

    if w == 32 and eng.wide:
        eng.acc.copy_(planes)
        for world in (2, 8):
            k2, w2 = compact_digits(c["order"], world)
            got = eng.recode_planes(torch.full((k2, c["n"]), -1, dtype=torch.int64), w2)
            want = [list(r) for r in zip(*(ph.digits_of(v, k2, w2) for v in c["masked"]))]
            assert ph.plane_ints(got) == want, f"world {world}"

    for form, model in ph.unmask_forms(eng, c, planes).items():
        ph.assert_model(c, model, form)
    if not eng.wide and w == 32:
        vals = torch.from_numpy(np.array(ph.lifted_values(c), dtype=np.uint64).view(np.int64))
        model = eng.unmask_values(vals, ph.values_tensor(eng, c["mask"]), c["mask_unit"],
                                  c["nb"]).numpy()
        ph.assert_model(c, model, "unmask_values")


# ------------------------------------------------------------ window check


def test_cpu_engine_window_check():
    cfg = mk.MaskConfig(1, 1, 6, 12)
    ph.check_window(CpuPlaneAggregator(cfg, cfg, 5))


def test_window_rule_per_width():
    """plane_window_ok is (k - 1) * w + 64 <= 64 (L + 1) - 1 at every width."""
    for cfg in ph.CONFIGS:
        eng = CpuPlaneAggregator(mk.MaskConfig(*cfg), mk.MaskConfig(*cfg), 1)
        for k in range(1, 14):
            for w in (1, 29, 31, 32, 33, 43, 54, 63):
                assert eng.plane_window_ok(k, w) == ph.window_ok(k, w, eng.n_limbs)


# -------------------------------------------------------------- 2^31 updates


def test_accumulator_refuses_more_than_2_31_updates():
    assert MAX_UPDATES_PER_ACCUMULATOR == 2**31
    cfg = mk.MaskConfig(1, 0, 0, 6)
    n = 5
    eng = CpuPlaneAggregator(cfg, cfg, n)
    pool = eng.alloc_update_pool(2)
    pool.copy_(torch.from_numpy(np.random.default_rng(5).integers(
        0, 256, tuple(pool.shape), dtype=np.uint8)))
    pool[:, 6:n * eng.bpn:eng.bpn] = 0  # canonical-sized limbs, not that it matters
    eng.acc.fill_((2**31 - 1) * (2**32 - 1))
    eng.nb_models = 2**31 - 1
    before = eng.acc.clone()
    eng.aggregate_pool(pool, 1, unit_sum=3)
    assert eng.nb_models == 2**31 and eng.unit_acc == 3
    assert int(eng.acc.min()) >= 0 and not torch.equal(eng.acc, before)
    before = eng.acc.clone()
    with pytest.raises(OverflowError):
        eng.aggregate_pool(pool, 1, unit_sum=3)
    assert torch.equal(eng.acc, before) and eng.nb_models == 2**31 and eng.unit_acc == 3
    eng.nb_models = 2**31 - 1
    with pytest.raises(OverflowError):
        eng.aggregate_pool(pool, 2)
    assert torch.equal(eng.acc, before) and eng.nb_models == 2**31 - 1
    eng.reset()
    eng.aggregate_pool(pool, 2)
    assert eng.nb_models == 2
