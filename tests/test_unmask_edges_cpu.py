"""CpuPlaneAggregator unmask at exact quotients, clamp bounds and through every
entry form, against the Fraction reference of tests/unmask_edges.py - the CPU
twin of tests/test_gpu_unmask_edges.py. The reference itself is pinned to the
exact-rational oracle (_core.mask) here."""
import numpy as np
import pytest

import unmask_edges as ue
from unmask_edges import mk


def cpu_engine(case):
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    return CpuPlaneAggregator(case["vect_cfg"], case["unit_cfg"], case["n"])


def assert_inputs_have_edges(case, cfg, scalars):
    """The condition on the inputs, on the reference alone."""
    assert case["exact"].mean() >= 0.25
    k = len(scalars)
    if len(set(scalars)) == 1:
        for w in ue.EXACT_EQUAL_WEIGHTS.get((cfg[2], k), ()):
            i = case["columns"].index((w,) * k)
            assert case["exact"][i] and case["ref"][i] == w
    assert any(abs(s * w) > case["add"] for col in case["columns"]
               for s, w in zip(case["scalars"], col))
    assert (case["ref"] < 0).any() and (case["ref"] > 0).any()


@pytest.mark.parametrize("cfg_args", [(0, 2, 2, 3), (1, 3, 6, 3), (1, 0, 4, 3), (1, 1, 4, 9)],
                         ids=["i32", "i64", "f32", "f64"])
def test_reference_is_the_oracle(cfg_args):
    """mask_model + Aggregation.unmask on the same weights: the oracle's
    masked sums minus its masks are the reference's t and n1, and its model is
    the reference quotient, truncated (integers) or rounded once (floats)."""
    n, scalars = 64, ((1, 3), (1, 5), (1, 7))
    case = ue.forge(cfg_args, cfg_args, scalars, n)
    cfg = case["vect_cfg"]
    pair = mk.MaskConfigPair(cfg, cfg)
    order = case["order"]
    agg, mask_agg = mk.Aggregation(pair, n), mk.Aggregation(pair, n)
    for j, (num, den) in enumerate(scalars):
        seed = bytes([j + 1]) * 32
        w = np.array([col[j] for col in case["columns"]], dtype=case["np_type"])
        agg.aggregate(mk.mask_model(seed, mk.Scalar(num, den), w, pair))
        mask_agg.aggregate(mk.derive_mask(seed, n, pair))
    for i in range(n):
        got = (int(agg.object.element(i)) - int(mask_agg.object.element(i))) % order
        assert got == case["t"][i], f"t[{i}]"
    assert (int(agg.object.unit_value) - int(mask_agg.object.unit_value)) % order == case["n1"]
    oracle = np.asarray(agg.unmask(mask_agg.object))
    assert oracle.dtype == case["np_type"]
    if cfg_args[1] == 1:
        # the oracle's own Ratio -> f64 conversion is good to one ulp, not
        # correctly rounded (17 of these 64 differ, each by exactly one)
        assert (np.abs(oracle - case["ref"]) <= np.spacing(np.abs(case["ref"]))).all()
    else:
        assert (oracle == case["ref"]).all(), np.nonzero(oracle != case["ref"])[0][:5]


@pytest.mark.parametrize("case", ue.INTEGER_CASES, ids=ue.case_id)
def test_integer_unmask_exact(case):
    """Every entry form returns the truncated exact quotient."""
    cfg, scalars = case
    rnd = ue.forge(cfg, cfg, scalars)
    assert_inputs_have_edges(rnd, cfg, scalars)
    eng = cpu_engine(rnd)
    assert eng.wide == (cfg[2] == 6)
    for form, out in ue.unmask_forms(eng, rnd).items():
        assert out.dtype == rnd["np_type"]
        bad = np.nonzero(out != rnd["ref"])[0]
        assert bad.size == 0, (f"{form}: {bad.size} wrong, first {bad[:5]}: columns "
                               f"{[rnd['columns'][i] for i in bad[:5]]} got {out[bad[:5]]} "
                               f"want {rnd['ref'][bad[:5]]}")


def test_integer_unmask_without_exact_divisor():
    """An I32 vector config under an F64 unit config: exp_shift * scalar_sum
    is no integer, the double steps stay, and they are within 1."""
    vect, unit, scalars = ue.NO_DIVISOR_CASE
    rnd = ue.forge(vect, unit, scalars)
    eng = cpu_engine(rnd)
    eng.unit_acc = rnd["unit_acc"]
    assert eng._unmask_scalars(rnd["mask_unit"], rnd["nb"])[1]["divisor"] is None
    outs = ue.unmask_forms(eng, rnd)
    for form, out in outs.items():
        assert (out == outs["unmask"]).all(), form
        assert np.abs(out.astype(np.int64) - rnd["ref"]).max() <= 1, form


@pytest.mark.parametrize("case", ue.FLOAT_CASES, ids=ue.case_id)
def test_float_unmask_within_bound(case):
    """Float models keep the double steps: the emulation of the kernel and
    the CPU plane both hold the bound derived in unmask_edges.float_bound."""
    cfg, scalars = case
    rnd = ue.forge(cfg, cfg, scalars)
    bound = ue.float_bound(rnd)
    ref = rnd["ref"].astype(np.float64)
    assert (np.abs(ref) == rnd["add"]).any() and (ref == 0).any()
    emu = ue.emulate_kernel_doubles(rnd)
    err = np.abs(emu.astype(np.float64) - ref)
    print(f"emulation: max err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    for form, out in ue.unmask_forms(cpu_engine(rnd), rnd).items():
        assert out.dtype == rnd["np_type"]
        err = np.abs(out.astype(np.float64) - ref)
        assert (err <= bound).all(), f"{form}: {np.max(err / bound):.3f} of the bound"
