"""K4 unmask on the GPU at exact quotients, clamp bounds and through every
entry form, against the Fraction reference of tests/unmask_edges.py (pinned to
the oracle in tests/test_unmask_edges_cpu.py, which runs the same matrix on the
CPU plane).

Integer models: wherever exp_shift * scalar_sum is an integer the result is the
exact truncated quotient - also where that quotient is itself an integer and a
double one ulp low would truncate to the integer below (k = 3, 6, 9, 11; k = 4,
whose scalar_sum is exactly 1.0, is the control). Float models keep the double
steps and hold the error bound of unmask_edges.float_bound: on the GPU the
largest error seen is 0.04 of it.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import unmask_edges as ue  # noqa: E402

pytestmark = pytest.mark.gpu


def gpu_engine(case):
    from xaynet_amd.ops import GpuMaskedAggregator, gpu_available

    if not gpu_available():
        pytest.fail("GPU expected for -m gpu tests but not available")
    return GpuMaskedAggregator(case["vect_cfg"], case["unit_cfg"], case["n"])


@pytest.mark.parametrize("case", ue.INTEGER_CASES, ids=ue.case_id)
def test_integer_unmask_exact(case):
    """unmask, unmask_planes, unmask_values / compact planes and two column
    shards all return the truncated exact quotient."""
    cfg, scalars = case
    rnd = ue.forge(cfg, cfg, scalars)
    assert rnd["exact"].mean() >= 0.25
    eng = gpu_engine(rnd)
    assert (eng.wide, eng.bpn == 9) == ((cfg[2] == 6),) * 2  # B6/M3: the lo/hi path
    outs = ue.unmask_forms(eng, rnd)
    assert set(outs) == {"unmask", "unmask_planes", "shards",
                         "compact_planes" if eng.wide else "unmask_values"}
    for form, out in outs.items():
        assert out.dtype == rnd["np_type"]
        bad = np.nonzero(out != rnd["ref"])[0]
        print(f"{ue.case_id(case)} {form}: {bad.size} wrong, equal-weight columns "
              f"{sorted({rnd['columns'][i][0] for i in bad if len(set(rnd['columns'][i])) == 1})}")
        assert bad.size == 0, (f"{form}: {bad.size} wrong, first {bad[:5]}: columns "
                               f"{[rnd['columns'][i] for i in bad[:5]]} got {out[bad[:5]]} "
                               f"want {rnd['ref'][bad[:5]]}")


def test_integer_unmask_without_exact_divisor():
    """An I32 vector config under an F64 unit config: exp_shift * scalar_sum
    is no integer, so the double steps stay; the GPU equals the CPU plane doing
    the same and both are within 1 of the reference."""
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    vect, unit, scalars = ue.NO_DIVISOR_CASE
    rnd = ue.forge(vect, unit, scalars)
    eng = gpu_engine(rnd)
    cpu = CpuPlaneAggregator(rnd["vect_cfg"], rnd["unit_cfg"], rnd["n"])
    expect = ue.unmask_forms(cpu, rnd)["unmask"]
    assert eng._unmask_scalars(rnd["mask_unit"], rnd["nb"])[1]["divisor"] is None
    for form, out in ue.unmask_forms(eng, rnd).items():
        assert (out == expect).all(), form
        assert np.abs(out.astype(np.int64) - rnd["ref"]).max() <= 1, form


@pytest.mark.parametrize("case", ue.FLOAT_CASES, ids=ue.case_id)
def test_float_unmask_within_bound(case):
    """f32 on a u64 order and f64 on a wide one (exp_shift 10^20): all entry
    forms agree bit for bit and hold the bound against the once-rounded exact
    quotient."""
    cfg, scalars = case
    rnd = ue.forge(cfg, cfg, scalars)
    bound = ue.float_bound(rnd)
    ref = rnd["ref"].astype(np.float64)
    outs = ue.unmask_forms(gpu_engine(rnd), rnd)
    for form, out in outs.items():
        assert out.dtype == rnd["np_type"]
        assert (out == outs["unmask"]).all(), form
        err = np.abs(out.astype(np.float64) - ref)
        print(f"{ue.case_id(case)} {form}: max err/bound {np.max(err / bound):.3f}")
        assert (err <= bound).all(), f"{form}: {np.max(err / bound):.3f} of the bound"
