"""K2 and K4 on the GPU at full digit-plane headroom.

The inputs and the Python-integer reference of tests/plane_headroom.py (pinned
on the host instantiation of the same arithmetic and on the CPU plane in
tests/test_plane_headroom_cpu.py): plane entries up to 2^31 * (2^32 - 1), up to
2^64 - 1, and - compact planes - up to 2^63, where the recombination carries
through every limb and the reduction mod order runs tens of steps.

Kernels reached, by config (32-bit planes at both tops unless noted):
  (0,2,0,3)    k2_canonicalize; k4_unmask_offset<.,1> with divisor, from
               planes and (unmask_values) from value sums
  (1,0,4,3)    k4_unmask and k4_unmask_values (double steps)
  (1,3,6,3)    k2_canonicalize_u128<32>, <0> (2x33), k2_recode_planes_u128,
               k4_unmask_offset<.,2> with divisor
  (1,1,4,9)    k4_unmask_u128<.,32> and <.,0> (2x56), exp_shift 10^20
  (1,1,6,12)   the same at a 128-bit order; compact 3x43
  (1,2,255,3)  k4_unmask_offset<.,2>, Bmax
  (2,3,255,9), (1,3,255,12)
               k2_canonicalize_ml<3>, k2_recode_planes_ml<3>,
               k4_unmask_offset<.,3> with 4 and 5 planes
  (1,0,255,3), (2,0,255,12)
               the same at <5>, f32 output
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import plane_headroom as ph  # noqa: E402
from plane_headroom import mk  # noqa: E402

pytestmark = pytest.mark.gpu


def gpu_engine(c):
    from xaynet_amd.ops import GpuMaskedAggregator, gpu_available

    if not gpu_available():
        pytest.fail("GPU expected for -m gpu tests but not available")
    return ph.engine_for(GpuMaskedAggregator, c)


@pytest.mark.parametrize("case", ph.CASES, ids=ph.case_id)
def test_planes_to_values(case):
    """K2 canonicalize of the respelled planes is the Python sum mod order,
    the ripple columns one by one."""
    c = ph.case(*case)
    eng = gpu_engine(c)
    out = eng.new_values().fill_(-1)
    eng.planes_to_values(ph.planes_tensor(eng, c["planes"]), out, digit_bits=c["digit_bits"])
    got = ph.values_ints(eng, out)
    for i in range(c["n_ripple"]):
        assert got[i] == c["masked"][i], (
            f"ripple column {i} {[hex(p[i]) for p in c['planes']]}: got {got[i]:#x} "
            f"want {c['masked'][i]:#x}")
    assert got == c["masked"], ph.first_diff(got, c["masked"])


@pytest.mark.parametrize("cfg", [c for c in ph.CONFIGS if ph.shape_of(c)[2] > 1], ids=ph.cfg_id)
def test_top_of_the_window(cfg):
    """K2 canonicalize on values in the top half of the reduction window
    (plane shapes that meet the window rule with equality): the divisor of
    the shift-subtract loop grows to its last step."""
    c = ph.edge_case(cfg)
    eng = gpu_engine({"cfg": c["cfg"], "n": c["n"], "unit_acc": 0})
    out = eng.new_values().fill_(-1)
    eng.planes_to_values(ph.planes_tensor(eng, c["planes"]), out, digit_bits=c["digit_bits"])
    got = ph.values_ints(eng, out)
    assert got == c["want"], ph.first_diff(got, c["want"])


@pytest.mark.parametrize("case", [c for c in ph.CASES if c[1][1] == 32 and
                                  ph.shape_of(c[0])[2] > 1], ids=ph.case_id)
def test_recode_planes(case):
    """K2 recode of a full accumulator writes exactly the w-bit digits of the
    value mod order, for a 2- and an 8-rank world."""
    from xaynet_amd.parallel import compact_digits

    c = ph.case(*case)
    eng = gpu_engine(c)
    eng.acc.copy_(ph.planes_tensor(eng, c["planes"]))
    for world in (2, 8):
        k2, w2 = compact_digits(c["order"], world)
        got = eng.recode_planes(torch.full((k2, c["n"]), -1, dtype=torch.int64, device="cuda"),
                                w2)
        want = [list(r) for r in zip(*(ph.digits_of(v, k2, w2) for v in c["masked"]))]
        assert ph.plane_ints(got) == want, f"world {world}"


@pytest.mark.parametrize("case", ph.CASES, ids=ph.case_id)
def test_unmask(case):
    """K4 through unmask, unmask_planes, two column shards and - u64 orders -
    unmask_values on masked + m * order just below 2^64. Integer models are
    the reference exactly. Float models are bit-equal to the same kernel's
    result on the small-entry planes of the same round (the double steps see
    only t) and hold the existing bound against the reference."""
    c = ph.case(*case)
    eng = gpu_engine(c)
    outs = ph.unmask_forms(eng, c, ph.planes_tensor(eng, c["planes"]))
    assert set(outs) == {"unmask_planes", "shards"} | ({"unmask"} if c["digit_bits"] == 32
                                                       else set())
    if not eng.wide:
        lifted = ph.lifted_values(c)
        assert max(lifted) >= 2**64 - c["order"]
        vals = torch.from_numpy(np.array(lifted, dtype=np.uint64).view(np.int64)).to("cuda")
        outs["unmask_values"] = eng.unmask_values(
            vals, ph.values_tensor(eng, c["mask"]), c["mask_unit"], c["nb"]).cpu().numpy()
    for form, out in outs.items():
        ph.assert_model(c, out, form)
    if c["is_float"]:
        plain = ph.unmask_forms(eng, c, ph.planes_tensor(eng, c["plain"]))
        for form, out in outs.items():
            small = plain["unmask_planes" if form == "unmask_values" else form]
            assert np.array_equal(out.view(np.uint8), small.view(np.uint8)), form


@pytest.mark.parametrize("case", ph.CASES, ids=ph.case_id)
def test_adds_on_top_of_full_planes(case):
    """values_to_planes and - 32-bit planes below 2^63, where three more digits
    still fit an entry - add_rows_to_planes of 3 rows onto planes pre-filled
    with `top`: every entry is top + the digits, and the planes read back as
    the Python sum mod order."""
    c = ph.case(*case)
    k, w, top_name = c["form"]
    order, top, n = c["order"], c["top"], c["n"]
    eng = gpu_engine(c)
    rows = [c["masked"], c["mask"], [(order - 1 - v) for v in c["masked"]]]
    rows = rows if top_name == "doc" else rows[:1]
    planes = ph.planes_tensor(eng, [[top] * n] * k)
    if len(rows) > 1:
        eng.add_rows_to_planes(torch.stack([ph.values_tensor(eng, r) for r in rows]), planes)
    else:
        eng.values_to_planes(ph.values_tensor(eng, rows[0]), planes, digit_bits=w)
    want = [[top + sum(ph.digits_of(r[i], k, w)[d] for r in rows) for i in range(n)]
            for d in range(k)]
    assert max(max(row) for row in want) < 2**64
    assert ph.plane_ints(planes) == want
    out = eng.new_values()
    eng.planes_to_values(planes, out, digit_bits=w)
    total = sum(top << (w * d) for d in range(k))
    assert ph.values_ints(eng, out) == [(total + sum(r[i] for r in rows)) % order
                                        for i in range(n)]
    if len(rows) > 1:  # and one row through values_to_planes on top of that
        eng.values_to_planes(ph.values_tensor(eng, rows[0]), planes, digit_bits=w)
        eng.planes_to_values(planes, out, digit_bits=w)
        assert ph.values_ints(eng, out) == [(total + sum(r[i] for r in rows) + rows[0][i])
                                            % order for i in range(n)]


def test_gpu_engine_window_check():
    """[5, n] x 32 and [4, n] x 63 planes of a 128-bit order could spell 2^192
    and more: refused, outputs untouched; every shape in use still passes."""
    from xaynet_amd.ops import GpuMaskedAggregator, gpu_available

    if not gpu_available():
        pytest.fail("GPU expected for -m gpu tests but not available")
    cfg = mk.MaskConfig(1, 1, 6, 12)
    ph.check_window(GpuMaskedAggregator(cfg, cfg, 130))


def test_launchers_refuse_shapes_outside_the_window():
    """Below the engine: _hip itself refuses the shapes, for callers that
    bring their own pointers."""
    from xaynet_amd import _hip

    order = ph.shape_of((1, 1, 6, 12))[0]
    n = 130
    out = torch.full((2, n), 7, dtype=torch.int64, device="cuda")
    for k, w in ((5, 32), (4, 63)):
        planes = torch.ones(k, n, dtype=torch.int64, device="cuda")
        with pytest.raises(RuntimeError):
            _hip.canonicalize(planes.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), n, k,
                              str(order), w)
        with pytest.raises(RuntimeError):
            _hip.unmask(planes.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                        out.data_ptr(), n, k, str(order), str(10**20), 3.0, 1.0, 1, w)
    compact = torch.full((3, n), 7, dtype=torch.int64, device="cuda")
    acc = torch.ones(5, n, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):
        _hip.recode_planes(acc.data_ptr(), compact.data_ptr(), n, 5, str(order), 3, 43)
    torch.cuda.synchronize()
    assert int(out.min()) == 7 == int(out.max()) and int(compact.min()) == 7 == int(compact.max())


def test_accumulator_refuses_more_than_2_31_updates():
    """aggregate_pool raises before it launches K3."""
    from xaynet_amd.ops import GpuMaskedAggregator, gpu_available

    if not gpu_available():
        pytest.fail("GPU expected for -m gpu tests but not available")
    cfg = mk.MaskConfig(1, 0, 0, 6)
    eng = GpuMaskedAggregator(cfg, cfg, 130)
    pool = eng.alloc_update_pool(2).fill_(1)
    eng.nb_models = 2**31 - 1
    eng.aggregate_pool(pool, 1)
    assert eng.nb_models == 2**31
    before = eng.acc.clone()
    assert int(before.max()) > 0
    with pytest.raises(OverflowError):
        eng.aggregate_pool(pool, 1)
    assert torch.equal(eng.acc, before) and eng.nb_models == 2**31
