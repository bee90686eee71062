"""The exact float unmask on the GPU (k4_unmask_exact, L = 1, 2, 3 and 5):
every entry form returns the rational d / Q rounded once, bit for bit, against
the Fraction reference of tests/unmask_exact_inputs.py (pinned to the oracle
in tests/test_unmask_exact_cpu.py, which runs the same matrix on the CPU
plane); default-mode calls are what they were; and one in-process round
through GpuCoordinatorDriver(exact_unmask=True) publishes the CPU
coordinator's rational model rounded once.
"""
import struct
import time
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import unmask_edges as ue  # noqa: E402
import unmask_exact_inputs as ux  # noqa: E402
from unmask_exact_inputs import mk  # noqa: E402

from xaynet_amd import _core  # noqa: E402

pytestmark = pytest.mark.gpu


def gpu_engine(rnd):
    from xaynet_amd.ops import GpuMaskedAggregator, gpu_available

    if not gpu_available():
        pytest.fail("GPU expected for -m gpu tests but not available")
    return GpuMaskedAggregator(rnd["vect_cfg"], rnd["unit_cfg"], rnd["n"])


def cpu_engine(rnd):
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    return CpuPlaneAggregator(rnd["vect_cfg"], rnd["unit_cfg"], rnd["n"])


def check_round(rnd, what):
    """Exact mode: every form is the reference and the CPU plane, bit for
    bit. Default mode: every form is the CPU plane's default, as before."""
    eng, cpu = gpu_engine(rnd), cpu_engine(rnd)
    outs = ux.unmask_forms(eng, rnd)
    assert set(outs) == {"unmask", "unmask_planes", "shards",
                         "compact_planes" if eng.wide else "unmask_values"}
    cpu_outs = ux.unmask_forms(cpu, rnd)
    for form, out in outs.items():
        bad = int((ux.bits(out) != ux.bits(rnd["ref"])).sum())
        print(f"{what} {form}: {bad} of {rnd['n']} differ from the reference")
        ux.assert_bits_equal(out, rnd["ref"], f"{what} {form}")
        ux.assert_bits_equal(out, cpu_outs[form], f"{what} {form} vs the CPU plane")
    default = ue.unmask_forms(eng, rnd, rnd["dtype"])
    cpu_default = ue.unmask_forms(cpu, rnd, rnd["dtype"])
    for form, out in default.items():
        bad = int((ux.bits(out) != ux.bits(cpu_default[form])).sum())
        print(f"{what} default {form}: {bad} of {rnd['n']} differ from the CPU plane")
        ux.assert_bits_equal(out, cpu_default[form], f"{what} default {form}")
    return default


@pytest.mark.parametrize("case", ue.FLOAT_CASES, ids=ue.case_id)
def test_forged_float_cases_exact(case):
    """The existing float cases (f32 on a u64 order, f64 on a wide one): the
    once-rounded quotient in exact mode, where the double steps miss it."""
    rnd = ux.forged(case)
    ux.assert_double_steps_miss(rnd, 0.5 if case[0] == (1, 1, 4, 9) else 0.005)
    default = check_round(rnd, ue.case_id(case))
    missed = int((ux.bits(default["unmask"]) != ux.bits(rnd["ref"])).sum())
    print(f"{ue.case_id(case)}: the default kernel misses the reference in {missed} elements")
    assert missed > 0


@pytest.mark.parametrize("entry", ux.CRAFTED, ids=ux.crafted_id)
def test_crafted_rounds_exact(entry):
    """Ties with even and odd neighbours, the integers next to them,
    representable quotients, 0, +-1, +-C, every bit length; f32 output under
    the wide configs down to the subnormal grid and up past f32 max."""
    rnd = ux.craft(*entry)
    eng = gpu_engine(rnd)
    assert eng.n_limbs == ux.LIMBS[entry[0]]
    check_round(rnd, ux.crafted_id(entry))
    eng.unit_acc = rnd["unit_acc"]
    eng.acc.copy_(ue.planes_tensor(eng, rnd["lifted"], eng.n_digits, 32))
    f32 = eng.unmask_f32(ue.values_tensor(eng, rnd["mask"]), rnd["mask_unit"], rnd["nb"],
                         exact=True).cpu().numpy()
    want = np.array([ux.round_exact(x, np.float32) for x in rnd["quotients"]], dtype=np.float32)
    ux.assert_bits_equal(f32, want, "unmask_f32")


def test_exact_mode_refusals():
    """The engine's ValueErrors, before any launch."""
    rnd = ue.forge((1, 0, 4, 3), (1, 1, 4, 3), ue.equal_scalars(3))
    eng = gpu_engine(rnd)
    with pytest.raises(ValueError, match="exact unmask"):
        ux.unmask_forms(eng, dict(rnd, dtype=0))
    vect, unit, scalars = ue.NO_DIVISOR_CASE
    rnd = ue.forge(vect, unit, scalars)
    with pytest.raises(ValueError, match="integer model"):
        ux.unmask_forms(gpu_engine(rnd), dict(rnd, dtype=None))
    cfg, scalars = ue.INTEGER_CASES[0]
    rnd = ue.forge(cfg, cfg, scalars)
    for form, out in ux.unmask_forms(gpu_engine(rnd), dict(rnd, dtype=None)).items():
        assert (out == rnd["ref"]).all(), form


# --------------------------------------------------------------- coordinator


def _rational_body(body: bytes):
    """The Option<Model> bincode body as Fractions: head 01, u64 n, then per
    element numerator and denominator as sign u32 (0 minus, 1 zero, 2 plus),
    u64 digit count, u32 digits from the lowest."""
    assert body[0] == 1
    (n,) = struct.unpack_from("<Q", body, 1)
    words = np.frombuffer(body, dtype="<u4", offset=9)
    pos, out = 0, []

    def big():
        nonlocal pos
        sign, count = int(words[pos]), int(words[pos + 1]) | int(words[pos + 2]) << 32
        value = sum(int(w) << (32 * j) for j, w in enumerate(words[pos + 3 : pos + 3 + count]))
        pos += 3 + count
        return -value if sign == 0 else value

    for _ in range(n):
        num = big()
        out.append(Fraction(num, big()))
    assert pos == len(words)
    return out


def _run_round(staged: bool, weights, length: int, make_driver=None):
    """One in-process round; returns the published body."""
    co, sdk = _core.coordinator, _core.sdk
    s = co.Settings()
    s.sum_prob = 0.5
    s.update_prob = 1.0
    s.model_length = length
    c = mk.MaskConfig(1, 0, 4, 3)  # Prime/F32/B4/M3
    s.mask_cfg = mk.MaskConfigPair(c, c)
    s.set_sum(1, 100, 0.05, 3.0)
    s.set_update(3, 100, 0.05, 3.0)
    s.set_sum2(1, 100, 0.05, 3.0)
    coord = co.Coordinator(s, co.InMemoryStorage(), co.InMemoryModels(), staged)
    driver = make_driver(coord, c, length) if staged else None
    if driver is not None:
        driver.start()
    client = sdk.InProcessClient(coord)
    rng = np.random.default_rng(31)
    # 12: a sum participant and at least three updaters in all but 2% of the draws
    participants = [
        sdk.Participant(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), 1, 1, client)
        for _ in range(12)
    ]
    coord.start()
    t0 = time.time()
    body = None
    try:
        while time.time() - t0 < 60.0 and body is None:
            for p in participants:
                p.tick()
                if p.should_set_model:
                    p.set_model(weights)
            got = coord.fetch_model()
            if got and got[0] == 1:
                body = bytes(got)
            time.sleep(0.002)
    finally:
        coord.stop()
        if driver is not None:
            driver.stop()
    assert body is not None, "no global model published"
    if driver is not None:
        assert driver.rounds_unmasked >= 1, "model did not come from the GPU driver"
    return body


def test_coordinator_round_publishes_the_rational_rounded_once():
    """1027 f32 weights under Prime/F32/B4/M3, once through the staged
    coordinator with GpuCoordinatorDriver(exact_unmask=True), once through the
    CPU coordinator, which publishes the rationals themselves. Every
    participant trains the same model with scalar 1, so the rational d / Q =
    k * (v - a * E) / (k * E) is the same whichever k >= 3 updaters a round
    accepted (the protocol needs a sum participant besides them, so there are
    twelve participants, not three). The GPU plane's f32 weights are those
    rationals rounded once, bit for bit."""
    from xaynet_amd.ops.driver import GpuCoordinatorDriver

    length = ux.N
    rng = np.random.default_rng(37)
    weights = rng.normal(0, 0.05, length).astype(np.float32)
    weights[:5] = (0.0, 1e-9, -1e-9, 1e4, -1e4)

    gpu_body = _run_round(
        True, weights, length,
        lambda coord, c, n: GpuCoordinatorDriver(coord, c, c, n, pool_size=4, exact_unmask=True))
    cpu_body = _run_round(False, weights, length)
    rationals = _rational_body(cpu_body)
    assert len(rationals) == length and any(x.denominator > 1 for x in rationals)
    want = np.array([ux.round_exact(x, np.float32) for x in rationals], dtype=np.float32)
    got = np.asarray(_core.sdk.decode_model(gpu_body, 0))
    ux.assert_bits_equal(got, want, "published model")
