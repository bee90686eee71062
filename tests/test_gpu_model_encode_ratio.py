"""The rational model body on the GPU (k7r_words / k7r_emit, L = 1, 2, 3 and
5): engine.encode_model_rational against the Fraction reference of
tests/model_encode_ratio_ref.py, byte for byte, on rounds crafted from (Q,
[d]) by tests/unmask_exact_inputs.py; the decoder's rational mode closes the
loop; and one in-process round through GpuCoordinatorDriver(rational_model=
True) publishes the CPU coordinator's bytes.
"""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import model_encode_ratio_ref as ref  # noqa: E402
import unmask_edges as ue  # noqa: E402
import unmask_exact_inputs as ux  # noqa: E402
from unmask_exact_inputs import mk  # noqa: E402

from xaynet_amd import _core  # noqa: E402

pytestmark = pytest.mark.gpu

# one crafted round (tests/unmask_exact_inputs.CRAFTED) per limb count
ROUNDS = {
    1: ((1, 0, 4, 3), 3 * 5**5 * 2**9, ux.F32),
    2: ((1, 1, 4, 9), 5 * 2**58, ux.F64),
    3: ((1, 3, 255, 12), 10**10, ux.F32),
    5: ((1, 0, 255, 3), 10**45, ux.F32),
}
# a block edge on either side, and more than one block total in the scan
LENGTHS = [1, 255, 256, 257, 3 * 256 + 5]
SKIP = 2  # the crafted numerators start 0, 1, -1, -C, C: a slice from -1 on


def gpu_engine(rnd, n):
    from xaynet_amd.ops import GpuMaskedAggregator, gpu_available

    if not gpu_available():
        pytest.fail("GPU expected for -m gpu tests but not available")
    eng = GpuMaskedAggregator(rnd["vect_cfg"], rnd["unit_cfg"], n)
    eng.unit_acc = rnd["unit_acc"]
    return eng


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("n_limbs", sorted(ROUNDS))
def test_encode_model_rational_crafted(n_limbs, n):
    from xaynet_amd.parallel import compact_digits

    rnd = ux.craft(*ROUNDS[n_limbs])
    cut = slice(SKIP, SKIP + n)
    want = ref.body(rnd["d"][cut], rnd["q"])
    eng = gpu_engine(rnd, n)
    assert eng.n_limbs == n_limbs
    mask = ue.values_tensor(eng, rnd["mask"][cut])
    eng.acc.copy_(ue.planes_tensor(eng, rnd["lifted"][cut], eng.n_digits, 32))
    got = eng.encode_model_rational(mask, rnd["mask_unit"], nb_models=rnd["nb"])
    print(f"L={n_limbs} n={n}: {len(got)} bytes, {(len(got) - 9) / n:.1f} a weight")
    assert got.tobytes() == want, "accumulator planes"
    if eng.wide:
        k, bits = compact_digits(rnd["order"], 2)
        planes = ue.planes_tensor(eng, rnd["lifted"][cut], k, bits)
        got = eng.encode_model_rational_planes(planes, mask, rnd["mask_unit"], rnd["nb"],
                                               digit_bits=bits)
        assert got.tobytes() == want, "compact planes"


@pytest.mark.parametrize("n_limbs", [1, 2], ids=["f32", "f64"])
def test_decoder_closes_the_loop(n_limbs):
    """decode_model(rational=True) of the produced body is unmask(exact=True),
    bit for bit: the same rational, rounded once on either way."""
    rnd = ux.craft(*ROUNDS[n_limbs])
    eng = gpu_engine(rnd, rnd["n"])
    mask = ue.values_tensor(eng, rnd["mask"])
    eng.acc.copy_(ue.planes_tensor(eng, rnd["lifted"], eng.n_digits, 32))
    want = eng.unmask(mask, rnd["mask_unit"], nb_models=rnd["nb"], exact=True).cpu().numpy()
    body = eng.encode_model_rational(mask, rnd["mask_unit"], nb_models=rnd["nb"])
    assert body.tobytes() == ref.body(rnd["d"], rnd["q"])
    got = eng.decode_model(body, rnd["dtype"], rational=True)
    assert got is not None
    ux.assert_bits_equal(got.cpu().numpy(), want, "decoded body")
    ux.assert_bits_equal(want, rnd["ref"], "exact unmask")


def test_refusal_before_any_launch():
    """Mismatched exp_shift (an F32 vector under an F64 unit config): Q is no
    integer, and the engine says so as exact mode does."""
    rnd = ue.forge((1, 0, 4, 3), (1, 1, 4, 3), ue.equal_scalars(3))
    eng = gpu_engine(rnd, rnd["n"])
    mask = ue.values_tensor(eng, rnd["mask"])
    with pytest.raises(ValueError, match="exact unmask"):
        eng.encode_model_rational(mask, rnd["mask_unit"], nb_models=rnd["nb"])


# --------------------------------------------------------------- coordinator


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


def test_coordinator_round_publishes_the_cpu_body():
    """1027 f32 weights under Prime/F32/B4/M3, once through the staged
    coordinator with GpuCoordinatorDriver(rational_model=True), once through
    the CPU coordinator. Every participant trains the same model with scalar
    1, so the reduced rational k * (v - a * E) / (k * E) is the same whichever
    k >= 3 updaters a round accepted: the two bodies are the same bytes."""
    from xaynet_amd.ops.driver import GpuCoordinatorDriver

    length = ux.N
    rng = np.random.default_rng(37)
    weights = rng.normal(0, 0.05, length).astype(np.float32)
    weights[:5] = (0.0, 1e-9, -1e-9, 1e4, -1e4)
    gpu_body = _run_round(
        True, weights, length,
        lambda coord, c, n: GpuCoordinatorDriver(coord, c, c, n, pool_size=4,
                                                 rational_model=True))
    cpu_body = _run_round(False, weights, length)
    assert gpu_body == cpu_body
    # and not what the default driver publishes: rounded weights as dyadic rationals
    assert gpu_body != bytes(_core.sdk.encode_model(np.asarray(_core.sdk.decode_model(cpu_body, 0))))
