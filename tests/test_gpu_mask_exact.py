"""Exact update masking on the GPU (K1 + the K5w exact kernel): the wire
object equals the rational oracle's byte for byte, through the engine, the
participant accelerator and a whole round. Every comparison is equality."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mask_exact_inputs as mx  # noqa: E402
from xaynet_amd import _core  # noqa: E402

co = _core.coordinator
mk = _core.mask
sdk = _core.sdk

pytestmark = pytest.mark.gpu


def _gpu():
    from xaynet_amd.ops import gpu_available

    if not gpu_available():
        pytest.skip("no MI355X visible")


@pytest.mark.parametrize("scalar", mx.GPU_SCALARS, ids=lambda s: f"{s[0]}_{s[1]}")
@pytest.mark.parametrize("cfg_args", mx.CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_mask_weights_exact_equals_oracle(cfg_args, scalar):
    """Whole wire objects; 3/2 exceeds the B0 unit bound, so it pins the
    clamp of the unit part."""
    _gpu()
    from xaynet_amd.ops import GpuMaskedAggregator

    num, den = scalar
    c = mk.MaskConfig(*cfg_args)
    eng = GpuMaskedAggregator(c, c, mx.N)
    wire = eng.mask_weights(mx.SEED, torch.from_numpy(mx.weights(cfg_args).copy()), num, den,
                            exact=True)
    want = bytes(mx.oracle(cfg_args, num, den).serialize())
    if wire != want:
        bpn = c.bytes_per_number
        bad = [i for i in range(mx.N)
               if wire[8 + i * bpn:8 + (i + 1) * bpn] != want[8 + i * bpn:8 + (i + 1) * bpn]]
        w = mx.weights(cfg_args)
        pytest.fail(f"{len(bad)} elements differ, first {bad[:5]}: {[w[i] for i in bad[:5]]}; "
                    f"unit part equal: {wire[8 + mx.N * bpn:] == want[8 + mx.N * bpn:]}")


def test_mask_weights_exact_refuses_a_wide_scalar():
    """Past the clamp a term of 2^63 or more has no exact kernel."""
    _gpu()
    from xaynet_amd.ops import GpuMaskedAggregator

    c = mk.MaskConfig(1, 0, 255, 3)  # the unit bound, f32::MAX, does not clamp 2^70
    eng = GpuMaskedAggregator(c, c, 8)
    with pytest.raises(ValueError):
        eng.mask_weights(mx.SEED, torch.zeros(8), 2**70, 1, exact=True)


def test_accelerator_exact_mode_uses_the_hook_scalar():
    _gpu()
    from xaynet_amd.ops.accel import ParticipantAccel

    cfg_args = (1, 0, 0, 6)
    w = mx.weights(cfg_args)
    accel = ParticipantAccel(exact=True)
    cfg8 = cfg_args + cfg_args
    wire = accel.mask_model(mx.SEED, 0, w.tobytes(), mx.N, cfg8, 1, 3)
    assert wire == bytes(mx.oracle(cfg_args, 1, 3).serialize())
    assert accel.mask_model(mx.SEED, 0, w.tobytes(), mx.N, cfg8, 2**70, 1) is None
    # the default accelerator keeps its constructor scalar and the double kernel
    plain = ParticipantAccel().mask_model(mx.SEED, 0, w.tobytes(), mx.N, cfg8, 1, 3)
    assert plain is not None and len(plain) == len(wire) and plain != wire


def _round(rng, weights, length):
    """One in-process round (CPU aggregation plane) of ten participants of
    scalar 1/3 with an exact accelerator; returns the published model and the
    hook's results."""
    from xaynet_amd.ops.accel import ParticipantAccel

    s = co.Settings()
    s.sum_prob = 0.5
    s.update_prob = 1.0
    s.model_length = length
    c = mk.MaskConfig(1, 0, 0, 6)
    s.mask_cfg = mk.MaskConfigPair(c, c)
    s.set_sum(1, 100, 0.05, 10.0)
    s.set_update(3, 100, 0.05, 10.0)
    s.set_sum2(1, 100, 0.05, 10.0)
    coord = co.Coordinator(s, co.InMemoryStorage(), co.InMemoryModels(), False)
    client = sdk.InProcessClient(coord)
    accel = ParticipantAccel(exact=True)
    hooked = []

    def mask_model(seed, dtype, raw, n, cfg8, num, den):
        wire = accel.mask_model(seed, dtype, raw, n, cfg8, num, den)
        hooked.append((num, den, wire is not None))
        return wire

    participants = []
    for _ in range(10):
        p = sdk.Participant(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), 1, 3, client)
        p.set_mask_model_hook(mask_model)
        p.set_sum2_hook(accel.aggregate_masks)
        participants.append(p)

    coord.start()
    t0 = time.time()
    model = None
    try:
        while time.time() - t0 < 60.0 and model is None:
            for p in participants:
                p.tick()
                if p.should_set_model:
                    p.set_model(weights)
            body = coord.fetch_model()
            if body and body[0] == 1:
                model = np.asarray(sdk.decode_model(body, 0))
    finally:
        coord.stop()
    return model, hooked


def test_round_with_exact_accelerator_publishes_the_oracle_model():
    """Every updater sends the oracle's bytes for the same vector and scalar,
    so the weighted mean is what one oracle-masked copy unmasks to, whoever
    was selected."""
    _gpu()
    length = 4099
    rng = np.random.default_rng(77)
    weights = rng.uniform(-1, 1, length).astype(np.float32)
    weights[:6] = [1.0, -1.0, 0.0, 1e-10, -1e-10, 1 / 3]

    c = mk.MaskConfig(1, 0, 0, 6)
    pair = mk.MaskConfigPair(c, c)
    agg = mk.Aggregation(pair, length)
    agg.aggregate(mk.mask_model_oracle(mx.SEED, mk.Scalar(1, 3), weights, pair))
    want = np.asarray(agg.unmask(mk.derive_mask(mx.SEED, length, pair)), dtype=np.float32)

    for selection in (np.random.default_rng(41), np.random.default_rng(42)):
        model, hooked = _round(selection, weights, length)
        assert model is not None
        assert len(hooked) >= 3 and all(h == (1, 3, True) for h in hooked), hooked
        assert model.dtype == np.float32 and np.array_equal(model, want)
