"""The rational model encoder on the host: _core.sdk.model_codec_encode_ratio,
the host instantiation of the element functions the K7r kernels compile
(ml_gcd, exact division, mc_ratio_write), against the Fraction reference of
tests/model_encode_ratio_ref.py, byte for byte; and CpuPlaneAggregator's
encode_model_rational against the CPU plane's own body."""
import math

import numpy as np
import pytest

import model_encode_ratio_ref as ref
import unmask_edges as ue
from unmask_exact_inputs import mk

from xaynet_amd import _core

# one config per limb count: its order bounds |d|
CONFIGS = {1: (1, 0, 4, 3), 2: (1, 1, 4, 9), 3: (1, 3, 255, 12), 5: (1, 0, 255, 3)}


def divisors(n_limbs):
    """A one-digit Q, one of half the width, and one of the full width of the
    limbs; each 2^4 * 3^2 * 5 * 7 times something, so that proper common
    factors exist."""
    top = 2 ** (64 * n_limbs)
    return [5040, (2 ** (32 * n_limbs) // 5040 + 1) * 5040, (top - 1) // 5040 * 5040]


def elements(q, n_limbs):
    order = int(mk.MaskConfig(*CONFIGS[n_limbs]).order)
    top = 2 ** (64 * n_limbs)
    ds = [0, 1, -1, q, -q,
          q + 1, -(q + 1),                       # gcd 1
          8 * 1000003, -16 * 999983,             # a power of two, a proper factor of both
          21 * 1000003, -(3 * 7 * 999983),       # an odd proper factor
          2 ** 2 * 3 * 1000003,                  # both
          2 ** (64 * (n_limbs - 1) + 20) + 1,    # top limb with a zero high half
          -(2 ** (64 * (n_limbs - 1) + 32) - 2),
          order - 1, -(order - 1)]
    if 3 * q < top:  # +-3Q is no L-limb value under the full-width Q
        ds += [3 * q, -3 * q]
    assert all(abs(d) < top for d in ds)
    return ds


@pytest.mark.parametrize("n_limbs", [1, 2, 3, 5])
def test_encode_ratio_matches_fraction(n_limbs):
    for q in divisors(n_limbs):
        assert 0 < q < 2 ** (64 * n_limbs)
        ds = elements(q, n_limbs)
        gcds = {math.gcd(abs(d), q) for d in ds}
        assert {1, 8, 16, 21, 12, q} <= gcds
        got = _core.sdk.model_codec_encode_ratio([d < 0 for d in ds], [abs(d) for d in ds], q,
                                                 limbs=n_limbs)
        want = ref.body(ds, q)
        assert got == want, f"L={n_limbs} q={q}: first difference at byte " \
            f"{next(i for i, (a, b) in enumerate(zip(got + b'x', want + b'y')) if a != b)}"
    assert len(ref.body([0], 7)) == 9 + 4 * 7
    full = 2 ** (64 * n_limbs) - 1  # every digit of both sides: 6 + 4L words
    assert len(_core.sdk.model_codec_encode_ratio([False], [full - 1], full, limbs=n_limbs)) \
        == 9 + 4 * (6 + 4 * n_limbs)


def test_encode_ratio_refuses():
    enc = _core.sdk.model_codec_encode_ratio
    for args in (([False], [1, 2], 3), ([False], [1], 0), ([False], [-1], 3),
                 ([False], [2**320], 3), ([False], [1], 2**320)):
        with pytest.raises(ValueError):
            enc(*args)
    with pytest.raises(ValueError):
        enc([False], [2**64], 3, limbs=1)
    assert enc([], [], 3) == b"\x01" + bytes(8)


@pytest.mark.parametrize("cfg_args", [(1, 0, 4, 3), (1, 3, 2, 3), (1, 1, 4, 9), (1, 0, 255, 3)],
                         ids=["f32-b4", "i64-b2", "f64-b4", "f32-bmax"])
def test_cpu_plane_body_is_the_oracle_body(cfg_args):
    """mask_model + Aggregation on real MaskObjects: the body the CPU plane
    publishes (Aggregation.unmask + encode_option_model) is the bytes of
    CpuPlaneAggregator.encode_model_rational for the same sums and masks."""
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    n, scalars = 48, ((1, 3), (1, 5), (1, 7))
    cfg = mk.MaskConfig(*cfg_args)
    pair = mk.MaskConfigPair(cfg, cfg)
    rng = np.random.default_rng(11)
    agg, mask_agg = mk.Aggregation(pair, n), mk.Aggregation(pair, n)
    for j, (num, den) in enumerate(scalars):
        seed = bytes([j + 1]) * 32
        w = rng.normal(0, 0.5, n)
        w[:3] = (0.0, 1.0, -1.0)
        if cfg_args[1] >= 2:
            w = np.round(w * 50)
        agg.aggregate(mk.mask_model(seed, mk.Scalar(num, den), w.astype(ue.NP_DTYPES[cfg_args[1]]),
                                    pair))
        mask_agg.aggregate(mk.derive_mask(seed, n, pair))
    want = agg.unmask_body(mask_agg.object)
    eng = CpuPlaneAggregator(cfg, cfg, n)
    eng.unit_acc = int(agg.object.unit_value)
    eng.acc.copy_(ue.planes_tensor(eng, [int(agg.object.element(i)) for i in range(n)],
                                   eng.n_digits, 32))
    mask = ue.values_tensor(eng, [int(mask_agg.object.element(i)) for i in range(n)])
    got = eng.encode_model_rational(mask, int(mask_agg.object.unit_value), nb_models=len(scalars))
    assert got.tobytes() == want
