"""The exact update quantiser (csrc/gpu/mask_quant.h) on the host: the text
the K5w exact kernel compiles, checked against the rational oracle with no
tolerance, and the form checks of the `_hip.mask_weights` keywords that select
it. No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest

import mask_exact_inputs as mx

mk = mx.mk


@pytest.mark.parametrize("scalar", mx.SCALARS, ids=lambda s: f"{s[0]}_{s[1]}")
@pytest.mark.parametrize("cfg_args", mx.CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_quantize_exact_equals_oracle(cfg_args, scalar):
    num, den = scalar
    p, q = mx.clamped_scalar(cfg_args, num, den)
    got = mk.quantize_exact(mx.weights(cfg_args), mk.MaskConfig(*cfg_args), p, q)
    want = mx.oracle_values(cfg_args, num, den)
    assert len(got) == mx.N
    bad = [i for i in range(mx.N) if int(got[i]) != want[i]]
    assert not bad, (len(bad), bad[:5], [(got[i], want[i]) for i in bad[:3]])


def test_quantize_exact_takes_elements_as_typed():
    """An f32 vector under an f64 config is quantised from its f32 values."""
    cfg = mk.MaskConfig(1, 1, 0, 3)
    w32 = np.array([1 / 3, -1e-10, 0.75], dtype=np.float32)
    assert mk.quantize_exact(w32, cfg, 1, 3) == mk.quantize_exact(w32.astype(np.float64), cfg, 1, 3)
    assert mk.quantize_exact(np.array([7, -7], np.int32), cfg, 1, 9) == \
        mk.quantize_exact(np.array([7, -7], np.int64), cfg, 1, 9)


def test_quantize_exact_rejects_wide_scalars_and_f64_bmax():
    cfg = mk.MaskConfig(1, 0, 0, 3)
    w = np.zeros(1, np.float32)
    for num, den in [(2**63, 1), (1, 2**63), (1, 0), (-1, 1)]:
        with pytest.raises(ValueError):
            mk.quantize_exact(w, cfg, num, den)
    with pytest.raises(ValueError):  # 2112-bit order
        mk.quantize_exact(np.zeros(1), mk.MaskConfig(1, 1, 255, 3), 1, 1)
    assert mk.quantize_exact(w, cfg, 2**63 - 1, 2**63 - 1) == [str(10**10)]


def test_quantize_exact_property():
    """Random finite and special floats under random reduced scalars, for a
    u64, a u128 and a Bmax order."""
    hyp = pytest.importorskip("hypothesis")
    st = hyp.strategies

    specials = [0.0, -0.0, 1.0, -1.0, float("inf"), float("-inf"), float("nan")]
    cases = {
        (1, 0, 0, 6): (32, [1e-45, -1e-45, 3.4e38]),
        (1, 1, 0, 3): (64, [5e-324, -5e-324, 1.7e308]),
        (1, 0, 255, 3): (32, [1e-45, -1e-45, 3.4e38]),
    }

    @hyp.settings(max_examples=150, deadline=None)
    @hyp.given(data=st.data(), cfg_args=st.sampled_from(sorted(cases)),
               num=st.integers(0, 2**63 - 1), den=st.integers(1, 2**63 - 1),
               small=st.booleans())
    def check(data, cfg_args, num, den, small):
        width, edge = cases[cfg_args]
        if small:  # scalars at most 1 keep more elements off the clamp
            num = num % (den + 1)
        elems = st.one_of(st.floats(width=width, allow_nan=False, allow_infinity=False),
                          st.floats(-1.5, 1.5, width=width),
                          st.sampled_from(specials + edge))
        w = np.array(data.draw(st.lists(elems, min_size=1, max_size=24)),
                     dtype=mx.NP_DTYPES[cfg_args[1]])
        p, q = mx.clamped_scalar(cfg_args, num, den)
        hyp.assume(p < 2**63 and q < 2**63)
        cfg = mk.MaskConfig(*cfg_args)
        pair = mk.MaskConfigPair(cfg, cfg)
        order = int(cfg.order)
        masked = mk.mask_model_oracle(mx.SEED, mk.Scalar(num, den), w, pair)
        mask = mk.derive_mask(mx.SEED, len(w), pair)
        want = [(int(masked.element(i)) - int(mask.element(i))) % order for i in range(len(w))]
        assert [int(v) for v in mk.quantize_exact(w, cfg, p, q)] == want

    check()


# ---- `_hip.mask_weights(..., scalar_num, scalar_den)`: form checks, len = 0

U64_ORDER = mk.MaskConfig(1, 0, 0, 6).order
EXP = str(10**10)


def test_mask_weights_exact_keyword_forms():
    _hip = pytest.importorskip("xaynet_amd._hip", reason="_hip extension not built")

    def call(add_shift=1.0, **kw):
        return _hip.mask_weights(0, 0, 0, 0, 0, 0, 6, U64_ORDER, 1.0, add_shift, EXP, **kw)

    call()  # the old positional call
    call(scalar_num=1, scalar_den=3)
    call(scalar_num=0, scalar_den=1)
    call(scalar_num=2**63 - 1, scalar_den=2**63 - 1)
    for kw in ({"scalar_num": 2**63, "scalar_den": 1}, {"scalar_num": 1, "scalar_den": 2**63},
               {"scalar_num": 2**70, "scalar_den": 2**70},
               {"scalar_num": 1, "scalar_den": 0}):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):  # the exact kernel takes add_shift as an integer
        call(add_shift=1.5, scalar_num=1, scalar_den=1)
    call(add_shift=1.5)  # the double kernel does not mind
    # a Bmax order (L = 5) with its 2^128-sized add_shift
    c = mk.MaskConfig(1, 0, 255, 3)
    _hip.mask_weights(0, 0, 0, 0x1000, 0, 0, c.bytes_per_number, c.order, 1.0,
                      float((2**24 - 1) << 104), str(10**45), scalar_num=1, scalar_den=3)
