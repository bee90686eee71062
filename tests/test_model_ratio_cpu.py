"""The rational model decode on the host: _core.sdk.model_codec_decode(...,
rational=True), the walk over mc_read_ratio (csrc/gpu/model_codec.h) that
k7d_emit<T, true> compiles, bit for bit against Fraction rounded once."""
import pytest

import model_codec_inputs as mci
import model_ratio_inputs as mri
from xaynet_amd import _core

sdk = _core.sdk


@pytest.mark.parametrize("name", mci.DTYPES)
def test_values_and_rejections(name):
    code = mci.DTYPE_CODE[name]
    body, want, rejected = mri.split(name)
    mri.check(sdk.model_codec_decode(body, code, rational=True), want, name)
    assert sdk.model_codec_decode(body, code) is None  # 1/3 is no canonical element
    assert len(rejected) == {"float32": 0, "float64": 0, "int32": 18, "int64": 5}[name]
    bad = {str(p): mri.element(*p) for p in rejected}
    bad.update(mri.BAD)
    for label, words in bad.items():
        assert sdk.model_codec_decode(mri.body_of([words]), code, rational=True) is None, label
        framed = mri.body_of([mri.ZERO, words, mri.ONE])
        assert sdk.model_codec_decode(framed, code, rational=True) is None, (name, label)


@pytest.mark.parametrize("name", mci.DTYPES)
def test_random_pairs_of_every_width(name):
    """Up to ten digits a side; the integer types get quotients they hold."""
    qbits = {"int32": 31, "int64": 63}.get(name)
    body, want, rejected = mri.split(name, mri.random_pairs(400, 5, 10, qbits))
    assert not rejected
    mri.check(sdk.model_codec_decode(body, mci.DTYPE_CODE[name], rational=True), want, name)


@pytest.mark.parametrize("name", mci.DTYPES)
def test_canonical_bodies_and_the_cpu_engine(name):
    pytest.importorskip("torch")
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    cfg = _core.mask.MaskConfig(1, 0, 0, 3)
    cpu = CpuPlaneAggregator(cfg, cfg, 16)
    code = mci.DTYPE_CODE[name]
    for label, vec in mci.vectors(name).items():  # elements of up to 34 digits
        body = sdk.encode_model(vec)
        want = sdk.model_codec_decode(body, code)
        mri.check(sdk.model_codec_decode(body, code, rational=True), want, (name, label))
    body, want, _ = mri.split(name)
    mri.check(cpu.decode_model(body, code, rational=True).numpy(), want, name)
    assert cpu.decode_model(body, code) is None
