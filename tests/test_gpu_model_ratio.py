"""K7d's rational mode on the GPU: GpuMaskedAggregator.decode_model(...,
rational=True) (k7d_emit<T, true>) bit for bit against Fraction rounded once,
through every level of the boundary resolve, and ParticipantAccel on top."""
import pytest

torch = pytest.importorskip("torch")

import model_codec_inputs as mci  # noqa: E402
import model_ratio_inputs as mri  # noqa: E402
from xaynet_amd import _core, _hip  # noqa: E402

sdk = _core.sdk
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from xaynet_amd.ops import GpuMaskedAggregator, gpu_available

    if not gpu_available():
        pytest.skip("no MI355X visible")
    cfg = _core.mask.MaskConfig(1, 0, 0, 3)
    return GpuMaskedAggregator(cfg, cfg, 16, device="cuda:0")


def check(t, want, what):
    assert t is not None and t.is_cuda and t.dim() == 1 and t.is_contiguous(), what
    mri.check(t.cpu().numpy(), want, what)


@pytest.mark.parametrize("name", mci.DTYPES)
def test_values_and_rejections(eng, name):
    code = mci.DTYPE_CODE[name]
    body, want, rejected = mri.split(name)
    check(eng.decode_model(body, code, rational=True), want, name)
    assert eng.decode_model(body, code) is None
    bad = {str(p): mri.element(*p) for p in rejected}
    bad.update(mri.BAD)
    for label, words in bad.items():
        assert eng.decode_model(mri.body_of([words]), code, rational=True) is None, (name, label)
    for pair in ((1, 3), (-7, 2)):  # n = 1
        one = mri.split(name, [pair])
        check(eng.decode_model(one[0], code, rational=True), one[1], (name, pair))
    canonical = sdk.encode_model(mci.edges(name))
    check(eng.decode_model(canonical, code, rational=True), sdk.decode_model(canonical, code), name)


@pytest.mark.parametrize("name,qbits", (("float32", None), ("int64", 63)))
def test_more_than_one_workgroup_of_elements(eng, name, qbits):
    body, want, rejected = mri.split(name, mri.random_pairs(257, 9, 10, qbits))
    assert not rejected and len(want) == 257
    check(eng.decode_model(body, mci.DTYPE_CODE[name], rational=True), want, name)


@pytest.mark.parametrize("name", ("float32", "float64"))
def test_every_resolve_level_and_the_block_edges(eng, name):
    """tile_blocks = 2 over a dozen blocks: block maps, tile maps, the walk and
    the replay all run, with an element that starts in a block's last word."""
    code = mci.DTYPE_CODE[name]
    pairs = list(mri.block_edges(_hip._model_decode_plan(1)["block_words"]))
    body, want, _ = mri.split(name, pairs)
    plan = _hip._model_decode_plan((len(body) - 9) // 4, 2)
    assert plan["levels"] == 2 and plan["tiles"] > 2
    check(eng.decode_model(body, code, tile_blocks=2, rational=True), want, name)
    check(eng.decode_model(body, code, rational=True), want, name)
    # one rejected element in the last block
    bad = mri.body_of([mri.element(*p) for p in pairs] + [mri.BAD["Minus denominator"]])
    assert eng.decode_model(bad, code, tile_blocks=2, rational=True) is None
    check(eng.decode_model(body, code, tile_blocks=2, rational=True), want, name)


def test_accelerator_serves_rationals_and_falls_back(eng, monkeypatch):
    from xaynet_amd.ops.accel import ParticipantAccel
    from xaynet_amd.ops.engine import GpuMaskedAggregator

    served = []
    inner = GpuMaskedAggregator.decode_model

    def counting(self, *a, **kw):
        t = inner(self, *a, **kw)
        served.append(t is not None)
        return t

    monkeypatch.setattr(GpuMaskedAggregator, "decode_model", counting)
    accel = ParticipantAccel()
    body, want, _ = mri.split("float32", mri.random_pairs(300, 3))
    check(accel.decode_model(body, 0, rational=True), want, "rational")
    wide = mri.body_of([mri.element(1, 3), mri.BAD["eleven-digit numerator"]])
    check(accel.decode_model(wide, 0, rational=True), sdk.decode_model(wide, 0), "fallback")
    assert served == [True, False]  # the kernels served the first, the CPU decoder the second
