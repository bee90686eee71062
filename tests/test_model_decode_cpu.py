"""The strict model decoder on the host: _core.sdk.model_codec_decode, the
sequential walk over mc_span / mc_read (csrc/gpu/model_codec.h) that the K7d
kernels run in parallel. Held bit for bit against the independent decoder of
message/bincode.cpp (sdk.decode_model) on canonical bodies, and against the
encoder wherever it accepts: an accepted body re-encodes to itself."""
import numpy as np
import pytest

import model_codec_inputs as mci
import model_decode_inputs as mdi
from xaynet_amd import _core

sdk = _core.sdk

UINT = {"float32": np.uint32, "float64": np.uint64, "int32": np.uint32, "int64": np.uint64}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        np.array_equal(a.view(UINT[a.dtype.name]), b.view(UINT[b.dtype.name]))


@pytest.mark.parametrize("name", mci.DTYPES)
def test_equals_the_cpu_decoder_and_reencodes(name):
    code = mci.DTYPE_CODE[name]
    for label, vec in mci.vectors(name).items():
        body = sdk.encode_model(vec)
        got = sdk.model_codec_decode(body, code)
        assert got is not None and got.dtype == np.dtype(name), (name, label)
        assert same_bits(got, sdk.decode_model(body, code)), (name, label)
        assert sdk.model_codec_encode(got) == body, (name, label)


@pytest.mark.parametrize("name", mci.DTYPES)
def test_empty_model(name):
    got = sdk.model_codec_decode(b"\x01" + bytes(8), mci.DTYPE_CODE[name])
    assert got is not None and got.shape == (0,) and got.dtype == np.dtype(name)


@pytest.mark.parametrize("name", mci.DTYPES)
def test_non_canonical_elements_are_rejected(name):
    code = mci.DTYPE_CODE[name]
    for label, (body, rejected) in mdi.element_bodies(name).items():
        got = sdk.model_codec_decode(body, code)
        if rejected:
            assert got is None, (name, label, got)
        else:  # the other dtypes hold the value: the encoder's own bytes
            assert got is not None and sdk.model_codec_encode(got) == body, (name, label)


def test_what_the_cpu_decoder_makes_of_them():
    """The independent decoder is a lenient one: it rounds 1/3, reduces 2/2."""
    bodies = mdi.element_bodies("float32")
    assert sdk.decode_model(bodies["1/3"][0], 0)[1] == np.float32(1 / 3)
    assert sdk.decode_model(bodies["unreduced 2/2"][0], 0)[1] == 1.0
    assert sdk.decode_model(bodies["2^24 + 1"][0], 0)[1] == 16777216.0
    assert sdk.decode_model(bodies["denominator sign 0"][0], 0) is None


def test_int_min_is_an_i32():
    body = mdi.body_of([mdi.ZERO, mdi.INT_MIN32, mdi.ONE])
    got = sdk.model_codec_decode(body, mci.DTYPE_CODE["int32"])
    assert got is not None and got.tolist() == [0, -2**31, 1]
    assert sdk.model_codec_encode(got) == body


@pytest.mark.parametrize("name", mci.DTYPES)
def test_framing_defects_are_rejected(name):
    code = mci.DTYPE_CODE[name]
    good, bad = mdi.framing_bodies(name)
    got = sdk.model_codec_decode(good, code)
    assert got is not None and same_bits(got, sdk.decode_model(good, code))
    for label, body in bad.items():
        assert sdk.model_codec_decode(body, code) is None, (name, label)


def test_the_cpu_decoder_ignores_trailing_words_and_the_head_value():
    good, bad = mdi.framing_bodies("float32")
    for label in ("one zero word more", "head 02"):
        assert sdk.decode_model(bad[label], 0).tolist() == [0.0, 0.5, 1.0]


@pytest.mark.parametrize("name", mci.DTYPES)
def test_corrupted_bodies_decode_only_to_their_own_encoding(name):
    """One word of a valid 50-element body overwritten, 500 cases per dtype
    (2000 in all): whatever the decoder still accepts is a canonical body, the
    encoding of what it returned."""
    code = mci.DTYPE_CODE[name]
    body = sdk.encode_model(mdi.mixed_vector(name, 50))
    assert sdk.model_codec_decode(body, code) is not None
    accepted = 0
    for bad in mdi.corruptions(body, 500, seed=4000 + code):
        got = sdk.model_codec_decode(bad, code)
        if got is not None:
            accepted += 1
            assert sdk.model_codec_encode(got) == bad
    assert accepted < 500  # most single-word changes break the structure


def test_decode_plan_is_consistent():
    """Needs the built extension, no device."""
    _hip = pytest.importorskip("xaynet_amd._hip", reason="_hip extension not built")
    bw = _hip._model_decode_plan(1)["block_words"]
    assert bw >= 64
    default_tile = _hip._model_decode_plan(1)["tile_blocks"]
    for words in (0, 1, 7, bw - 1, bw, bw + 1, 5 * bw + 3, default_tile * bw,
                  default_tile * bw + 1, 25_000_000 * 8):
        for tile in (0, 1, 4, default_tile):
            p = _hip._model_decode_plan(words, tile)
            tb = tile or default_tile
            assert p["block_words"] == bw and p["tile_blocks"] == tb
            assert p["blocks"] == -(-words // bw)
            assert p["tiles"] == -(-p["blocks"] // tb)
            assert p["levels"] == (2 if p["tiles"] > 1 else 1)
            assert p["work_bytes"] >= 16 + 4 * 42 * p["blocks"]
    # a larger tile than the kernels hold in LDS is no plan
    assert _hip._model_decode_plan(7, default_tile + 1)["block_words"] == 0


def test_cpu_engine_decode_model():
    torch = pytest.importorskip("torch")
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    cfg = _core.mask.MaskConfig(1, 0, 0, 3)
    cpu = CpuPlaneAggregator(cfg, cfg, 16)
    for name in mci.DTYPES:
        code = mci.DTYPE_CODE[name]
        body = sdk.encode_model(mci.edges(name))
        t = cpu.decode_model(np.frombuffer(body, dtype=np.uint8), code)
        assert isinstance(t, torch.Tensor) and t.device.type == "cpu"
        assert same_bits(t.numpy(), sdk.decode_model(body, code))
        assert bytes(cpu.encode_model(t)) == body
        assert cpu.decode_model(mdi.element_bodies(name)["1/3"][0], code) is None
    arr = np.frombuffer(body + bytes(3), dtype=np.uint8)
    for bad in (arr[::2], arr.reshape(4, -1), 7):
        with pytest.raises(ValueError):
            cpu.decode_model(bad, 0)
