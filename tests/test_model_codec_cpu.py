"""The GPU model encoder's element functions (csrc/gpu/model_codec.h) on the
host, against the CPU encoder of message/bincode.cpp: byte equality, over the
shared inputs and over raw bit patterns. Needs no GPU."""
import time

import numpy as np
import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

import model_codec_inputs as mci
from xaynet_amd import _core

sdk = _core.sdk
co = _core.coordinator
mk = _core.mask

CASES = [(name, label) for name in mci.DTYPES for label in ("edges", "random", "heavy")]


def _check(arr):
    ref = sdk.encode_model(arr)
    body = sdk.model_codec_encode(arr)
    assert body == ref
    words = sdk.model_codec_words(arr)
    assert words.dtype == np.uint32 and words.shape == arr.shape
    assert 4 * int(words.sum(dtype=np.uint64)) == len(body) - 9
    return body, words


@pytest.mark.parametrize("name,label", CASES)
def test_codec_equals_cpu_encoder(name, label):
    arr = mci.vectors(name)[label]
    body, words = _check(arr)
    # the generic rational path reads the same elements back and writes them
    # again, unchanged
    assert sdk.reencode_model_slow(body) == body
    # per-element counts: every prefix of the vector encodes to the bytes the
    # counts say
    for cut in (1, 2, len(arr) // 2):
        assert len(sdk.encode_model(arr[:cut])) == 9 + 4 * int(words[:cut].sum())


# Element sizes in u32 words, worked out by hand from write_dyadic.
def test_element_sizes():
    f32, f64 = np.float32, np.float64
    least_full32 = np.array([0x00FFFFFF], dtype=np.uint32).view(f32)[0]
    least_full64 = np.array([0x001FFFFFFFFFFFFF], dtype=np.uint64).view(f64)[0]
    for arr, want in [
        (np.array([0.0, -0.0, np.nan, np.inf, -np.inf], dtype=f32), [7] * 5),
        (np.array([0.5, -0.75, 1.0, 3.0], dtype=f32), [8, 8, 8, 8]),
        (np.array([least_full32, np.finfo(f32).max], dtype=f32), [12, 11]),
        (np.array([least_full64, np.finfo(f64).max, 0.0], dtype=f64), [42, 39, 7]),
        (np.array([0, 1, -1, 2**31 - 1, -(2**31)], dtype=np.int32), [7, 8, 8, 8, 8]),
        (np.array([0, 2**63 - 1, -(2**63), 2**32], dtype=np.int64), [7, 9, 9, 9]),
    ]:
        assert sdk.model_codec_words(arr).tolist() == want
        _check(arr)
    # the mean over U(-1, 1) f32 weights is 8 words
    u = np.random.default_rng(5).uniform(-1, 1, 20000).astype(f32)
    assert abs(float(sdk.model_codec_words(u).mean()) - 8.0) < 0.01


def test_empty_and_shape_errors():
    for name in mci.DTYPES:
        empty = np.zeros(0, dtype=name)
        assert sdk.model_codec_encode(empty) == sdk.encode_model(empty) == b"\x01" + bytes(8)
        assert sdk.model_codec_words(empty).shape == (0,)
    with pytest.raises(ValueError):
        sdk.model_codec_encode(np.zeros((2, 2), dtype=np.float32))
    with pytest.raises(ValueError):
        sdk.model_codec_words(np.zeros(3, dtype=np.float16))


@settings(max_examples=200, deadline=None)
@given(st.lists(st.integers(0, 2**32 - 1), min_size=1, max_size=64))
def test_f32_bit_patterns(bits):
    _check(np.array(bits, dtype=np.uint32).view(np.float32))


@settings(max_examples=200, deadline=None)
@given(st.lists(st.integers(0, 2**64 - 1), min_size=1, max_size=64))
def test_f64_bit_patterns(bits):
    _check(np.array(bits, dtype=np.uint64).view(np.float64))


@settings(max_examples=100, deadline=None)
@given(st.lists(st.integers(-(2**63), 2**63 - 1), min_size=1, max_size=64))
def test_int_values(vals):
    _check(np.array(vals, dtype=np.int64))
    _check(np.array(vals, dtype=np.int64).astype(np.int32))


def test_plan_levels():
    """The plan the K7 launcher uses: blocks, scan levels, workspace."""
    _hip = pytest.importorskip("xaynet_amd._hip", reason="_hip extension not built")
    one = _hip._model_plan(1)
    B = one["block_elems"]
    assert one["blocks"] == 1 and one["scan_levels"] == 1 and one["tiles"] == 0
    zero = _hip._model_plan(0)
    assert zero["blocks"] == 0 and zero["work_bytes"] == 0
    # the last length of one level and the first of two
    edge = _hip._model_plan(1)["block_elems"] * 4096
    assert _hip._model_plan(edge)["scan_levels"] == 1
    two = _hip._model_plan(edge + 1)
    assert two["scan_levels"] == 2 and two["blocks"] == 4097
    assert two["tiles"] == -(-two["blocks"] // two["tile_blocks"]) == 5
    for n in (1, B, edge, edge + 1, 2**32):
        p = _hip._model_plan(n)
        assert p["blocks"] == -(-n // B)
        bases = p["tiles"] if p["scan_levels"] == 2 else p["blocks"]
        assert p["work_bytes"] >= 8 + 8 * bases + 4 * p["blocks"] + 4 * p["tiles"]
    # length 0 launches nothing and needs no device
    assert _hip._model_encode(0, 0, 0, 0, 0, 0) == 9
    with pytest.raises(ValueError):
        _hip._model_encode(0, 4, 0, 0, 0, 0)


def _staged_coordinator(length):
    s = co.Settings()
    s.sum_prob = 0.5
    s.update_prob = 1.0
    s.model_length = length
    c = mk.MaskConfig(1, 0, 0, 3)
    s.mask_cfg = mk.MaskConfigPair(c, c)
    s.set_sum(1, 100, 0.05, 10.0)
    s.set_update(3, 100, 0.05, 10.0)
    s.set_sum2(1, 100, 0.05, 10.0)
    return co.Coordinator(s, co.InMemoryStorage(), co.InMemoryModels(), True)


def test_supply_unmasked_model_buffer_forms():
    """bytes, a bytearray, a memoryview and an unaligned uint8 array view (what
    the GPU engine's encode_model returns) are accepted; a strided view and a
    str are not."""
    body = sdk.encode_model(np.linspace(-1, 1, 64, dtype=np.float32))
    padded = np.frombuffer(b"\0\0\0" + body, dtype=np.uint8)
    coord = _staged_coordinator(64)
    coord.supply_unmasked_model(body)
    coord.supply_unmasked_model(memoryview(body))
    coord.supply_unmasked_model(bytearray(body))
    coord.supply_unmasked_model(padded[3:])
    with pytest.raises(BufferError):
        coord.supply_unmasked_model(memoryview(padded)[::2])
    with pytest.raises(TypeError):
        coord.supply_unmasked_model("not bytes")


def test_supplied_views_publish_the_same_model():
    """Staged rounds whose unmask plane supplies the body as bytes, as a
    memoryview and as an array view from byte 3 of a buffer: the coordinator
    publishes exactly the supplied bytes each time."""
    length, n = 64, 12
    forms = [bytes, memoryview,
             lambda b: np.frombuffer(b"\0\0\0" + b, dtype=np.uint8)[3:]]
    bodies = [sdk.encode_model(np.full(length, (k + 1) / 8, dtype=np.float32))
              for k in range(len(forms))]
    coord = _staged_coordinator(length)
    client = sdk.InProcessClient(coord)
    rng = np.random.default_rng(41)
    participants = [sdk.Participant(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), 1, 1, client)
                    for _ in range(n)]
    weights = rng.uniform(-1, 1, length).astype(np.float32)
    published, supplied_round = [], -1
    coord.start()
    t0 = time.time()
    try:
        while time.time() - t0 < 60.0 and len(published) < len(forms):
            for p in participants:
                p.tick()
                if p.should_set_model:
                    p.set_model(weights)
            coord.drain_staged_updates()
            k = len(published)
            if coord.pending_unmask() is not None and coord.round_id != supplied_round:
                supplied_round = coord.round_id
                coord.supply_unmasked_model(forms[k](bodies[k]))
            got = coord.fetch_model()
            if got and bytes(got) == bodies[k]:
                published.append(bytes(got))
            time.sleep(0.002)
    finally:
        coord.stop()
    assert published == bodies
