"""K7d on the GPU: GpuMaskedAggregator.decode_model against the CPU decoder
(sdk.decode_model) bit for bit on canonical bodies, and against the host walk
over the same element functions (sdk.model_codec_decode) in its verdict on
everything else: elements straddling every block boundary offset, every level
of the boundary resolve, rejected and corrupted bodies, the participant
accelerator and one staged round through the SDK wrapper."""
import struct
import time
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import model_codec_inputs as mci  # noqa: E402
import model_decode_inputs as mdi  # noqa: E402
from xaynet_amd import _core, _hip  # noqa: E402

co = _core.coordinator
sdk = _core.sdk
mk = _core.mask

pytestmark = pytest.mark.gpu

UINT = {"float32": np.uint32, "float64": np.uint64, "int32": np.uint32, "int64": np.uint64}
LONGEST_BITS = {"float64": (1 << 52) | ((1 << 52) - 1), "float32": (1 << 23) | ((1 << 23) - 1)}
LONGEST_WORDS = {"float64": 42, "float32": 12}


@pytest.fixture(scope="module")
def eng():
    from xaynet_amd.ops import GpuMaskedAggregator, gpu_available

    if not gpu_available():
        pytest.skip("no MI355X visible")
    cfg = mk.MaskConfig(1, 0, 0, 3)
    return GpuMaskedAggregator(cfg, cfg, 16, device="cuda:0")


def bits(a):
    return a.view(UINT[a.dtype.name])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def decode(eng, body, name, **kw):
    """eng.decode_model as a host array, or None."""
    t = eng.decode_model(body, mci.DTYPE_CODE[name], **kw)
    if t is None:
        return None
    assert t.is_cuda and t.dim() == 1 and t.is_contiguous()
    return t.cpu().numpy()


@lru_cache(maxsize=None)
def reference(name, label, n):
    """(CPU body, CPU-decoded weights) of vector `label` tiled to n elements."""
    body = sdk.encode_model(mci.tiled(mci.vectors(name)[label], n))
    want = sdk.decode_model(body, mci.DTYPE_CODE[name])
    want.setflags(write=False)
    return body, want


def raw_status(body, name, n=None, nbytes=None, extra=b""):
    """_hip._model_decode on buffers of its own: the body at byte 3 of a device
    buffer, `extra` behind it, `nbytes` of it declared."""
    nbytes = len(body) if nbytes is None else nbytes
    if n is None:
        n = struct.unpack("<Q", body[1:9])[0] if len(body) >= 9 else 0
    host = np.zeros((3 + len(body) + len(extra) + 3) // 4 * 4 + 64, dtype=np.uint8)
    host[3:3 + len(body)] = np.frombuffer(body, dtype=np.uint8)
    host[3 + len(body):3 + len(body) + len(extra)] = np.frombuffer(extra, dtype=np.uint8)
    dev = torch.from_numpy(host).to("cuda:0")
    plan = _hip._model_decode_plan(max(nbytes - 9, 0) // 4)
    work = torch.empty(max(plan["work_bytes"], 16), dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(max(n, 1) if n < 2**20 else 1, dtype=torch.int64, device="cuda:0")
    status = _hip._model_decode(dev.data_ptr() + 3, nbytes, mci.DTYPE_CODE[name], n,
                                work.data_ptr(), out.data_ptr())
    return status, out.cpu().numpy().view(name)[:n] if n < 2**20 else None


@pytest.mark.parametrize("name", mci.DTYPES)
def test_whole_vectors(eng, name):
    for label, vec in mci.vectors(name).items():
        body, want = reference(name, label, len(vec))
        got = eng.decode_model(body, mci.DTYPE_CODE[name])
        assert got is not None, (name, label)
        assert same_bits(got.cpu().numpy(), want), (name, label)
        assert bytes(eng.encode_model(got)) == body, (name, label)


def straddle_values(name, bw, k):
    """Weights whose body has the type's longest element start k words before
    the first block boundary and again k words before the second, 20 mixed
    elements in between, and 7- and 8-word elements everywhere else."""
    longest = np.array([LONGEST_BITS[name]], dtype=UINT[name]).view(name)
    assert int(sdk.model_codec_words(longest)[0]) == LONGEST_WORDS[name]

    def filler(total):  # 7a + 8b words of zeros, ones and halves
        b = total % 7
        a = (total - 8 * b) // 7
        assert a >= 0
        v = np.zeros(a + b, dtype=name)
        v[a:] = np.resize(np.array([1.0, 0.5], dtype=name), b)
        return v

    mixed = np.array(mdi.mixed_vector(name, 20, seed=k))
    used = bw - k + LONGEST_WORDS[name] + int(sdk.model_codec_words(mixed).sum())
    v = np.concatenate([filler(bw - k), longest, mixed, filler(2 * bw - k - used), longest,
                        mixed[:3]])
    starts = np.concatenate([[0], np.cumsum(sdk.model_codec_words(v))])
    at = len(filler(bw - k))
    assert starts[at] == bw - k and 2 * bw - k in starts
    return v


@pytest.mark.parametrize("name", ("float64", "float32"))
def test_every_straddle(eng, name):
    """k = the element's length ends it exactly on the boundary; k = 1 leaves
    all but its first word to the next block."""
    bw = _hip._model_decode_plan(1)["block_words"]
    for k in range(1, LONGEST_WORDS[name] + 1):
        body = sdk.encode_model(straddle_values(name, bw, k))
        want = sdk.decode_model(body, mci.DTYPE_CODE[name])
        got = decode(eng, body, name)
        assert got is not None and same_bits(got, want), (name, k)


def test_every_resolve_level_at_small_size(eng):
    """tile_blocks = 4 makes a body of 3 * block_words elements run the tile
    maps, the walk over the tiles and the replay; so do bodies of exactly 1, 2,
    4 and 5 blocks, on either side of the one-tile case."""
    bw = _hip._model_decode_plan(1)["block_words"]
    tile = 4
    for name in ("float32", "float64"):
        body, want = reference(name, "heavy", 3 * bw)
        plan = _hip._model_decode_plan((len(body) - 9) // 4, tile)
        assert plan["levels"] == 2 and plan["tiles"] > 2
        assert _hip._model_decode_plan((len(body) - 9) // 4)["levels"] == 1
        small = decode(eng, body, name, tile_blocks=tile)
        default = decode(eng, body, name)
        assert small is not None and same_bits(small, want) and same_bits(default, want)
    heavy = mci.tiled(mci.heavy_tail("float64"), 6 * bw)
    ends = np.cumsum(sdk.model_codec_words(heavy))
    for blocks in (1, 2, tile, tile + 1):
        n = int(np.searchsorted(ends, blocks * bw, side="right"))  # the most that fit
        body = sdk.encode_model(heavy[:n])
        plan = _hip._model_decode_plan((len(body) - 9) // 4, tile)
        assert plan["blocks"] == blocks and plan["levels"] == (2 if blocks > tile else 1)
        got = decode(eng, body, "float64", tile_blocks=tile)
        assert got is not None and same_bits(got, sdk.decode_model(body, 1)), blocks


def test_one_natural_multi_tile_body(eng):
    n = 2**20 + 17
    body, want = reference("float32", "heavy", n)
    plan = _hip._model_decode_plan((len(body) - 9) // 4)
    assert plan["tiles"] > 1 and plan["levels"] == 2
    got = decode(eng, body, "float32")
    assert got is not None and same_bits(got, want)


@pytest.mark.parametrize("name", mci.DTYPES)
def test_rejections(eng, name):
    good, framing = mdi.framing_bodies(name)
    cases = {label: (body, True) for label, body in framing.items()}
    cases.update(mdi.element_bodies(name))
    cases["valid"] = (good, False)
    for label, (body, rejected) in cases.items():
        status, out = raw_status(body, name)
        got = decode(eng, body, name)
        want = sdk.model_codec_decode(body, mci.DTYPE_CODE[name])
        assert (want is None) == rejected, (name, label)
        if rejected:
            assert status != 0 and got is None, (name, label)
        else:
            assert status == 0 and same_bits(got, want) and same_bits(out, want), (name, label)


def test_decode_after_reject(eng):
    body, want = reference("float64", "random", 3000)
    bad = bytearray(body)
    bad[9 + 4 * 1000 + 4: 9 + 4 * 1000 + 8] = struct.pack("<I", 2**32 - 1)  # some count or digit
    if sdk.model_codec_decode(bytes(bad), 1) is not None:
        bad = bytearray(body[:-4])
    assert decode(eng, bytes(bad), "float64") is None
    assert same_bits(decode(eng, body, "float64"), want)
    assert decode(eng, mdi.element_bodies("float64")["1/3"][0], "float64") is None
    assert same_bits(decode(eng, body, "float64"), want)


def test_length_is_what_counts_not_memory():
    from xaynet_amd.ops import gpu_available

    if not gpu_available():
        pytest.skip("no MI355X visible")
    body, want = reference("float32", "random", 700)
    # behind the body, in the same device buffer: words that go on like elements
    extra = np.array([2, 1, 0, 5, 2, 1, 0, 1] * 8, dtype="<u4").tobytes()
    status, out = raw_status(body, "float32", extra=extra)
    assert status == 0 and same_bits(out, want)
    # cut in the middle of the last element, whose rest is physically there
    status, _ = raw_status(body, "float32", nbytes=len(body) - 8, extra=extra)
    assert status != 0
    # and the words behind do not become elements when the count asks for one more
    status, _ = raw_status(body, "float32", n=701, extra=extra)
    assert status != 0


def test_device_equals_host_on_garbage(eng):
    """200 single-word corruptions of a 300-element f64 body (several blocks):
    the kernels' verdict is the host walk's, and so are the values. A hang
    here is a defect of the chain bound."""
    body = sdk.encode_model(mdi.mixed_vector("float64", 300))
    bw = _hip._model_decode_plan(1)["block_words"]
    assert (len(body) - 9) // 4 > 2 * bw
    accepted = 0
    for i, bad in enumerate(mdi.corruptions(body, 200, seed=515)):
        want = sdk.model_codec_decode(bad, 1)
        got = decode(eng, bad, "float64", tile_blocks=(0, 1, 2)[i % 3])
        assert (got is None) == (want is None), i
        if want is not None:
            accepted += 1
            assert same_bits(got, want), i
    assert 0 < accepted < 200


def test_lengths_zero_and_one_and_shorter_after_longer(eng):
    long_body, long_want = reference("float64", "heavy", 5000)
    assert same_bits(decode(eng, long_body, "float64"), long_want)
    for name in mci.DTYPES:
        empty = eng.decode_model(b"\x01" + bytes(8), mci.DTYPE_CODE[name])
        assert empty.is_cuda and empty.shape == (0,) and empty.cpu().numpy().dtype == name
        one = np.array([-3], dtype=name)
        got = decode(eng, sdk.encode_model(one), name)
        assert got is not None and same_bits(got, one)
    assert decode(eng, b"\x01" + bytes(7) + b"\x01", "float32") is None  # n = 2^56, no elements
    short_body, short_want = reference("float32", "random", 300)
    assert same_bits(decode(eng, short_body, "float32"), short_want)


def test_rejected_inputs(eng, monkeypatch):
    from xaynet_amd.ops import engine as engine_mod

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(engine_mod._hip, "_model_decode", no_launch)
    body, _ = reference("float32", "random", 300)
    arr = np.frombuffer(body + bytes(3), dtype=np.uint8)
    for bad in (arr[::2], arr.reshape(4, -1), 7, None):
        with pytest.raises(ValueError):
            eng.decode_model(bad, 0)
    with pytest.raises(ValueError):
        eng.decode_model(body, 4)


def test_accelerator_equals_the_cpu_decoder_on_every_body(eng):
    """The values of sdk.decode_model on the device, None where it gives
    None: the kernels serve the canonical bodies, the CPU decoder the rest."""
    from xaynet_amd.ops.accel import ParticipantAccel
    from xaynet_amd.ops.engine import GpuMaskedAggregator

    accel = ParticipantAccel()
    served = []
    inner = GpuMaskedAggregator.decode_model

    def counting(self, body, dtype, tile_blocks=0):
        t = inner(self, body, dtype, tile_blocks)
        served.append(t is not None)
        return t

    GpuMaskedAggregator.decode_model = counting
    try:
        for name in mci.DTYPES:
            code = mci.DTYPE_CODE[name]
            good, framing = mdi.framing_bodies(name)
            bodies = {label: reference(name, label, 777)[0] for label in ("edges", "heavy")}
            canonical = len(bodies) + 1
            bodies["valid"] = good
            bodies.update(framing)
            bodies.update({k: b for k, (b, _) in mdi.element_bodies(name).items()})
            before = sum(served)
            for label, body in bodies.items():
                want = sdk.decode_model(body, code)
                got = accel.decode_model(body, code)
                if want is None:
                    assert got is None, (name, label)
                else:
                    assert got.is_cuda and same_bits(got.cpu().numpy(), want), (name, label)
            assert sum(served) - before >= canonical
    finally:
        GpuMaskedAggregator.decode_model = inner


def test_staged_round_hands_out_a_device_tensor(monkeypatch):
    """One staged round, three gpu=True SDK participants among the twelve:
    global_model_tensor() is the fetched body decoded by the kernels, and
    global_model() is still the list."""
    import xaynet_sdk.xaynet_sdk as wrapper
    from xaynet_amd.ops import gpu_available, make_coordinator_driver
    from xaynet_amd.ops.engine import GpuMaskedAggregator

    if not gpu_available():
        pytest.skip("no MI355X visible")
    n, length = 12, 3001
    s = co.Settings()
    s.sum_prob = 0.5
    s.update_prob = 1.0
    s.model_length = length
    c = mk.MaskConfig(1, 0, 0, 3)  # Prime/F32/B0/M3
    s.mask_cfg = mk.MaskConfigPair(c, c)
    s.set_sum(1, 100, 0.05, 10.0)
    s.set_update(3, 100, 0.05, 10.0)
    s.set_sum2(1, 100, 0.05, 10.0)
    coord = co.Coordinator(s, co.InMemoryStorage(), co.InMemoryModels(), True)  # staged
    driver = make_coordinator_driver(coord, c, c, length, pool_size=8)
    driver.start()
    client = sdk.InProcessClient(coord)
    rng = np.random.default_rng(31)
    gpu_parts = [wrapper.Participant("in-process", 1.0, None, gpu=True, client=client)
                 for _ in range(3)]
    inners = [p._inner for p in gpu_parts]
    inners += [sdk.Participant(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), 1, 1, client)
               for _ in range(n - 3)]
    weights = [rng.uniform(-1, 1, length).astype(np.float32) for _ in range(n)]
    coord.start()
    t0 = time.time()
    body = None
    calls = []
    inner_decode = GpuMaskedAggregator.decode_model

    def counting(self, b, dtype, tile_blocks=0):
        t = inner_decode(self, b, dtype, tile_blocks)
        calls.append(t is not None)
        return t

    try:
        while time.time() - t0 < 60.0 and body is None:
            for i, p in enumerate(inners):
                p.tick()
                if p.should_set_model:
                    p.set_model(weights[i])
            got = coord.fetch_model()
            if got and got[0] == 1:
                body = bytes(got)
            time.sleep(0.002)
        assert body is not None, "no global model published"
        # nobody ticks from here on: the published model stays this round's
        monkeypatch.setattr(GpuMaskedAggregator, "decode_model", counting)
        for p in gpu_parts:
            fetched = p._inner.global_model_bincode()
            assert fetched is not None and bytes(fetched) == body
            want = sdk.decode_model(fetched, 0)
            t = p.global_model_tensor()
            assert t.is_cuda and t.dtype == torch.float32 and t.shape == (length,)
            assert same_bits(t.cpu().numpy(), want)
            assert p.global_model() == want.tolist()
    finally:
        coord.stop()
        driver.stop()
    assert calls == [True, True, True]  # the kernel path served every one
