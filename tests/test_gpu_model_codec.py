"""K7 on the GPU: GpuMaskedAggregator.encode_model against the CPU encoder,
byte for byte, over the shared inputs at every block-boundary length, at
lengths that run each level of the block-total scan, and through a staged
round of the coordinator driver."""
import time
from functools import lru_cache

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import model_codec_inputs as mci  # noqa: E402
from xaynet_amd import _core, _hip  # noqa: E402

co = _core.coordinator
sdk = _core.sdk
mk = _core.mask

pytestmark = pytest.mark.gpu

HEAD0 = b"\x01" + bytes(8)  # Some, zero elements


@pytest.fixture(scope="module")
def eng():
    from xaynet_amd.ops import GpuMaskedAggregator, gpu_available

    if not gpu_available():
        pytest.skip("no MI355X visible")
    cfg = mk.MaskConfig(1, 0, 0, 3)
    return GpuMaskedAggregator(cfg, cfg, 16, device="cuda:0")


@lru_cache(maxsize=None)
def reference(name, label, n):
    """(input, CPU body) of vector `label` tiled to n elements."""
    arr = mci.tiled(mci.vectors(name)[label], n)
    arr.setflags(write=False)
    return arr, sdk.encode_model(arr)


def gpu_body(eng, arr):
    return bytes(eng.encode_model(torch.from_numpy(np.array(arr)).to("cuda:0")))


@pytest.mark.parametrize("name", mci.DTYPES)
def test_block_boundary_lengths(eng, name):
    B = _hip._model_plan(1)["block_elems"]
    assert B >= 64
    for label in ("edges", "random", "heavy"):
        for n in (1, B - 1, B, B + 1, 3 * B + 7):
            arr, want = reference(name, label, n)
            assert gpu_body(eng, arr) == want, (name, label, n)


@pytest.mark.parametrize("name", mci.DTYPES)
def test_whole_vectors(eng, name):
    """Every element of the edge, random and heavy-tail vectors."""
    for label, vec in mci.vectors(name).items():
        arr, want = reference(name, label, len(vec))
        assert gpu_body(eng, arr) == want, (name, label)


def test_scan_runs_every_level(eng):
    """2^20 + 17 f32 weights are 4097 blocks, one more than a single scan
    workgroup takes: the block totals are scanned inside 5 tiles of 1024
    blocks, and the tile totals, which differ widely under the heavy-tail mix,
    by the base scan. Every block past the first tile needs a non-zero tile
    base and an in-tile prefix, so both levels show in the bytes."""
    n = 2**20 + 17
    plan = _hip._model_plan(n)
    assert plan["scan_levels"] == 2 and plan["tiles"] > 1
    arr, want = reference("float32", "heavy", n)
    assert gpu_body(eng, arr) == want


def test_one_level_scan_carries_across_chunks(eng):
    """1025 blocks stay one level, but the single scan workgroup takes them in
    two chunks of 1024 with a carry; f64 gives the largest block totals."""
    B = _hip._model_plan(1)["block_elems"]
    n = 1025 * B + 3
    plan = _hip._model_plan(n)
    assert plan["scan_levels"] == 1 and plan["blocks"] == 1026
    arr, want = reference("float64", "heavy", n)
    assert gpu_body(eng, arr) == want


def test_length_zero(eng):
    for dt in (torch.float32, torch.float64, torch.int32, torch.int64):
        assert bytes(eng.encode_model(torch.empty(0, dtype=dt, device="cuda:0"))) == HEAD0


def test_shorter_call_after_a_long_one(eng):
    long_arr, long_want = reference("float64", "heavy", 5000)
    short_arr, short_want = reference("float32", "random", 300)
    assert gpu_body(eng, long_arr) == long_want
    out = eng.encode_model(torch.from_numpy(np.array(short_arr)).to("cuda:0"))
    assert out.dtype == np.uint8 and out.shape == (len(short_want),)
    assert bytes(out) == short_want


def test_small_buffer_is_left_untouched(eng):
    """_model_encode returns the body length and writes nothing when the
    buffer is a byte short; with the exact size it writes the body at byte 3."""
    arr, want = reference("float32", "edges", 700)
    w = torch.from_numpy(np.array(arr)).to("cuda:0")
    work = torch.empty(_hip._model_plan(700)["work_bytes"], dtype=torch.uint8, device="cuda:0")
    out = torch.full((3 + len(want) + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")
    assert _hip._model_encode(w.data_ptr(), 0, 700, work.data_ptr(), out.data_ptr(),
                              3 + len(want) - 1) == len(want)
    assert bool((out == 0xAB).all())
    assert _hip._model_encode(w.data_ptr(), 0, 700, work.data_ptr(), out.data_ptr(),
                              3 + len(want)) == len(want)
    host = out.cpu().numpy()
    assert bytes(host[3:3 + len(want)]) == want
    assert (host[3 + len(want):] == 0xAB).all() and (host[:3] == 0xAB).all()


def test_rejected_inputs(eng, monkeypatch):
    from xaynet_amd.ops import engine as engine_mod

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(engine_mod._hip, "_model_encode", no_launch)
    dev = torch.zeros(64, dtype=torch.float32, device="cuda:0")
    for bad in (dev[::2],                                   # strided view
                torch.zeros(64, dtype=torch.float32),       # CPU tensor
                dev.to(torch.float16),                      # f16
                dev.reshape(8, 8)):                         # 2-D
        with pytest.raises(ValueError):
            eng.encode_model(bad)


def test_cpu_engine_gives_the_same_bytes(eng):
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    cfg = mk.MaskConfig(1, 0, 0, 3)
    cpu = CpuPlaneAggregator(cfg, cfg, 16)
    for name in mci.DTYPES:
        arr, want = reference(name, "edges", 777)
        t = torch.from_numpy(np.array(arr))
        assert bytes(cpu.encode_model(t)) == want == bytes(eng.encode_model(t.to("cuda:0")))
    with pytest.raises(ValueError):
        cpu.encode_model(torch.zeros(8, dtype=torch.float16))


def test_driver_round_publishes_the_gpu_body():
    """One staged round through GpuCoordinatorDriver: the published body is
    the encoding of its own decoded weights, and it came from the engine's
    encode_model."""
    from xaynet_amd.ops import gpu_available, make_coordinator_driver

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
    calls = []
    inner = driver.eng.encode_model

    def counting(weights):
        calls.append(weights.numel())
        return inner(weights)

    driver.eng.encode_model = counting
    driver.start()
    client = sdk.InProcessClient(coord)
    rng = np.random.default_rng(29)
    participants = [sdk.Participant(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), 1, 1, client)
                    for _ in range(n)]
    weights = [rng.uniform(-1, 1, length).astype(np.float32) for _ in range(n)]
    coord.start()
    t0 = time.time()
    body = None
    try:
        while time.time() - t0 < 60.0 and body is None:
            for i, p in enumerate(participants):
                p.tick()
                if p.should_set_model:
                    p.set_model(weights[i])
            got = coord.fetch_model()
            if got and got[0] == 1:
                body = bytes(got)
            time.sleep(0.002)
    finally:
        coord.stop()
        driver.stop()
    assert body is not None, "no global model published"
    assert driver.rounds_unmasked >= 1 and calls and calls[-1] == length
    model = np.asarray(sdk.decode_model(body, 0))
    assert model.shape == (length,) and np.abs(model).max() <= 1.0 + 1e-5
    assert np.abs(model).mean() > 1e-3
    assert sdk.encode_model(model) == body
