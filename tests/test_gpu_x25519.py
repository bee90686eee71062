"""K9, batched X25519 and the sealed-box key agreement on the GPU, against
RFC 7748 in plain integers (x25519_ref.py) and the CPU box. Every comparison
is byte equality."""
import time

import numpy as np
import pytest
import torch
from x25519_ref import ORDER8, pairs, x25519

from xaynet_amd import _core
from xaynet_amd.ops import GpuBox, gpu_available

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not gpu_available(), reason="needs an AMD GPU"),
]

crypto = _core.crypto
TILE0 = 16384 - 32  # message bytes in a box's first tile
LENS = [0, 1, 32, 33, TILE0, TILE0 + 16384 + 1]
PK, SK = crypto.box_seed_keypair(b"\x21" * 32)
LOW = ORDER8[0].to_bytes(32, "little")


@pytest.fixture(scope="module")
def box():
    return GpuBox("cuda:0")


@pytest.fixture(scope="module")
def ladders():
    batch = pairs(257)
    return batch, [x25519(s, u) for s, u in batch]


def host(t):
    return bytes(t.cpu().numpy())


def rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# one lane, the wave seam and the workgroup seam (a workgroup is one wave)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257])
def test_x25519_batch_against_the_integer_ladder(box, ladders, n):
    batch, want = ladders
    assert box.x25519_batch([s for s, _ in batch[:n]], [u for _, u in batch[:n]]) == want[:n]


def test_x25519_batch_base_point(box, ladders):
    scalars = [s for s, _ in ladders[0][40:75]]
    assert box.x25519_batch(scalars) == [crypto.x25519_base(s) for s in scalars]


def test_sealbox_open_with_device_keys(box):
    rng = np.random.default_rng(19)
    msgs = [rand(rng, n) for n in LENS]
    sealed = [crypto.sealbox_seal(m, PK) for m in msgs]
    sealed[2] = torch.frombuffer(bytearray(sealed[2]), dtype=torch.uint8).to("cuda:0")
    # a low-order ephemeral key: the shared secret is zero, and a tag made
    # under the key of that secret is valid
    low = LOW + crypto.secretbox_seal(b"low order", crypto.blake2b(LOW + PK, 24),
                                      crypto.box_beforenm(LOW, SK))
    assert crypto.sealbox_open(low, PK, SK) == b"low order"
    flipped = bytearray(crypto.sealbox_seal(msgs[3], PK))
    flipped[5] ^= 1  # a bit of the ephemeral key
    sealed += [low, b"\x01" * 47, bytes(flipped)]
    want = msgs + [b"low order", None, None]
    opened, ok = box.sealbox_open_batch(sealed, PK, SK, device_keys=True)
    assert [None if t is None else host(t) for t in opened] == want
    assert ok.tolist() == [w is not None for w in want]
    assert box.opened_offsets[-2] is None  # shorter than epk || tag: never packed
    off = box.opened_offsets[-1]
    assert host(box.opened_buffer[off:off + len(msgs[3])]) == bytes(len(msgs[3]))


@pytest.mark.parametrize("per_message", [False, True])
def test_sealbox_seal_with_device_keys(box, per_message):
    rng = np.random.default_rng(23)
    msgs = [rand(rng, n) for n in LENS]
    keys = [crypto.box_seed_keypair(bytes([i]) * 32) for i in range(len(msgs))]
    if not per_message:
        keys = [(PK, SK)] * len(msgs)
    pk = [k[0] for k in keys] if per_message else PK
    sealed = [host(t) for t in box.sealbox_seal_batch(msgs, pk, device_keys=True)]
    assert [crypto.sealbox_open(s, *k) for s, k in zip(sealed, keys)] == msgs
    assert len({s[:32] for s in sealed}) == len(sealed)  # a fresh ephemeral key a box


def test_seed_dicts(box, monkeypatch):
    monkeypatch.setattr(GpuBox, "SEEDS_MIN_BATCH", 0)
    rng = np.random.default_rng(29)
    seeds = [rand(rng, 32) for _ in range(257)]
    enc = [bytearray(crypto.sealbox_seal(s, PK)) for s in seeds]
    forged = {0: 31, 64: 40, 256: 79}  # an epk bit, a tag bit, the last cipher byte
    for i, at in forged.items():
        enc[i][at] ^= 1
    want = [None if i in forged else s for i, s in enumerate(seeds)]
    assert box.open_seeds(enc, PK, SK) == want
    keys = [crypto.box_seed_keypair(bytes([i]) * 32) for i in range(65)]
    boxes = box.seal_seed(seeds[1], [k[0] for k in keys])
    assert [len(b) for b in boxes] == [80] * 65
    assert [crypto.sealbox_open(b, *k) for b, k in zip(boxes, keys)] == [seeds[1]] * 65


def test_full_round_with_gpu_seeds(monkeypatch):
    """A round of participants with the hooks that attach() installs; the spies
    forward to them. Every sum participant is saved as its sum2 step begins, and
    a CPU participant (no accelerator) restored from that state is fed the same
    round parameters and seed dict: it opens the same seeds in the same order,
    and the GPU participant's Sum2 mask is, byte for byte, the CPU aggregation
    of the masks of those seeds, which is what the CPU participant sends."""
    from xaynet_amd.ops.accel import ParticipantAccel

    co, mk, sdk = _core.coordinator, _core.mask, _core.sdk
    monkeypatch.setattr(GpuBox, "SEEDS_MIN_BATCH", 0)
    n, length = 10, 1000
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
    rng = np.random.default_rng(41)
    accel = ParticipantAccel(gpu_seeds=True)
    seen = {"open_seeds": [], "seal_seed": [], "aggregate_masks": []}
    for name, calls in seen.items():
        def spy(*args, inner=getattr(accel, name), calls=calls):
            calls.append((args, inner(*args)))
            return calls[-1][1]
        setattr(accel, name, spy)

    sign_seeds = [rand(rng, 32) for _ in range(n)]
    participants = [sdk.Participant(seed, 1, 1, client) for seed in sign_seeds]
    for p in participants:
        accel.attach(p)
    weights = [rng.uniform(-1, 1, length).astype(np.float32) for _ in range(n)]

    coord.start()
    t0 = time.time()
    model, saved = None, []
    try:
        while time.time() - t0 < 60.0 and model is None:
            for i, p in enumerate(participants):
                before = None
                if p.phase_id == 4:  # Sum2: its step runs once the seed dict is there
                    before = (i, bytes(p.save()), bytes(coord.fetch_round_params()),
                              bytes(coord.fetch_seeds(p.pk)))
                    if before[3][:1] != b"\x01":
                        continue
                done = len(seen["aggregate_masks"])
                p.tick()
                if p.should_set_model:
                    p.set_model(weights[i])
                if len(seen["aggregate_masks"]) > done:
                    saved.append(before + seen["aggregate_masks"][-1])
            body = coord.fetch_model()
            if body and body[0] == 1:
                model = np.asarray(sdk.decode_model(body, 0))
            time.sleep(0.002)
    finally:
        coord.stop()
    assert model is not None
    assert np.isfinite(model).all() and np.abs(model).max() <= 1.0 + 1e-5
    sealed = {args[0] for args, boxes in seen["seal_seed"] if boxes is not None}
    assert len(sealed) >= 3 and len(sealed) == len(seen["seal_seed"])
    assert saved and len(seen["open_seeds"]) == len(saved)
    assert all(got is not None for _, got in seen["open_seeds"])

    for i, state, params, seed_dict, (gpu_seeds, _, _), gpu_mask in saved:
        bodies, posted, cpu_seeds = {"params": params, "seeds": seed_dict}, [], []
        cpu = sdk.Participant.restore(
            state, sdk.PyTransportClient(lambda path, pk: bodies.get(path),
                                         lambda msg: posted.append(msg) or True),
            sign_seeds[i])
        cpu.set_sum2_hook(lambda seeds, *_: cpu_seeds.extend(seeds))  # None: the CPU sum
        for _ in range(3):
            if not posted:
                cpu.tick()
        assert posted and cpu.phase_id == 1  # its Sum2 message went out
        assert list(gpu_seeds) == cpu_seeds and 3 <= len(cpu_seeds) <= len(sealed)
        assert set(cpu_seeds) <= sealed
        agg = mk.Aggregation(s.mask_cfg, length)
        for seed in cpu_seeds:
            agg.aggregate(mk.derive_mask(seed, length, s.mask_cfg))
        assert gpu_mask == bytes(agg.object.serialize())
