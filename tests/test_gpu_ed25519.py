"""K10, batched Ed25519 verification on the GPU, against RFC 8032 in plain
integers (ed25519_ref.py) and the CPU pipeline. Booleans and bytes: equality."""
import numpy as np
import pytest
import torch
from ed25519_ref import padded, verify

from xaynet_amd import _core
from xaynet_amd.ops import GpuBox, gpu_available

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not gpu_available(), reason="needs an AMD GPU"),
]

crypto, msgmod = _core.crypto, _core.message
PK, SK = crypto.box_seed_keypair(b"\x21" * 32)
SEED = b"\x5e" * 32  # the round seed
SIGN_SEED = b"\x11" * 32
SPK, SSK = crypto.sign_keypair_from_seed(SIGN_SEED)


@pytest.fixture(scope="module")
def box():
    return GpuBox("cuda:0")


@pytest.fixture(scope="module")
def batch():
    cases = padded(257)
    return cases, [verify(*c) for c in cases]


def device(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0")


# a single lane, the wave seam, several workgroups
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_verify_batch_against_the_integer_reference(box, batch, n):
    cases, want = batch
    sigs, msgs, pks = zip(*cases[:n])
    assert box.verify_batch(sigs, msgs, pks) == want[:n]


def test_verify_batch_shared_key_and_device_items(box, batch):
    cases, want = batch
    pk = cases[3][2]
    same = [(i, c) for i, c in enumerate(cases) if c[2] == pk]
    sigs, msgs = [c[0] for _, c in same], [c[1] for _, c in same]
    sigs[1], msgs[5], msgs[9] = device(sigs[1]), device(msgs[5]), device(msgs[9])
    assert box.verify_batch(sigs, msgs, pk) == [want[i] for i, _ in same]
    assert box.verify_batch(sigs, msgs, device(pk)) == [want[i] for i, _ in same]
    assert box.verify_batch([], [], pk) == []
    for bad in [(sigs[:2], msgs[:1], pk), ([b"\0" * 63], [b""], pk), ([b"\0" * 64], [b""], pk[:31])]:
        with pytest.raises(ValueError):
            box.verify_batch(*bad)


def message(tag, payload, flags=0, length=None, sk=SSK):
    """A signed PET message from raw payload bytes."""
    n = 136 + len(payload) if length is None else length
    body = SPK + PK + n.to_bytes(4, "big") + bytes([tag, flags, 0, 0]) + payload
    return crypto.sign_detached(body[:n - 64], sk) + body


def cpu_flags(sealed, seed):
    plain = crypto.sealbox_open(sealed, PK, SK) if len(sealed) >= 48 else None
    if plain is None or len(plain) < 136:
        return plain, 0
    length, pk = int.from_bytes(plain[128:132], "big"), plain[64:96]
    if not 136 <= length <= len(plain):
        return plain, 0
    flags = int(crypto.verify_detached(plain[:64], plain[64:length], pk))
    if seed is not None and not plain[133] & 1 and plain[132] in (1, 2, 3):
        if length >= 200:
            flags |= 2 * crypto.verify_detached(plain[136:200], seed + b"sum", pk)
        if plain[132] == 2 and length >= 264:
            flags |= 4 * crypto.verify_detached(plain[200:264], seed + b"update", pk)
    return plain, flags


@pytest.mark.parametrize("seed", [SEED, None])
def test_open_messages(box, seed):
    rng = np.random.default_rng(30)
    filler = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
    sum_sig = crypto.sign_detached(SEED + b"sum", SSK)
    upd_sig = crypto.sign_detached(SEED + b"update", SSK)
    plains = [
        msgmod.encode(msgmod.TAG_SUM, sum_sig + b"\x44" * 32, SIGN_SEED, PK, max_payload=512)[0],
        message(2, sum_sig + upd_sig + filler),
        message(3, sum_sig + filler[:333]),
        message(2, filler[:300], flags=1),                          # a multipart chunk
        message(2, sum_sig + upd_sig[:20] + bytes([upd_sig[20] ^ 1]) + upd_sig[21:] + filler),  # a wrong update signature
        message(1, sum_sig + filler[:32], length=135),
        message(1, sum_sig[:63], length=136 + 63),                  # too short for its sum signature
    ]
    flipped = bytearray(message(1, sum_sig + filler[:32]))
    flipped[9] ^= 4
    plains.append(bytes(flipped))
    sealed = [crypto.sealbox_seal(p, PK) for p in plains]
    forged = bytearray(sealed[0])
    forged[40] ^= 1  # a bit of the tag
    sealed += [bytes(forged), b"\x01" * 47]
    sealed[1] = device(sealed[1])
    want = [cpu_flags(bytes(s.cpu().numpy()) if isinstance(s, torch.Tensor) else s, seed)
            for s in sealed]
    if seed is not None:
        assert [f for _, f in want] == [3, 7, 3, 1, 3, 0, 1, 2, 0, 0]
    else:
        assert all(f <= 1 for _, f in want)
    messages, flags = box.open_messages(sealed, PK, SK, round_seed=seed)
    assert flags == [f for _, f in want]
    assert [None if m is None else bytes(m.cpu().numpy()) for m in messages] == [p for p, _ in want]
