"""K8, batched XSalsa20-Poly1305 on the GPU, against the CPU box
(`_core.crypto`, pinned to the NaCl vectors in test_crypto.py) and a
big-integer Poly1305. Every comparison is byte equality."""
import numpy as np
import pytest
import torch

from xaynet_amd import _core
from xaynet_amd.ops import GpuBox, gpu_available

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not gpu_available(), reason="needs an AMD GPU"),
]

crypto = _core.crypto
P = 2**130 - 5
TILE0 = 16384 - 32  # message bytes in a box's first tile
LENS = [0, 1, 16, 31, 32, 33, 95, 96, 97]
LENS += [TILE0 + d for d in (-16, -1, 0, 1, 16)]
LENS += [TILE0 + 16384 + 1, 65 * 16384 + 5]  # the last: more tiles than finish lanes


def poly1305(msg, key):
    """(tag, whether the accumulator was exactly 2^130 - 5 before a reduction)"""
    r = int.from_bytes(key[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    acc, through_p = 0, False
    for i in range(0, len(msg), 16):
        acc = (acc + int.from_bytes(msg[i : i + 16] + b"\x01", "little")) * r
        through_p |= acc == P
        acc %= P
    return ((acc + int.from_bytes(key[16:], "little")) % 2**128).to_bytes(16, "little"), through_p


@pytest.fixture(scope="module")
def box():
    return GpuBox("cuda:0")


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(8)
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LENS]
    keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in LENS]
    nonces = [rng.integers(0, 256, 24, dtype=np.uint8).tobytes() for _ in LENS]
    sealed = [crypto.secretbox_seal(m, n, k) for m, n, k in zip(msgs, nonces, keys)]
    return msgs, keys, nonces, sealed


def host(t):
    return bytes(t.cpu().numpy())


def test_seal_and_open_agree_with_the_cpu_box(box, batch):
    msgs, keys, nonces, sealed = batch
    assert [host(t) for t in box.secretbox_seal_batch(msgs, keys, nonces)] == sealed
    opened, ok = box.secretbox_open_batch(sealed, keys, nonces)
    assert ok.all()
    assert [host(t) for t in opened] == msgs
    assert box.opened_buffer.data_ptr() % 16 == 0 and all(o % 16 == 0 for o in box.opened_offsets)


def test_sealed_box_interop_both_ways(box, batch):
    msgs = batch[0][:12]
    pk, sk = crypto.box_seed_keypair(b"\x21" * 32)
    opened, ok = box.sealbox_open_batch([crypto.sealbox_seal(m, pk) for m in msgs], pk, sk)
    assert ok.all() and [host(t) for t in opened] == msgs
    on_device = torch.frombuffer(bytearray(msgs[-1]), dtype=torch.uint8).to("cuda:0")
    sealed = box.sealbox_seal_batch(msgs[:-1] + [on_device], pk)
    assert [crypto.sealbox_open(host(t), pk, sk) for t in sealed] == msgs


def test_forged_boxes_open_to_nothing(box, batch):
    msgs, keys, nonces, sealed = batch
    flips = {3: 0, 10: len(sealed[10]) - 1, 14: 16}  # a tag bit, the last and the first cipher byte
    forged = [bytearray(s) for s in sealed]
    for i, at in flips.items():
        forged[i][at] ^= 1
    opened, ok = box.secretbox_open_batch(forged, keys, nonces)
    assert [i for i, t in enumerate(opened) if t is None] == sorted(flips)
    assert [i for i, good in enumerate(ok.tolist()) if not good] == sorted(flips)
    assert all(host(t) == msgs[i] for i, t in enumerate(opened) if t is not None)
    # the forged boxes' plaintext is gone from the packed buffer too
    for i in flips:
        off = box.opened_offsets[i]
        assert host(box.opened_buffer[off : off + LENS[i]]) == bytes(LENS[i])


R_MAX = (0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF).to_bytes(16, "little")
ONE = (1).to_bytes(16, "little")
MAC_CASES = [(R_MAX + b"\xff" * 16, b"\xff" * n)
             for n in (16, 17, 1022 * 16, 1022 * 16 + 1024 * 16 + 1)]
MAC_CASES += [(bytes(16) + bytes(range(16)), bytes(range(200)))]  # r = 0
# r = 1 and the one block that lifts the accumulator to exactly 2^130 - 5:
# after a first block b0 the sum is b0 + 2^128, so the second is p - that - 2^128
B0 = 2**128 - 1
MAC_CASES += [(ONE + bytes(range(16)),
               B0.to_bytes(16, "little") + (P - (B0 + 2**128) - 2**128).to_bytes(16, "little"))]


@pytest.mark.parametrize("case", range(len(MAC_CASES)))
def test_poly1305_edges(box, case):
    key, msg = MAC_CASES[case]
    tag, through_p = poly1305(msg, key)
    assert through_p == (case == len(MAC_CASES) - 1)
    assert box.poly1305(msg, key) == tag
