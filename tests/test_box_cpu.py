"""The GPU box arithmetic (csrc/gpu/box_stream.h) on the host, with tiles of 4
Salsa blocks so that the tile, tree and finish seams sit at tiny lengths.
Byte equality against the CPU secretbox and a big-integer Poly1305."""
import pytest

from xaynet_amd import _core

crypto = _core.crypto
OPEN, SEAL, MAC = 0, 1, 2
B = 4  # Salsa blocks a tile: tile 0 ends at message byte 4 * 64 - 32
KEY = bytes(range(1, 33))
NONCE = bytes(range(100, 124))

LENS = [0, 1, 15, 16, 17, 31, 32, 33]
LENS += [edge + d for edge in (4 * 64 - 32, 8 * 64 - 32) for d in (-17, -16, -1, 0, 1, 16)]
LENS += [70 * 4 * 64 - 32 + 5]  # more tiles than finish lanes: the stride wraps


def poly1305(msg, key):
    r = int.from_bytes(key[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    acc = 0
    for i in range(0, len(msg), 16):
        block = int.from_bytes(msg[i : i + 16] + b"\x01", "little")
        acc = (acc + block) * r % (2**130 - 5)
    return ((acc + int.from_bytes(key[16:], "little")) % 2**128).to_bytes(16, "little")


@pytest.mark.parametrize("n", LENS)
def test_tiled_box_equals_cpu_secretbox(n):
    msg = bytes((7 * i + n) % 251 for i in range(n))
    sealed = crypto.secretbox_seal(msg, NONCE, KEY)
    assert crypto.secretbox_open(sealed, NONCE, KEY) == msg
    assert crypto.box_stream_host(SEAL, msg, NONCE, KEY, B) == sealed
    assert crypto.box_stream_host(OPEN, sealed, NONCE, KEY, B) == msg
    assert crypto.box_stream_host(MAC, sealed[16:], b"", KEY, B) == poly1305(sealed[16:], KEY)
    if n:
        forged = sealed[:-1] + bytes([sealed[-1] ^ 1])
        assert crypto.box_stream_host(OPEN, forged, NONCE, KEY, B) is None


def test_beforenm_is_the_sealed_box_key():
    pk, sk = crypto.box_seed_keypair(b"\x05" * 32)
    sealed = crypto.sealbox_seal(b"seed material", pk)
    nonce = crypto.blake2b(sealed[:32] + pk, 24)
    key = crypto.box_beforenm(sealed[:32], sk)
    assert crypto.secretbox_open(sealed[32:], nonce, key) == b"seed material"
