"""The K9 arithmetic (csrc/gpu/fe25519.h) on the host against RFC 7748 in
plain integers and the CPU box. Byte equality throughout."""
from x25519_ref import ORDER8, RFC, pairs, x25519

from xaynet_amd import _core

crypto = _core.crypto


def test_x25519_host_edges_and_random_pairs():
    batch = pairs(45 + 200)
    for s, u in batch:
        assert crypto.x25519_host(s, u) == x25519(s, u), (s.hex(), u.hex())
    # entries 42..44 are the RFC's own vectors: their outputs as the RFC prints them
    assert [crypto.x25519_host(s, u).hex() for s, u in batch[42:45]] == [r for _, _, r in RFC]


def test_seal_nonce_host_is_blake2b_24():
    for s, u in pairs(45 + 8)[40:]:
        assert crypto.seal_nonce_host(s, u) == crypto.blake2b(s + u, 24)


def test_box_key_from_the_ladder_takes_a_low_order_key():
    sk = b"\x5a" * 32
    low, other = ORDER8[0].to_bytes(32, "little"), pairs(60)[59][1]
    assert crypto.x25519_host(sk, low) == bytes(32)  # not rejected: the zero secret
    for epk in (low, other):
        assert crypto.box_key_host(epk, sk) == crypto.box_beforenm(epk, sk)
