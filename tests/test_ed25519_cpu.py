"""The K10 arithmetic (csrc/gpu/ed25519.h) on the host against RFC 8032 in
plain integers (ed25519_ref.py). Booleans and bytes: equality throughout."""
import numpy as np
import pytest
from ed25519_ref import CASES, L, decompress, verify

from xaynet_amd import _core

crypto = _core.crypto
WANT = [verify(*c) for c in CASES]


def test_reference_reads_the_host_rules():
    assert [crypto.verify_detached(*c) for c in CASES] == WANT
    assert WANT[:3] == [True] * 3 and True in WANT[3:] and False in WANT


@pytest.mark.parametrize("i", range(len(CASES)))
def test_verify_host(i):
    assert crypto.ed25519_verify_host(*CASES[i]) == WANT[i]


def test_sc_reduce512_host():
    rng = np.random.default_rng(10)
    values = [0, L - 1, L, 2**252, 2**512 - 1, 2**512 - L, 3 * L - 1]
    values += [int.from_bytes(rng.integers(0, 256, 64, dtype=np.uint8).tobytes(), "little")
               for _ in range(48)]
    for v in values:
        got = crypto.sc_reduce512_host(v.to_bytes(64, "little"))
        assert got == (v % L).to_bytes(32, "little"), hex(v)


def test_decompress_host():
    for pk in {c[2] for c in CASES}:
        want = decompress(pk)
        if want is not None:
            want = tuple(v.to_bytes(32, "little") for v in want)
        assert crypto.ed25519_decompress_host(pk) == want, pk.hex()
