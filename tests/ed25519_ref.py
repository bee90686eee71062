"""RFC 8032 Ed25519 verification in plain Python integers with the acceptance
rules of crypto::ed25519_verify (csrc/gpu/ed25519.h lists them), and the case
list the K10 tests share."""
import hashlib

import numpy as np

from xaynet_amd import _core

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
SQRTM1 = pow(2, (P - 1) // 4, P)
crypto = _core.crypto


def decompress(pk: bytes):
    """(x, y) with y reduced mod p, or None."""
    y = (int.from_bytes(pk, "little") & (2**255 - 1)) % P
    sign = pk[31] >> 7
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * v**3 * pow(u * v**7, (P - 5) // 8, P) % P
    if (v * x * x - u) % P:
        if (v * x * x + u) % P:
            return None
        x = x * SQRTM1 % P
    if x == 0 and sign:
        return None
    return (P - x if x & 1 != sign else x), y


def add(p, q):
    """Extended coordinates (X, Y, Z, T), the unified addition of RFC 8032 5.1.4."""
    (x1, y1, z1, t1), (x2, y2, z2, t2) = p, q
    a, b = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P
    c, d = 2 * D * t1 * t2 % P, 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return e * f % P, g * h % P, f * g % P, e * h % P


def mul(k, p):
    r = (0, 1, 1, 0)
    while k:
        if k & 1:
            r = add(r, p)
        p, k = add(p, p), k >> 1
    return r


def point(xy):
    return xy[0], xy[1], 1, xy[0] * xy[1] % P


def encode(p) -> bytes:
    zi = pow(p[2], P - 2, P)
    return (p[1] * zi % P | (p[0] * zi % P & 1) << 255).to_bytes(32, "little")


BASE = point(decompress((4 * pow(5, P - 2, P) % P).to_bytes(32, "little")))


def verify(sig: bytes, msg: bytes, pk: bytes) -> bool:
    s, a = int.from_bytes(sig[32:], "little"), decompress(pk)
    if s >= L or a is None:
        return False
    k = int.from_bytes(hashlib.sha512(sig[:32] + pk + msg).digest(), "little") % L
    return encode(add(mul(s, BASE), mul(k, point((P - a[0], a[1]))))) == sig[:32]


def _le(v):
    return v.to_bytes(32, "little")


def _flip(b, bit):
    out = bytearray(b)
    out[bit // 8] ^= 1 << bit % 8
    return bytes(out)


def _cases():
    """(signature, message, key) triples."""
    rfc = [("d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a", "",
            "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e06522490155"
            "5fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b"),
           ("3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c", "72",
            "92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da"
            "085ac1e43e15996e458f3613d0f11d8c387b2eaeb4302aeeb00d291612bb0c00"),
           ("fc51cd8e6218a1a38da47ed00230f0580816ed13ba3303ac5deb911548908025", "af82",
            "6291d657deec24024827e69c3abe01a30ce548a284743a445e3680d7db5ac3ac"
            "18ff9b538d16f290ae67f760984dc6594a7c15e9716ed28dc027beceea1ec40a")]
    out = [(bytes.fromhex(s), bytes.fromhex(m), bytes.fromhex(k)) for k, m, s in rfc]
    rng = np.random.default_rng(20)
    pk, sk = crypto.sign_keypair_from_seed(b"\x2a" * 32)
    # R || A || M crosses the padding seams 111/112 and 239/240, the block
    # seams 127/128/129, and runs to 32 blocks
    for n in (0, 1, 47, 48, 63, 64, 65, 175, 176, 4032):
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        sig = crypto.sign_detached(msg, sk)
        out.append((sig, msg, pk))
        out.append((_flip(sig, 7 * n % 255), msg, pk))          # R
        out.append((_flip(sig, 256 + 5 * n % 250), msg, pk))    # s
        if n:
            out.append((sig, _flip(msg, 8 * n - 1 - n % 8), pk))
        else:
            out.append((sig, b"\x00", pk))
        out.append((sig, msg, _flip(pk, 3 * n % 256)))
    sig, msg, _ = out[3]
    s = int.from_bytes(sig[32:], "little")
    for v in (s + L, L, L - 1, 0, 2**256 - 1):
        out.append((sig[:32] + _le(v), msg, pk))
    # the identity, the same point as p + 1, x = 0 with the sign bit, order 2
    ident, order2 = _le(1), _le(P - 1)
    for key in (ident, _le(P + 1), _le(1 | 1 << 255), order2):
        out.append((encode(mul(5, BASE)) + _le(5), b"any message", key))
    out.append((encode(mul(7, BASE)) + _le(7), b"", ident))
    # a y for which u / v is no square
    y = next(y for y in range(2, 100) if decompress(_le(y)) is None)
    out.append((sig, msg, _le(y)))
    # R re-encoded as y + p where that fits in 255 bits (y < 19): the identity's
    # y = 1, a valid signature under the identity key but for that encoding
    out.append((_le(1 + P) + _le(0), b"R as y + p", ident))
    out.append((_le(1) + _le(0), b"R as y + p", ident))
    return out


CASES = _cases()


def padded(n: int):
    """The case list, then random valid and bit-flipped signatures up to n."""
    out = list(CASES)
    rng = np.random.default_rng(21)
    while len(out) < n:
        pk, sk = crypto.sign_keypair_from_seed(rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
        msg = rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes()
        sig = crypto.sign_detached(msg, sk)
        out.append((_flip(sig, int(rng.integers(0, 512))) if len(out) % 3 == 0 else sig, msg, pk))
    return out[:n]
