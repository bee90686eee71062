"""RFC 7748 X25519 in plain Python integers, and the edge list the K9 tests
share: 14 points under three scalars each, then the RFC's own vectors."""
import numpy as np

P = 2**255 - 19
ORDER8 = (325606250916557431795983626356110631294008115727848805560023387167927233504,
          39382357235489614581723060781553021112529911719440698176882885853963445705823)
POINTS = [0, 1, P - 1, P, P + 1, *ORDER8, 2, 9, P - 2, 2**255 - 20, 2**255 - 1, 2**256 - 1,
          9 + 2**255]
# (scalar, point, result): RFC 7748 5.2, both vectors and the first iteration
RFC = [("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4",
        "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
        "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"),
       ("4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d",
        "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493",
        "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957"),
       ("09" + "00" * 31, "09" + "00" * 31,
        "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079")]


def x25519(scalar: bytes, point: bytes) -> bytes:
    k = (int.from_bytes(scalar, "little") & (2**254 - 8)) | 2**254
    x1 = int.from_bytes(point, "little") & (2**255 - 1)
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        bit = (k >> t) & 1
        if swap ^ bit:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = bit
        a, b, c, d = x2 + z2, x2 - z2, x3 + z3, x3 - z3
        aa, bb, da, cb = a * a % P, b * b % P, d * a % P, c * b % P
        e = aa - bb
        x3, z3 = (da + cb) ** 2 % P, x1 * (da - cb) ** 2 % P
        x2, z2 = aa * bb % P, e * (aa + 121665 * e) % P
    if swap:
        x2, z2 = x3, z3
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


def pairs(n: int, seed: int = 9):
    """n (scalar, point) pairs: the edge list first, random pairs behind it
    (or the first n of the edge list)."""
    rng = np.random.default_rng(seed)
    rand = lambda: rng.integers(0, 256, 32, dtype=np.uint8).tobytes()  # noqa: E731
    out = [(s, u.to_bytes(32, "little")) for u in POINTS for s in (bytes(32), b"\xff" * 32, rand())]
    out += [(bytes.fromhex(s), bytes.fromhex(u)) for s, u, _ in RFC]
    while len(out) < n:
        out.append((rand(), rand()))
    return out[:n]
