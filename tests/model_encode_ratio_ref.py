"""The reference of the rational model body (K7r): Fraction(d, Q), numerator
and denominator split into base-2^32 digits and packed with struct. Shared by
tests/test_model_encode_ratio_cpu.py and tests/test_gpu_model_encode_ratio.py.
A plain module, no fixtures."""
import struct
from fractions import Fraction


def _big(sign, x):
    digits = []
    while x:
        digits.append(x & 0xFFFFFFFF)
        x >>= 32
    return struct.pack(f"<IQ{len(digits)}I", sign, len(digits), *digits)


def body(ds, q):
    """The Option<Model> bincode body of the weights d / q: head 01, u64 n,
    then per weight the reduced numerator (sign Minus 0, NoSign 1, Plus 2) and
    the positive denominator."""
    out = [struct.pack("<BQ", 1, len(ds))]
    for d in ds:
        f = Fraction(d, q)
        sign = 1 if f == 0 else 0 if f < 0 else 2
        out.append(_big(sign, abs(f.numerator)) + _big(2, f.denominator))
    return b"".join(out)
