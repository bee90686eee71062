"""The Python surface of xaynet_amd._hip that ops/engine.py, ops/sum2.py and
the scripts rely on. Needs the built extension but no GPU."""
import gc

import pytest

_hip = pytest.importorskip("xaynet_amd._hip", reason="_hip extension not built")

PUBLIC_NAMES = {
    "MaskExpander",
    "add_to_planes",
    "aggregate_batch",
    "canonicalize",
    "device_count",
    "host_register",
    "host_unregister",
    "mask_pack",
    "mask_weights",
    "mod_add",
    "pack",
    "recode_planes",
    "synchronize",
    "unmask",
    "unmask_values",
    "unpack",
}


def test_hip_public_surface():
    names = {n for n in dir(_hip) if not n.startswith("_")}
    assert names == PUBLIC_NAMES
    assert {n for n in dir(_hip.MaskExpander) if not n.startswith("_")} == {"expand"}
    # the workspace is allocated on first use: constructing and collecting an
    # expander needs no device
    expander = _hip.MaskExpander()
    del expander
    gc.collect()


# The width boundary itself: 2^64 is the smallest wide order.
U64_ORDER = str(2**64 - 1)
WIDE_ORDER = str(2**64)
HI = 0x1000  # any non-null "pointer": len == 0, so it is never dereferenced

# Every binding that takes canonical values, as f(order, hi) with len = 0 and
# null data pointers. Past the form check such a call launches nothing.
VALUE_BINDINGS = {
    "expand": lambda o, hi: _hip.MaskExpander().expand(b"\0" * 32, 0, hi, 0, o, 8, 0),
    "canonicalize": lambda o, hi: _hip.canonicalize(0, 0, hi, 0, 3, o),
    "add_to_planes": lambda o, hi: _hip.add_to_planes(0, 0, hi, 0, 3, o),
    "mod_add": lambda o, hi: _hip.mod_add(0, hi, 0, hi, 0, o),
    "mod_add(b)": lambda o, hi: _hip.mod_add(0, HI if int(o) >> 64 else 0, 0, hi, 0, o),
    "unmask": lambda o, hi: _hip.unmask(0, 0, hi, 0, 0, 3, o, "1024", 0.0, 1.0, 0),
    "unmask_values": lambda o, hi: _hip.unmask_values(0, 0, hi, 0, 0, o, "1024", 0.0, 1.0, 0),
    "mask_pack": lambda o, hi: _hip.mask_pack(0, hi, 0, 0, 7, o, 0, 1.0, 1.0, "1024"),
    "mask_weights": lambda o, hi: _hip.mask_weights(0, 0, 0, hi, 0, 0, 7, o, 1.0, 1.0, "1024"),
    "pack": lambda o, hi: _hip.pack(0, hi, 0, 0, 7, o),
    "unpack": lambda o, hi: _hip.unpack(0, 0, hi, 0, 7, o),
}


@pytest.mark.parametrize("name", VALUE_BINDINGS)
def test_value_form_must_match_order_width(name):
    """(hi_ptr != 0) == (order >= 2^64), checked before any HIP call."""
    call = VALUE_BINDINGS[name]
    with pytest.raises(ValueError):
        call(WIDE_ORDER, 0)
    with pytest.raises(ValueError):
        call(U64_ORDER, HI)
    # the matching forms pass the check (expand then needs a device for its
    # workspace, unmask_values has no wide form)
    if name != "expand":
        call(U64_ORDER, 0)
        if name != "unmask_values":
            call(WIDE_ORDER, HI)


def test_width_restricted_bindings():
    for digit_bits in (16, 31, 33):  # the u64 kernels recombine 32-bit digits only
        with pytest.raises(ValueError):
            _hip.canonicalize(0, 0, 0, 0, 2, U64_ORDER, digit_bits)
        with pytest.raises(ValueError):
            _hip.add_to_planes(0, 0, 0, 0, 2, U64_ORDER, digit_bits)
        with pytest.raises(ValueError):
            _hip.unmask(0, 0, 0, 0, 0, 2, U64_ORDER, "1024", 0.0, 1.0, 0, digit_bits)
        _hip.canonicalize(0, 0, HI, 0, 2, WIDE_ORDER, digit_bits)
    with pytest.raises(ValueError):
        _hip.recode_planes(0, 0, 0, 2, U64_ORDER, 2, 39)
    _hip.recode_planes(0, 0, 0, 3, WIDE_ORDER, 2, 39)
    with pytest.raises(ValueError):
        _hip.unmask_values(0, 0, HI, 0, 0, WIDE_ORDER, "1024", 0.0, 1.0, 0)


def test_exact_offset_forms_for_u64_orders():
    """Integer outputs of u64 orders take the exact offset and divisor through
    both unmask bindings (len = 0: nothing is launched)."""
    _hip.unmask(0, 0, 0, 0, 0, 2, U64_ORDER, "1024", 0.0, 1.0, 3, 32, offset="5", divisor="3")
    _hip.unmask_values(0, 0, 0, 0, 0, U64_ORDER, "1024", 0.0, 1.0, 3, offset="5", divisor="3")
    _hip.unmask_values(0, 0, 0, 0, 0, U64_ORDER, "1024", 0.0, 1.0, 2, offset="5")
    with pytest.raises(ValueError):  # a divisor goes with an offset
        _hip.unmask_values(0, 0, 0, 0, 0, U64_ORDER, "1024", 0.0, 1.0, 3, divisor="3")
    with pytest.raises(ValueError):  # both are one word
        _hip.unmask_values(0, 0, 0, 0, 0, U64_ORDER, "1024", 0.0, 1.0, 3, offset=str(2**64))
    with pytest.raises(ValueError):  # the offset is below the order
        _hip.unmask(0, 0, 0, 0, 0, 2, U64_ORDER, "1024", 0.0, 1.0, 3, 32, offset=str(2**64))
    with pytest.raises(RuntimeError):  # float outputs of value sums keep the double kernel
        _hip.unmask_values(0, 0, 0, 0, 0, U64_ORDER, "1024", 0.0, 1.0, 0, offset="5")
    with pytest.raises(RuntimeError):  # integer outputs need a one-word exp_shift
        _hip.unmask(0, 0, HI, 0, 0, 2, WIDE_ORDER, str(10**20), 0.0, 1.0, 3, 32, offset="5")
