"""The Python surface of xaynet_amd._hip that ops/engine.py, ops/sum2.py and
the scripts rely on. Needs the built extension but no GPU."""
import gc

import pytest

_hip = pytest.importorskip("xaynet_amd._hip", reason="_hip extension not built")

PUBLIC_NAMES = {
    "MaskExpander",
    "add_u128_to_planes",
    "add_u64_to_planes",
    "aggregate_batch",
    "canonicalize",
    "canonicalize_u128",
    "device_count",
    "host_register",
    "host_unregister",
    "mask_pack",
    "mask_pack_u128",
    "mask_weights",
    "mod_add_u128",
    "mod_add_u64",
    "pack_u128",
    "pack_u64",
    "recode_planes_u128",
    "synchronize",
    "unmask",
    "unmask_u128",
    "unmask_values",
    "unpack_u128",
    "unpack_u64",
}


def test_hip_public_surface():
    names = {n for n in dir(_hip) if not n.startswith("_")}
    assert names == PUBLIC_NAMES
    assert {n for n in dir(_hip.MaskExpander) if not n.startswith("_")} == {
        "expand", "expand_u128"}
    # the workspace is allocated on first use: constructing and collecting an
    # expander needs no device
    expander = _hip.MaskExpander()
    del expander
    gc.collect()
