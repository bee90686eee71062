"""GPU-accelerated sum2 task: aggregate the update participants' masks.

The reference's hottest client-side loop (the sum participant
derives `n_updaters x model_length` PRNG draws and modularly adds them,
xaynet-sdk phases/sum2.rs:170-190). On an MI355X-equipped sum participant
this runs as K1 ChaCha20 expansion + K2 modular adds and emits the exact
MaskObject wire bytes the coordinator expects — bit-identical to the CPU
oracle (the K1 compaction reproduces the reference's sequential rejection
stream).

All orders below 2^320 (u64 fast path, split lo/hi u128 kernels, multi-limb
kernels for the f32 and i64 Bmax orders); only the f64 Bmax orders stay on the
CPU path.
"""
from __future__ import annotations

from .engine import GpuMaskedAggregator


def aggregate_masks(seeds, vect_cfg, unit_cfg, length: int, device: str = "cuda:0") -> bytes:
    """Derive and modularly aggregate one mask per 32-byte seed; returns the
    aggregated MaskObject wire bytes (MaskVect || MaskUnit)."""
    if not seeds:
        raise ValueError("no seeds")
    eng = GpuMaskedAggregator(vect_cfg, unit_cfg, length, device=device)
    return aggregate_masks_on(eng, eng.new_values(), eng.new_values(), seeds)


def aggregate_masks_on(eng, total, scratch, seeds) -> bytes:
    """aggregate_masks on an existing engine and two of its `new_values()`
    tensors (callers that serve many rounds keep all three)."""
    total.zero_()
    unit_order = int(eng.unit_cfg.order)
    unit_total = 0
    for seed in seeds:
        seed = bytes(seed)
        eng.derive_mask_values(seed, out=scratch)
        eng.mod_add_values(total, scratch)
        unit_total = (unit_total + eng.unit_draw(seed)) % unit_order
    return eng.wire_object(eng.pack_wire(total), unit_total)
