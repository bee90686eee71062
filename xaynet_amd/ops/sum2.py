"""GPU-accelerated sum2 task: aggregate the update participants' masks.

The reference's hottest client-side loop (the sum participant
derives `n_updaters x model_length` PRNG draws and modularly adds them,
xaynet-sdk phases/sum2.rs:170-190). On an MI355X-equipped sum participant
this runs as K1 ChaCha20 expansion and a sum over the masks, and emits the
exact MaskObject wire bytes the coordinator expects — bit-identical to the CPU
oracle (the K1 compaction reproduces the reference's sequential rejection
stream).

u64 and u128 orders take the batched path: the seeds are expanded
`eng.batch_size` to a launch into value rows (one copy of keys in and one of
accepted counts out per batch, where the per-seed loop pays both per seed),
the rows' 32-bit digits are summed into digit planes — plain integer adds, as
the update accumulator's — and the planes are reduced modulo the order once.
Up to about a million weights, where a mask's kernels take tens of
microseconds, the host round trips were the cost. Where no more than
`_MIN_GROUP - 1` rows fit the workspace budget, and for the multi-limb f32 and
i64 Bmax orders, the masks are added one at a time with K2 modular adds as
before: a plane pass for so few rows moves more bytes than the mod-adds it
replaces.

All orders below 2^320; only the f64 Bmax orders stay on the CPU path.
"""
from __future__ import annotations

from .engine import GpuMaskedAggregator

# Fewest value rows worth a plane pass. Per mask and element a K2 mod-add
# moves 24 bytes per limb (total read and written, mask read); a pass over G
# rows reads 8 per limb and touches the n_digits planes (16 bytes each) once
# per G. At G = 2 the two are level, from 4 on the planes win clearly.
_MIN_GROUP = 4


def aggregate_masks(seeds, vect_cfg, unit_cfg, length: int, device: str = "cuda:0") -> bytes:
    """Derive and modularly aggregate one mask per 32-byte seed; returns the
    aggregated MaskObject wire bytes (MaskVect || MaskUnit)."""
    if not seeds:
        raise ValueError("no seeds")
    eng = GpuMaskedAggregator(vect_cfg, unit_cfg, length, device=device)
    return aggregate_masks_on(eng, eng.new_values(), eng.new_values(), seeds)


def aggregate_masks_on(eng, total, scratch, seeds) -> bytes:
    """aggregate_masks on an existing engine and two of its `new_values()`
    tensors (callers that serve many rounds keep all three). The batched path
    works in planes and rows that the engine owns (`sum2_workspace`) and
    leaves `scratch` alone."""
    seeds = [bytes(seed) for seed in seeds]
    unit_order = int(eng.unit_cfg.order)
    unit_total = 0
    for seed in seeds:
        unit_total = (unit_total + eng.unit_draw(seed)) % unit_order
    group = eng.sum2_group
    if eng.n_limbs > 2 or group < _MIN_GROUP:
        total.zero_()
        for seed in seeds:
            eng.derive_mask_values(seed, out=scratch)
            eng.mod_add_values(total, scratch)
    else:
        planes, rows = eng.sum2_workspace(len(seeds))
        for i in range(0, len(seeds), group):
            part = rows[: len(seeds[i:i + group])]
            eng.derive_mask_values_batch(seeds[i:i + group], out=part)
            eng.add_rows_to_planes(part, planes)
        eng.planes_to_values(planes, total)
    return eng.wire_object(eng.pack_wire(total), unit_total)
