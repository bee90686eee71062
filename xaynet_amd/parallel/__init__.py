"""Multi-GPU composition of the masked-aggregation engine over RCCL/xGMI.

One process per GPU (`torch.distributed`, backend "nccl" = RCCL on ROCm).
Because the accumulator is carry-free u64 digit planes, the cross-GPU
reduction is a PLAIN int64 sum — exactly what RCCL provides — with the
modular correction applied once afterwards (docs/ARCHITECTURE.md decision
#2; SURVEY.md §2.6 collective mapping).

xGMI is point-to-point (7 links per GPU), so ring collectives are
per-link-bound: prefer reduce-scatter of the planes plus an all-gather of
the (4x smaller) unmasked output over a full all-reduce. When
`world * order < 2^64` the reduce-scatter can run on canonical u64 values
instead of digit planes, halving the bytes on the wire again.

Wide orders (2^64 <= order <= 2^128) carry 3-4 accumulator planes (24-32 B
per element). Their reduce-scatter re-digitises the locally canonicalised
value into the fewest digit planes that still leave headroom for the
cross-rank sum (`compact_digits`): 2 planes up to 120-bit orders, 3 beyond —
16 or 24 B per element on the wire. The multi-limb Bmax orders (138..320
bits, 5 or 10 accumulator planes) take the same path with more planes: 3 at
138 bits, 5 or 6 at 289..320.

`bench.py` and the multi-GPU serve plane both drive their timed N>1 path
through this module, so the benchmark measures the production code;
`tests/test_distributed_planes.py` pins the underlying math on CPU (gloo,
world_size 2).
"""
from __future__ import annotations

import os

import torch

__all__ = ["choose_reduce_strategy", "compact_digits", "ShardedAggregation"]


def compact_digits(order_int: int, world: int) -> tuple[int, int]:
    """Fewest digit planes (k) and their width (w) for a cross-rank sum.

    k is the smallest count with ceil(bits/k) + ceil(log2(world)) <= 63 and
    w = ceil(bits/k), bits = order_int.bit_length(): every canonical value
    splits into k digits below 2^w, and a sum of `world` such digits stays
    below 2^63 (plain int64 collective, no overflow). k == 1 is exactly the
    "values_rs" condition.
    """
    bits = order_int.bit_length()
    head = max(world - 1, 0).bit_length()  # ceil(log2(world))
    if head > 62:
        raise ValueError(f"world {world} leaves no digit headroom in int64")
    k = 1
    while -(-bits // k) + head > 63:
        k += 1
    return k, -(-bits // k)


def choose_reduce_strategy(world: int, length: int, order_int: int,
                           env: dict | None = None) -> str:
    """Pick the cross-GPU reduction for a round.

    Returns one of:
      "single"     — world == 1, no collective.
      "values_rs"  — reduce-scatter canonical u64 values (half the bytes of
                     the plane RS). Valid while the summed values cannot
                     overflow 63 bits: order_bits + ceil(log2(world)) <= 63.
      "planes_rs"  — reduce-scatter each int64 digit plane, unmask the local
                     shard, all-gather the output.
      "digits_rs"  — wide orders (>= 2^64): re-digitise the canonical value
                     into `compact_digits` planes, reduce-scatter those,
                     unmask the local shard, all-gather the output.
      "all_reduce" — full plane all-reduce (fallback when the length does
                     not shard evenly, or forced with XAYNET_ALLREDUCE=1).
    """
    env = os.environ if env is None else env
    if world <= 1:
        return "single"
    if length % world != 0 or env.get("XAYNET_ALLREDUCE", "0") == "1":
        return "all_reduce"
    if order_int >= 2**64:
        return "digits_rs"
    if order_int.bit_length() + (world - 1).bit_length() <= 63:
        return "values_rs"
    return "planes_rs"


class ShardedAggregation:
    """Drive one rank's share of a distributed aggregation round.

    Each rank owns a GpuMaskedAggregator of the FULL model length and
    aggregates its own participants' updates locally; `unmask_global`
    performs the cross-rank reduction + unmask and returns the full
    unmasked model on every rank.

    `mask_total` must be the GLOBAL canonical mask values (same on every
    rank — use `allreduce_mask` to combine per-rank partial mask sums).
    Wide orders pass the [n_limbs, length] limb rows the engine uses ([2,
    length] lo/hi up to 2^128).
    """

    def __init__(self, eng, dist, rank: int, world: int):
        self.eng = eng
        self.dist = dist
        self.rank = rank
        self.world = world
        self.strategy = choose_reduce_strategy(world, eng.length, eng.order_int)
        self._shard = eng.length // world if self.strategy.endswith("_rs") else eng.length
        # wide orders: (plane count, digit width) of the compact cross-rank planes
        self._digits = compact_digits(eng.order_int, world) if eng.wide else None
        if self._digits is not None:  # the int64 collective cannot overflow
            assert world * (2**self._digits[1] - 1) < 2**63
        self._buf = {}  # persistent scratch (steady-state rounds reuse them)

    def _scratch(self, name: str, *shape, dtype=torch.int64):
        t = self._buf.get(name)
        if t is None or t.shape != shape or t.dtype != dtype:
            t = torch.empty(*shape, dtype=dtype, device=self.eng.device)
            self._buf[name] = t
        return t

    def allreduce_mask(self, mask_partial: torch.Tensor) -> torch.Tensor:
        """Modular all-reduce of per-rank canonical mask sums: lift to digit
        planes (plain int64 sum is overflow-free), all-reduce, canonicalize."""
        eng = self.eng
        if self.world <= 1:
            return mask_partial
        # wide values lift into the same compact planes the digits_rs path uses
        k, w = self._digits if eng.wide else (eng.n_digits, 32)
        planes = self._scratch("mask_planes", k, eng.length)
        planes.zero_()
        eng.values_to_planes(mask_partial, planes, digit_bits=w)
        self.dist.all_reduce(planes)
        eng.planes_to_values(planes, mask_partial, digit_bits=w)
        return mask_partial

    def unmask_global(self, mask_total: torch.Tensor, unit_mask_total: int,
                      nb_models: int, exact: bool = False) -> torch.Tensor:
        """Cross-rank reduce + unmask; returns the full model on every rank.
        exact is the engine's exact unmask mode, whatever the strategy: the
        refusal (ValueError) depends on the unit sum and the config alone, so
        every rank raises it or none does, before any collective."""
        eng, dist = self.eng, self.dist
        if exact:
            _, vinfo, dt = eng._unmask_scalars(unit_mask_total, nb_models)
            eng.exact_divisor(vinfo, dt)
        if self.strategy == "single":
            return eng.unmask(mask_total, unit_mask_total, nb_models=nb_models, exact=exact)
        if self.strategy == "all_reduce":
            dist.all_reduce(eng.acc)
            return eng.unmask(mask_total, unit_mask_total, nb_models=nb_models, exact=exact)
        shard, lo = self._shard, self.rank * self._shard
        out_full = self._scratch("out_full", eng.length,
                                 dtype=eng._TORCH_DTYPES[eng.vect_cfg.dtype])
        if self.strategy == "values_rs":
            canon = eng.canonical(out=self._scratch("canon", eng.length))
            vals_shard = self._scratch("vals_shard", shard)
            dist.reduce_scatter_tensor(vals_shard, canon)
            out_shard = eng.unmask_values(vals_shard, mask_total[lo:lo + shard],
                                          unit_mask_total, nb_models, exact=exact)
        elif self.strategy == "digits_rs":
            k, w = self._digits
            compact = eng.recode_planes(self._scratch("compact", k, eng.length), w)
            shard_planes = self._scratch("shard_planes", k, shard)
            for d in range(k):
                dist.reduce_scatter_tensor(shard_planes[d], compact[d])
            out_shard = eng.unmask_planes(shard_planes, mask_total[:, lo:lo + shard],
                                          unit_mask_total, nb_models, digit_bits=w,
                                          exact=exact)
        else:  # planes_rs
            shard_planes = self._scratch("shard_planes", eng.n_digits, shard)
            for d in range(eng.n_digits):
                dist.reduce_scatter_tensor(shard_planes[d], eng.acc[d])
            out_shard = eng.unmask_planes(shard_planes, mask_total[lo:lo + shard],
                                          unit_mask_total, nb_models, exact=exact)
        dist.all_gather_into_tensor(out_full, out_shard)
        return out_full
