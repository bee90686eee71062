"""Wide (u128) group orders across ranks, on CPU.

Part A pins the strategy choice and the compact-digit arithmetic
(`compact_digits`): the cross-rank reduction of a wide order re-digitises
the canonical value into the fewest planes whose per-plane sum over `world`
ranks still fits int64.

Part B runs the real composition (`ShardedAggregation` over wide
`CpuPlaneAggregator`s) on gloo with 2 processes, and one serve-plane round,
against the exact CPU oracle (_core.mask.Aggregation)."""
import socket

import numpy as np
import pytest
import torch

from xaynet_amd import _core

mk = _core.mask

# ------------------------------------------------------------------ part A


def _catalogue_orders():
    """Every mask-config group order of at most 128 bits."""
    orders = set()
    for group in (0, 1, 2):
        for dtype in (0, 1, 2, 3):
            for bound in (0, 2, 4, 6, 255):
                for model in (3, 6, 9, 12):
                    try:
                        cfg = mk.MaskConfig(group, dtype, bound, model)
                    except Exception:  # noqa: BLE001 — not in the catalogue
                        continue
                    order = int(cfg.order)
                    if order.bit_length() <= 128:
                        orders.add(order)
    return sorted(orders)


@pytest.mark.parametrize("cfg_args,bits,expect", [
    ((1, 2, 6, 3), 65, (2, 33)),
    ((1, 1, 0, 3), 78, (2, 39)),
    ((1, 1, 4, 9), 111, (2, 56)),
    ((1, 1, 6, 12), 128, (3, 43)),
])
def test_compact_digits_values(cfg_args, bits, expect):
    from xaynet_amd.parallel import compact_digits

    order = int(mk.MaskConfig(*cfg_args).order)
    assert order.bit_length() == bits
    for world in (2, 4, 8):
        assert compact_digits(order, world) == expect


def test_compact_digits_invariants():
    from xaynet_amd.parallel import choose_reduce_strategy, compact_digits

    orders = _catalogue_orders()
    assert any(o >= 2**64 for o in orders) and any(o < 2**64 for o in orders)
    for order in orders:
        bits = order.bit_length()
        for world in (2, 4, 8, 64):
            k, w = compact_digits(order, world)
            assert world * (2**w - 1) < 2**63, (order, world)
            assert k * w >= bits, (order, world)
            # k is minimal: one plane fewer would overflow the cross-rank sum
            if k > 1:
                w_less = -(-bits // (k - 1))
                assert w_less + (world - 1).bit_length() > 63
            # k == 1 is exactly the canonical-values reduce-scatter condition
            if order < 2**64:
                assert (k == 1) == (choose_reduce_strategy(world, world * 8, order, env={})
                                    == "values_rs")


def test_choose_reduce_strategy_wide():
    from xaynet_amd.parallel import choose_reduce_strategy as pick

    for cfg_args in ((1, 2, 6, 3), (1, 1, 0, 3), (1, 1, 6, 12)):
        order = int(mk.MaskConfig(*cfg_args).order)
        assert order >= 2**64
        assert pick(1, 1000, order) == "single"
        for world in (2, 4, 8):
            assert pick(world, 1000 * world, order) == "digits_rs"
            assert pick(world, 1000 * world + 1, order) == "all_reduce"
            assert pick(world, 1000 * world, order,
                        env={"XAYNET_ALLREDUCE": "1"}) == "all_reduce"
    # the boundary: 2^64 itself is wide, anything below keeps its strategy
    assert pick(2, 1000, 2**64) == "digits_rs"
    assert pick(2, 1000, 2**64 - 59) == "planes_rs"


# ------------------------------------------------------------------ part B

LENGTH = 258
K = 4  # participants, scalar 1/4: every float step of the unmask is exact


def _weights(cfg, length, rng):
    if cfg.dtype in (2, 3):
        np_dt = np.int32 if cfg.dtype == 2 else np.int64
        return rng.integers(-10**6, 10**6 + 1, length).astype(np_dt)
    return rng.uniform(-1, 1, length).astype(np.float64)


def _forge_round(cfg_args, length, k, rng_seed=5):
    """k masked updates, their masks, and the oracle's unmasked model."""
    cfg = mk.MaskConfig(*cfg_args)
    pair = mk.MaskConfigPair(cfg, cfg)
    order, bpn = int(cfg.order), cfg.bytes_per_number
    rng = np.random.default_rng(rng_seed)
    agg, mask_agg = mk.Aggregation(pair, length), mk.Aggregation(pair, length)
    updates, masks, unit_acc = [], [], 0
    for _ in range(k):
        seed = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        masked = mk.mask_model(seed, mk.Scalar(1, k), _weights(cfg, length, rng), pair)
        agg.aggregate(masked)
        m = mk.derive_mask(seed, length, pair)
        mask_agg.aggregate(m)
        updates.append(bytes(masked.serialize())[8 : 8 + length * bpn])
        masks.append(bytes(m.serialize())[8 : 8 + length * bpn])
        unit_acc = (unit_acc + int(masked.unit_value)) % order
    mask_vect = bytes(mask_agg.object.serialize())[8 : 8 + length * bpn]
    return {
        "cfg": cfg, "updates": updates, "masks": masks, "unit_acc": unit_acc,
        "mask_vect": mask_vect, "mask_unit": int(mask_agg.object.unit_value),
        "oracle": np.asarray(agg.unmask(mask_agg.object)),
    }


def _as_tensor(wire: bytes) -> torch.Tensor:
    return torch.frombuffer(bytearray(wire), dtype=torch.uint8)


def _gloo_worker(rank: int, world: int, port: int, cfg_args):
    import torch.distributed as dist

    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator
    from xaynet_amd.parallel import ShardedAggregation

    dist.init_process_group(
        "gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world
    )
    try:
        rnd = _forge_round(cfg_args, LENGTH, K)
        cfg = rnd["cfg"]
        eng = CpuPlaneAggregator(cfg, cfg, LENGTH)
        assert eng.wide
        mine = list(range(rank, K, world))
        pool = eng.alloc_update_pool(len(mine))
        for row, p in enumerate(mine):
            eng.upload_update(pool, row, rnd["updates"][p])
        eng.aggregate_pool(pool, len(mine))
        eng.unit_acc = rnd["unit_acc"]

        sharded = ShardedAggregation(eng, dist, rank, world)
        assert sharded.strategy == "digits_rs"

        # per-rank partial mask sums -> modular all-reduce == oracle's mask
        partial = torch.zeros(2, LENGTH, dtype=torch.int64)
        for p in mine:
            eng.mod_add_values(partial, eng.unpack_wire(_as_tensor(rnd["masks"][p])))
        mask_total = sharded.allreduce_mask(partial)
        expect_mask = eng.unpack_wire(_as_tensor(rnd["mask_vect"]))
        assert torch.equal(mask_total, expect_mask), f"rank {rank}: mask all-reduce"

        out = sharded.unmask_global(mask_total, rnd["mask_unit"], K).numpy()
        oracle = rnd["oracle"]
        assert out.shape == (LENGTH,)
        if cfg.dtype == 2:
            assert out.dtype == np.int32
            assert (out == oracle).all(), f"rank {rank}: {(out != oracle).sum()} mismatches"
        else:
            assert out.dtype == np.float64
            assert np.abs(out - oracle).max() < 1e-9, f"rank {rank}"
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("cfg_args", [(1, 1, 0, 3), (1, 2, 6, 3)])
def test_gloo_wide_sharded_round(cfg_args):
    """world-2 digits_rs round over wide CPU engines: f64 within 1e-9 of the
    exact-rational oracle, int32 exact."""
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    world = 2
    mp.spawn(_gloo_worker, args=(world, port, cfg_args), nprocs=world, join=True)


def test_wide_cpu_engine_single():
    """The wide CPU twin on its own: canonical, recode round-trip and unmask
    agree with the oracle (what the gloo round composes)."""
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator
    from xaynet_amd.parallel import compact_digits

    rnd = _forge_round((1, 1, 6, 12), LENGTH, K)  # 128-bit prime order, k = 3
    cfg = rnd["cfg"]
    eng = CpuPlaneAggregator(cfg, cfg, LENGTH)
    pool = eng.alloc_update_pool(K)
    for p in range(K):
        eng.upload_update(pool, p, rnd["updates"][p])
    eng.aggregate_pool(pool, K)
    eng.unit_acc = rnd["unit_acc"]

    canon = eng.canonical()
    assert canon.shape == (2, LENGTH)
    assert torch.equal(eng.unpack_wire(eng.pack_wire(canon)), canon)
    k, w = compact_digits(eng.order_int, 8)
    assert (k, w) == (3, 43)
    planes = eng.recode_planes(torch.empty(k, LENGTH, dtype=torch.int64), w)
    assert int(planes.max()) < 2**w and int(planes.min()) >= 0
    back = torch.empty(2, LENGTH, dtype=torch.int64)
    eng.planes_to_values(planes, back, digit_bits=w)
    assert torch.equal(back, canon)
    lifted = torch.zeros(k, LENGTH, dtype=torch.int64)
    eng.values_to_planes(canon, lifted, digit_bits=w)
    assert torch.equal(lifted, planes)

    mask = eng.unpack_wire(_as_tensor(rnd["mask_vect"]))
    out = eng.unmask(mask, rnd["mask_unit"]).numpy()
    assert np.abs(out - rnd["oracle"]).max() < 1e-9
    shard = eng.unmask_planes(planes[:, 100:200].contiguous(), mask[:, 100:200],
                              rnd["mask_unit"], K, digit_bits=w).numpy()
    assert (shard == out[100:200]).all()


def test_serve_plane_round_wide():
    """One serve-plane round (2 CPU workers, gloo) on a wide f64 config."""
    from xaynet_amd.parallel.serve import ServePlane

    cfg_args = (1, 1, 0, 3)
    rnd = _forge_round(cfg_args, LENGTH, K)
    plane = ServePlane(cfg_args, LENGTH, 2, "cpu", slots_per_worker=4, batch=2)
    try:
        for v in rnd["updates"]:
            plane.put_update(v)
        out = plane.unmask(rnd["mask_vect"], rnd["mask_unit"], rnd["unit_acc"], K, round_id=1)
        assert out.dtype == np.float64
        assert np.abs(out - rnd["oracle"]).max() < 1e-9
    finally:
        plane.stop()
