"""Wide (u128) group orders on the GPU: integer unmask, generic digit widths,
compact-digit recode and the sharded (multi-rank) round.

Everything runs in ONE process on ONE device. Multi-rank rounds are emulated
in-process: W engines on the same device each aggregate their share of the
updates, one thread per rank calls `ShardedAggregation.unmask_global`, and
`LoopbackDist` stands in for the collectives by summing / copying the ranks'
tensors behind a barrier with a timeout (a broken rank fails the test, it
cannot hang it).

Inputs follow test_gpu_kernels.test_wide_order_f64_roundtrip_vs_oracle: CPU
`mask_model` updates uploaded as wire limbs, masks from `unpack_wire` of the
CPU-derived mask wire, a power-of-two participant count so every float step
of the unmask is exact."""
import functools
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from xaynet_amd import _core  # noqa: E402

mk = _core.mask

pytestmark = pytest.mark.gpu

LENGTH = 4 * 1027  # world 4 -> odd 1027-element shards, 8-byte-aligned only

# (k, digit_bits) of the compact planes and the config with that order width
RECODE_CASES = [
    ((1, 2, 6, 3), 1500, 4, 2, 33),     # 65-bit order
    ((1, 1, 0, 3), LENGTH, 8, 2, 39),   # 78
    ((1, 1, 4, 9), LENGTH, 8, 2, 56),   # 111
    ((1, 1, 6, 12), LENGTH, 8, 3, 43),  # 128 (prime)
]


def make_engine(cfg, length):
    from xaynet_amd.ops import GpuMaskedAggregator, gpu_available

    if not gpu_available():
        pytest.fail("GPU expected for -m gpu tests but not available")
    eng = GpuMaskedAggregator(cfg, cfg, length)
    assert eng.wide
    return eng


@functools.lru_cache(maxsize=None)
def forge_round(cfg_args, length, k):
    """k CPU-masked updates, their masks and the exact oracle; computed once
    per shape and shared (read-only) by the tests."""
    cfg = mk.MaskConfig(*cfg_args)
    pair = mk.MaskConfigPair(cfg, cfg)
    order, bpn = int(cfg.order), cfg.bytes_per_number
    rng = np.random.default_rng(8)
    agg, mask_agg = mk.Aggregation(pair, length), mk.Aggregation(pair, length)
    updates, masks, unit_acc = [], [], 0
    for _ in range(k):
        seed = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        if cfg.dtype in (2, 3):
            w = rng.integers(-10**6, 10**6 + 1, length).astype(
                np.int32 if cfg.dtype == 2 else np.int64)
        else:
            w = rng.uniform(-1, 1, length).astype(np.float64)
        masked = mk.mask_model(seed, mk.Scalar(1, k), w, pair)
        agg.aggregate(masked)
        m = mk.derive_mask(seed, length, pair)
        mask_agg.aggregate(m)
        updates.append(bytes(masked.serialize())[8 : 8 + length * bpn])
        masks.append(bytes(m.serialize())[8 : 8 + length * bpn])
        unit_acc = (unit_acc + int(masked.unit_value)) % order
    spots = sorted(set(range(0, length, 97)) | {length - 1})
    return {
        "cfg": cfg, "length": length, "k": k, "updates": updates, "masks": masks,
        "unit_acc": unit_acc,
        "mask_vect": bytes(mask_agg.object.serialize())[8 : 8 + length * bpn],
        "mask_unit": int(mask_agg.object.unit_value),
        "oracle": np.asarray(agg.unmask(mask_agg.object)),
        "elements": {i: int(agg.object.element(i)) for i in spots},
        "mask_elements": {i: int(mask_agg.object.element(i)) for i in spots},
    }


def load_engine(rnd, which=None):
    """Engine holding the aggregate of the updates in `which` (default all)."""
    eng = make_engine(rnd["cfg"], rnd["length"])
    which = list(range(rnd["k"])) if which is None else list(which)
    pool = eng.alloc_update_pool(len(which))
    for row, p in enumerate(which):
        eng.upload_update(pool, row, rnd["updates"][p])
    eng.aggregate_pool(pool, len(which))
    eng.unit_acc = rnd["unit_acc"]
    return eng


def unpack(eng, wire):
    t = torch.frombuffer(bytearray(wire), dtype=torch.uint8).to("cuda")
    return eng.unpack_wire(t)


def u128_at(split, i):
    """Element i of a [2, n] lo/hi int64 tensor (already on the CPU)."""
    return ((int(split[1][i]) % (1 << 64)) << 64) + (int(split[0][i]) % (1 << 64))


def assert_spots(split_dev, expect):
    split = split_dev.cpu().numpy()
    for i, v in expect.items():
        assert u128_at(split, i) == v, f"element {i}"


# ------------------------------------------------------------ loopback ranks


class LoopbackHub:
    """Shared state of W in-process ranks on one device."""

    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world, timeout=60)
        self.slots = [None] * world


class LoopbackDist:
    """The three collectives ShardedAggregation uses, for one rank. All
    ranks enqueue on the same (default) stream, so the host barriers also
    order the device work."""

    def __init__(self, hub, rank):
        self.hub, self.rank = hub, rank

    def _post(self, t):
        self.hub.slots[self.rank] = t
        self.hub.barrier.wait()
        return list(self.hub.slots)

    def all_reduce(self, t):
        total = torch.stack(self._post(t)).sum(dim=0)
        self.hub.barrier.wait()  # every rank has read the inputs
        t.copy_(total)

    def reduce_scatter_tensor(self, out, inp):
        n = out.numel()
        parts = [s[self.rank * n : (self.rank + 1) * n] for s in self._post(inp)]
        out.copy_(torch.stack(parts).sum(dim=0))
        self.hub.barrier.wait()

    def all_gather_into_tensor(self, out, inp):
        out.copy_(torch.cat(self._post(inp)))
        self.hub.barrier.wait()


def run_ranks(world, fn):
    """fn(rank, dist) on one thread per rank; returns the per-rank results.
    The first failure aborts the barrier so the other ranks stop at once."""
    hub = LoopbackHub(world)
    results, errors = [None] * world, []

    def body(rank):
        try:
            results[rank] = fn(rank, LoopbackDist(hub, rank))
        except BaseException as e:  # noqa: BLE001 — re-raised on the main thread
            errors.append((rank, e))
            hub.barrier.abort()

    threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a loopback rank did not finish"
    if errors:
        primary = [e for e in errors if not isinstance(e[1], threading.BrokenBarrierError)]
        rank, err = (primary or errors)[0]
        raise AssertionError(f"rank {rank} failed: {err!r}") from err
    return results


def sharded_round(rnd, world):
    """Every rank's unmask_global output plus the strategy taken."""
    from xaynet_amd.parallel import ShardedAggregation

    engines = [load_engine(rnd, range(r, rnd["k"], world)) for r in range(world)]
    mask_total = unpack(engines[0], rnd["mask_vect"])
    strategies = [None] * world

    def rank_fn(rank, dist):
        sharded = ShardedAggregation(engines[rank], dist, rank, world)
        strategies[rank] = sharded.strategy
        return sharded.unmask_global(mask_total, rnd["mask_unit"], rnd["k"]).clone()

    outs = run_ranks(world, rank_fn)
    assert len(set(strategies)) == 1
    return outs, strategies[0]


# --------------------------------------------------------------------- tests


@pytest.mark.parametrize("cfg_args,np_dtype", [((1, 2, 6, 3), np.int32),
                                               ((1, 3, 6, 3), np.int64)])
def test_wide_integer_unmask_vs_oracle(cfg_args, np_dtype):
    """Integer models on a wide order (bpn 9): k4_unmask_u128 truncates
    toward zero and equals the exact-rational oracle element-wise."""
    rnd = forge_round(cfg_args, 1500, 4)
    eng = load_engine(rnd)
    assert eng.bpn == 9
    out = eng.unmask(unpack(eng, rnd["mask_vect"]), rnd["mask_unit"]).cpu().numpy()
    oracle = rnd["oracle"]
    assert out.dtype == np_dtype and oracle.dtype == np_dtype
    assert np.abs(oracle).max() > 1000  # a real integer model, not all zeros
    assert (out == oracle).all(), f"{(out != oracle).sum()} mismatches vs oracle"


@pytest.mark.parametrize("cfg_args", [(1, 1, 0, 3), (1, 1, 4, 9)])
def test_wide_shard_unmask_equals_full(cfg_args):
    """unmask_planes on column shards of the accumulator (odd 1027-element
    shards, sliced non-contiguous mask) is bit-identical to unmask."""
    rnd = forge_round(cfg_args, LENGTH, 8)
    eng = load_engine(rnd)
    mask = unpack(eng, rnd["mask_vect"])
    full = eng.unmask(mask, rnd["mask_unit"])
    world, shard = 4, LENGTH // 4
    parts = []
    for r in range(world):
        lo = r * shard
        planes = eng.acc[:, lo : lo + shard].contiguous()
        parts.append(eng.unmask_planes(planes, mask[:, lo : lo + shard],
                                       rnd["mask_unit"], rnd["k"]))
    assert torch.equal(torch.cat(parts), full)


@pytest.mark.parametrize("cfg_args,length,k_updates,k,w", RECODE_CASES)
def test_wide_recode_roundtrip(cfg_args, length, k_updates, k, w):
    """recode_planes -> planes_to_values is the identity on canonical values,
    values_to_planes builds the same planes, digits stay below 2^w."""
    from xaynet_amd.parallel import compact_digits

    rnd = forge_round(cfg_args, length, k_updates)
    eng = load_engine(rnd)
    assert compact_digits(eng.order_int, 4) == (k, w)
    canon = eng.canonical()
    assert_spots(canon, rnd["elements"])

    planes = eng.recode_planes(
        torch.full((k, length), -1, dtype=torch.int64, device="cuda"), w)
    assert int(planes.min()) >= 0 and int(planes.max()) < 2**w
    back = torch.full((2, length), -1, dtype=torch.int64, device="cuda")
    eng.planes_to_values(planes, back, digit_bits=w)
    assert torch.equal(back, canon)

    lifted = torch.zeros(k, length, dtype=torch.int64, device="cuda")
    eng.values_to_planes(canon, lifted, digit_bits=w)
    assert torch.equal(lifted, planes)
    # values_to_planes ADDS: a second call doubles every digit, and the
    # doubled planes canonicalize to 2*v mod order
    eng.values_to_planes(canon, lifted, digit_bits=w)
    assert torch.equal(lifted, 2 * planes)
    eng.planes_to_values(lifted, back, digit_bits=w)
    assert_spots(back, {i: 2 * v % eng.order_int for i, v in rnd["elements"].items()})


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("cfg_args", [(1, 1, 0, 3), (1, 1, 6, 12)])
def test_wide_loopback_sharded_round(cfg_args, world):
    """digits_rs round over W in-process ranks: every rank's model is
    bit-identical to one engine that saw all 8 updates, and within 1e-9 of
    the exact-rational oracle (the bound of the existing wide test)."""
    rnd = forge_round(cfg_args, LENGTH, 8)
    outs, strategy = sharded_round(rnd, world)
    assert strategy == "digits_rs"
    single = load_engine(rnd)
    ref = single.unmask(unpack(single, rnd["mask_vect"]), rnd["mask_unit"])
    for rank, out in enumerate(outs):
        assert out.dtype == torch.float64
        assert torch.equal(out, ref), f"rank {rank} differs from the single-engine unmask"
    assert np.abs(ref.cpu().numpy() - rnd["oracle"]).max() < 1e-9


@pytest.mark.parametrize("cfg_args", [(1, 1, 0, 3), (1, 1, 6, 12)])
def test_wide_loopback_all_reduce_round(cfg_args):
    """A length that does not shard evenly falls back to the plane
    all-reduce, which is equally exact for wide engines."""
    rnd = forge_round(cfg_args, LENGTH + 1, 8)
    outs, strategy = sharded_round(rnd, 4)
    assert strategy == "all_reduce"
    single = load_engine(rnd)
    ref = single.unmask(unpack(single, rnd["mask_vect"]), rnd["mask_unit"])
    for rank, out in enumerate(outs):
        assert torch.equal(out, ref), f"rank {rank} differs from the single-engine unmask"
    assert np.abs(ref.cpu().numpy() - rnd["oracle"]).max() < 1e-9


@pytest.mark.parametrize("cfg_args", [(1, 1, 0, 3), (1, 1, 6, 12)])
def test_wide_loopback_allreduce_mask(cfg_args):
    """allreduce_mask of per-rank partial mask sums is the mod-order sum."""
    from xaynet_amd.parallel import ShardedAggregation

    rnd = forge_round(cfg_args, LENGTH, 8)
    world = 4
    engines = [make_engine(rnd["cfg"], LENGTH) for _ in range(world)]
    partials = []
    for r, eng in enumerate(engines):
        part = torch.zeros(2, LENGTH, dtype=torch.int64, device="cuda")
        for p in range(r, rnd["k"], world):
            eng.mod_add_values(part, unpack(eng, rnd["masks"][p]))
        partials.append(part)

    def rank_fn(rank, dist):
        sharded = ShardedAggregation(engines[rank], dist, rank, world)
        return sharded.allreduce_mask(partials[rank]).clone()

    expect = unpack(engines[0], rnd["mask_vect"])
    for rank, got in enumerate(run_ranks(world, rank_fn)):
        assert torch.equal(got, expect), f"rank {rank}"
    assert_spots(expect, rnd["mask_elements"])


def test_wide_digit_bits_32_regression():
    """The accumulator layout (digit_bits = 32) still canonicalizes and
    unmasks to the oracle after the generic-width change."""
    rnd = forge_round((1, 1, 0, 3), LENGTH, 8)
    eng = load_engine(rnd)
    canon = eng.canonical()
    assert_spots(canon, rnd["elements"])
    explicit = torch.empty_like(canon)
    eng.planes_to_values(eng.acc, explicit, digit_bits=32)
    assert torch.equal(explicit, canon)
    out = eng.unmask(unpack(eng, rnd["mask_vect"]), rnd["mask_unit"]).cpu().numpy()
    assert out.dtype == np.float64
    assert np.abs(out - rnd["oracle"]).max() < 1e-9
