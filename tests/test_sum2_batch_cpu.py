"""The batched sum2 composition (ops/sum2.aggregate_masks_on) over the CPU
engine, and the form checks of the `_hip` arguments it relies on. No GPU."""
import pytest
import torch

from xaynet_amd import _core
from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator
from xaynet_amd.ops.sum2 import aggregate_masks_on

mk = _core.mask

LENGTH = 257
SEEDS = [bytes([b]) * 32 for b in (0, 7, 251, 1, 2, 9, 100)]
CONFIGS = {
    "u64": (1, 0, 0, 3),
    "u128": (1, 1, 0, 3),
    "bmax": (1, 0, 255, 3),  # f32 Bmax: five limbs
}


def oracle_bytes(cfg, seeds, length):
    """mk.Aggregation over the oracle masks, as wire bytes."""
    pair = mk.MaskConfigPair(cfg, cfg)
    agg = mk.Aggregation(pair, length)
    for seed in seeds:
        agg.aggregate(mk.derive_mask(seed, length, pair))
    return bytes(agg.object.serialize())


@pytest.mark.parametrize("name", CONFIGS)
def test_aggregate_masks_on_cpu_engine_equals_oracle(name):
    cfg = mk.MaskConfig(*CONFIGS[name])
    # a budget of four value rows and their candidates: 7 seeds go 4, 3
    row_bytes = 8 * ((int(cfg.order).bit_length() + 63) // 64) * LENGTH
    eng = CpuPlaneAggregator(cfg, cfg, LENGTH, sum2_budget_bytes=2 * 4 * row_bytes)
    assert eng.sum2_group == 4
    assert eng.batch_size == (1 if name == "bmax" else 4)
    total, scratch = eng.new_values(), eng.new_values()
    eng.acc.fill_(5)  # the update accumulator is not the sum2 task's
    wire = aggregate_masks_on(eng, total, scratch, SEEDS)
    assert wire == oracle_bytes(cfg, SEEDS, LENGTH)
    assert bool((eng.acc == 5).all())
    # a second call starts from zeroed planes
    assert aggregate_masks_on(eng, total, scratch, SEEDS[:2]) == oracle_bytes(cfg, SEEDS[:2],
                                                                            LENGTH)


@pytest.mark.parametrize("name", CONFIGS)
def test_batch_shapes_follow_new_values(name):
    cfg = mk.MaskConfig(*CONFIGS[name])
    eng = CpuPlaneAggregator(cfg, cfg, 17)
    rows = eng.derive_mask_values_batch(SEEDS[:3])
    one = eng.new_values()
    assert rows.shape == (3, *one.shape) and rows.dtype == one.dtype
    assert eng.new_rows(3).shape == rows.shape
    for s in range(3):
        assert torch.equal(rows[s], eng.derive_mask_values(SEEDS[s]))
    # rows into planes: the same planes as one values_to_planes call per row
    planes = torch.zeros_like(eng.acc)
    eng.add_rows_to_planes(rows, planes)
    want = torch.zeros_like(eng.acc)
    for s in range(3):
        eng.values_to_planes(rows[s], want)
    assert torch.equal(planes, want)
    with pytest.raises(ValueError):
        eng.derive_mask_values_batch(SEEDS[:3], out=eng.new_rows(2))


# ---- `_hip` form checks: len = 0 and null pointers, so nothing is launched

U64_ORDER = str(2**64 - 1)
WIDE_ORDER = str(2**64)
HI = 0x1000


@pytest.fixture(scope="module")
def hip():
    return pytest.importorskip("xaynet_amd._hip", reason="_hip extension not built")


def test_expand_batch_forms(hip):
    ex = hip.MaskExpander()
    two = b"\0" * 64
    with pytest.raises(ValueError):  # not a multiple of 32
        ex.expand(b"\0" * 33, 0, 0, 0, U64_ORDER, 8, 0)
    with pytest.raises(ValueError):
        ex.expand(b"", 0, 0, 0, U64_ORDER, 8, 0)
    with pytest.raises(ValueError):  # two seeds, one start word
        ex.expand(two, 0, 0, 0, U64_ORDER, 8, 0, seed_stride=8)
    with pytest.raises(ValueError):
        ex.expand(two, 0, 0, 0, U64_ORDER, 8, [0, 0, 0], seed_stride=8)
    with pytest.raises(ValueError):  # two seeds, no seed_stride
        ex.expand(two, 0, 0, 0, U64_ORDER, 8, [0, 0])
    with pytest.raises(ValueError):  # more seeds than grid rows
        ex.expand(b"\0" * (32 * 65536), 0, 0, 0, U64_ORDER, 8, [0] * 65536, seed_stride=8)
    with pytest.raises(ValueError):  # the width rule still comes first
        ex.expand(two, 0, HI, 0, U64_ORDER, 8, [0, 0], seed_stride=8)
    with pytest.raises(TypeError):  # seed_stride and attempts are keyword-only
        ex.expand(two, 0, 0, 0, U64_ORDER, 8, [0, 0], 8)
    # the good forms pass the checks and, with len = 0, launch nothing
    assert ex.expand(two, 0, 0, 0, U64_ORDER, 8, [0, 5], seed_stride=8) == 0
    assert ex.expand(two, 0, HI, 0, WIDE_ORDER, 12, (3, 4), seed_stride=8, attempts=100) == 0
    assert ex.expand(b"\0" * 32, 0, 0, 0, U64_ORDER, 8, [7]) == 0
    assert ex.expand(b"\0" * 32, 0, 0, 0, U64_ORDER, 8, 7, attempts=64) == 0


def test_add_to_planes_row_forms(hip):
    with pytest.raises(ValueError):  # several rows, no stride
        hip.add_to_planes(0, 0, 0, 0, 2, U64_ORDER, rows=2)
    with pytest.raises(ValueError):
        hip.add_to_planes(0, 0, HI, 0, 3, WIDE_ORDER, 32, rows=5, row_stride=0)
    with pytest.raises(ValueError):
        hip.add_to_planes(0, 0, 0, 0, 2, U64_ORDER, rows=0)
    with pytest.raises(ValueError):
        hip.add_to_planes(0, 0, 0, 0, 2, U64_ORDER, rows=65536, row_stride=8)
    with pytest.raises(TypeError):  # keyword-only
        hip.add_to_planes(0, 0, 0, 0, 2, U64_ORDER, 32, 2, 8)
    hip.add_to_planes(0, 0, 0, 0, 2, U64_ORDER, rows=2, row_stride=8)
    hip.add_to_planes(0, 0, HI, 0, 3, WIDE_ORDER, 32, rows=5, row_stride=16)
    hip.add_to_planes(0, 0, 0, 0, 2, U64_ORDER)


def test_batch_rule(hip):
    """Seeds share a launch only for u64/u128 orders and only while one seed's
    launch has at most 2048 candidate workgroups."""
    size = hip.MaskExpander._batch_size
    cfg = mk.MaskConfig(1, 0, 0, 3)  # p = 0.07, 2048 attempts per workgroup
    budget = 1 << 30
    assert size(4099, cfg.order, cfg.prng_nbytes, budget) > 1
    assert size(300_007, cfg.order, cfg.prng_nbytes, budget) == 1  # 2085 workgroups
    assert size(4099, cfg.order, cfg.prng_nbytes, 1) == 1  # never below one seed
    assert size(1, cfg.order, cfg.prng_nbytes, 1 << 40) == 65535
    bmax = mk.MaskConfig(1, 0, 255, 3)
    assert size(257, bmax.order, bmax.prng_nbytes, budget) == 1
