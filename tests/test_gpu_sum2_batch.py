"""Batched sum2 mask expansion on the GPU: many seeds per launch, summed into
digit planes.

Every row of `derive_mask_values_batch` is compared bit for bit with the CPU
oracle's `_core.mask.derive_mask`, and the wire bytes of `aggregate_masks`
with `mk.Aggregation` over the oracle masks. Oracle masks are derived once per
(config, seed, length) and shared read-only."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from xaynet_amd import _core  # noqa: E402

mk = _core.mask

pytestmark = pytest.mark.gpu

LENGTH = 4099  # odd; 29 candidate workgroups per seed at p = 0.07, 17 scatter-loop trips
SEED_BYTES = (0, 7, 251, 1, 2)

PRIME_F32_M3 = (1, 0, 0, 3)      # bpn 6, 6-byte draws, acceptance 0.07
PRIME_F32_M6 = (1, 0, 0, 6)      # bpn 7, 7-byte draws (top word masked)
POW2_F32_M3 = (2, 0, 0, 3)       # power-of-two order: acceptance is a bit test
PRIME_F64_M3 = (1, 1, 0, 3)      # bpn 10: 3-word draws, 5 attempts per thread
PRIME_F64_B4_M9 = (1, 1, 4, 9)   # bpn 14: 4-word draws, 4 attempts per thread
PRIME_I64_BMAX_M12 = (1, 3, 255, 12)  # 138-bit order: three limbs
PRIME_F32_BMAX_M3 = (1, 0, 255, 3)    # 289-bit order: five limbs


def seeds_of(seed_bytes):
    return [bytes([b]) * 32 for b in seed_bytes]


def make_engine(cfg_args, length, **kw):
    from xaynet_amd.ops import GpuMaskedAggregator, gpu_available

    if not gpu_available():
        pytest.fail("GPU expected for -m gpu tests but not available")
    cfg = mk.MaskConfig(*cfg_args)
    return GpuMaskedAggregator(cfg, cfg, length, **kw)


@functools.lru_cache(maxsize=None)
def oracle_mask(cfg_args, seed, length):
    cfg = mk.MaskConfig(*cfg_args)
    return mk.derive_mask(seed, length, mk.MaskConfigPair(cfg, cfg))


def oracle_rows(cfg_args, seeds, length):
    """The oracle masks in the engine's layout: uint64 [S, n], or [S,
    n_limbs, n] limb rows for wide orders."""
    cfg = mk.MaskConfig(*cfg_args)
    bpn = cfg.bytes_per_number
    n_limbs = (int(cfg.order).bit_length() + 63) // 64
    rows = []
    for seed in seeds:
        raw = np.frombuffer(bytes(oracle_mask(cfg_args, seed, length).vect_bytes), dtype=np.uint8)
        padded = np.zeros((length, 8 * n_limbs), dtype=np.uint8)
        padded[:, :bpn] = raw.reshape(length, bpn)
        limbs = np.ascontiguousarray(padded).view("<u8").T  # [n_limbs, n]
        rows.append(limbs if n_limbs > 1 else limbs[0])
    return np.stack(rows)


def oracle_wire(cfg_args, seeds, length):
    cfg = mk.MaskConfig(*cfg_args)
    agg = mk.Aggregation(mk.MaskConfigPair(cfg, cfg), length)
    for seed in seeds:
        agg.aggregate(oracle_mask(cfg_args, seed, length))
    return bytes(agg.object.serialize())


def assert_rows_equal(rows, cfg_args, seeds, length):
    got = rows.cpu().numpy().view(np.uint64)
    want = oracle_rows(cfg_args, seeds, length)
    assert got.shape == want.shape
    for s in range(len(seeds)):
        assert np.array_equal(got[s], want[s]), f"seed {s} differs from the oracle"


def aggregate_on(eng, seeds):
    from xaynet_amd.ops.sum2 import aggregate_masks_on

    return aggregate_masks_on(eng, eng.new_values(), eng.new_values(), seeds)


def budget_for_batch(cfg_args, length, batch):
    """The smallest workspace budget (in KiB steps) at which `batch` seeds
    share a launch."""
    from xaynet_amd import _hip

    cfg = mk.MaskConfig(*cfg_args)
    for kib in range(1, 1 << 16):
        if _hip.MaskExpander._batch_size(length, cfg.order, cfg.prng_nbytes, kib << 10) == batch:
            return kib << 10
    raise AssertionError("no budget gives this batch size")


# ---- 1, 2: ragged start words, every draw width


@pytest.mark.parametrize("cfg_args", [PRIME_F32_M3, PRIME_F32_M6, POW2_F32_M3])
def test_u64_batch_ragged_start_words(cfg_args):
    seeds = seeds_of(SEED_BYTES)
    unit_cfg = mk.MaskConfig(*cfg_args)
    words = [mk.unit_draw(s, unit_cfg)[1] for s in seeds]
    assert len(set(words)) >= 2, "the seeds' unit draws must consume different word counts"
    eng = make_engine(cfg_args, LENGTH)
    assert eng.batch_size >= len(seeds)  # one launch
    rows = eng.derive_mask_values_batch(seeds)
    assert rows.shape == (len(seeds), LENGTH)
    assert_rows_equal(rows, cfg_args, seeds, LENGTH)
    assert aggregate_on(eng, seeds) == oracle_wire(cfg_args, seeds, LENGTH)


@pytest.mark.parametrize("cfg_args", [PRIME_F64_M3, PRIME_F64_B4_M9])
def test_u128_batch(cfg_args):
    seeds = seeds_of(SEED_BYTES[:3])
    eng = make_engine(cfg_args, LENGTH)
    assert eng.batch_size >= len(seeds)
    rows = eng.derive_mask_values_batch(seeds)
    assert rows.shape == (len(seeds), 2, LENGTH)
    assert_rows_equal(rows, cfg_args, seeds, LENGTH)
    assert aggregate_on(eng, seeds) == oracle_wire(cfg_args, seeds, LENGTH)


def test_public_aggregate_masks_takes_the_batched_path():
    from xaynet_amd.ops.sum2 import aggregate_masks

    seeds = seeds_of(SEED_BYTES)
    cfg = mk.MaskConfig(*PRIME_F32_M6)
    assert aggregate_masks(seeds, cfg, cfg, LENGTH) == oracle_wire(PRIME_F32_M6, seeds, LENGTH)


# ---- 3: batch boundaries


@pytest.mark.parametrize("length", [1, 17])
@pytest.mark.parametrize("cfg_args", [PRIME_F32_M3, PRIME_F64_M3])
def test_batches_of_three_three_one(cfg_args, length):
    """7 seeds under a budget that fits 3 per launch; one workgroup per seed."""
    seeds = seeds_of(range(40, 47))
    eng = make_engine(cfg_args, length, sum2_budget_bytes=budget_for_batch(cfg_args, length, 3))
    assert eng.batch_size == 3
    rows = eng.derive_mask_values_batch(seeds)
    assert_rows_equal(rows, cfg_args, seeds, length)
    assert aggregate_on(eng, seeds) == oracle_wire(cfg_args, seeds, length)
    # into a caller's rows, the tail of a larger buffer
    buf = eng.new_rows(9)
    buf.fill_(-1)
    eng.derive_mask_values_batch(seeds, out=buf[2:])
    assert_rows_equal(buf[2:], cfg_args, seeds, length)
    assert bool((buf[:2] == -1).all())


def test_row_groups_of_single_seed_launches():
    """A budget with room for 5 value rows but not for two seeds' candidate
    planes: launches of one seed, plane passes of 5 and 2 rows."""
    seeds = seeds_of(range(40, 47))
    eng = make_engine(PRIME_F32_M3, LENGTH, sum2_budget_bytes=2 * 5 * 8 * LENGTH)
    assert eng.batch_size == 1 and eng.sum2_group == 5
    assert aggregate_on(eng, seeds) == oracle_wire(PRIME_F32_M3, seeds, LENGTH)
    # too few rows for a plane pass: the per-seed mod-add loop
    eng = make_engine(PRIME_F32_M3, LENGTH, sum2_budget_bytes=2 * 2 * 8 * LENGTH)
    assert eng.sum2_group == 2
    assert aggregate_on(eng, seeds) == oracle_wire(PRIME_F32_M3, seeds, LENGTH)


# ---- 4: shortfall


def test_shortfall_is_finished_by_the_single_seed_loop():
    """With attempts for len/2 expected acceptances (sigma ~ 45 against a gap
    of ~2050) every seed of the batch falls short and is completed by the
    single-seed loop from (totals[s], attempts)."""
    from xaynet_amd import _hip

    seeds = seeds_of(SEED_BYTES[:3])
    cfg = mk.MaskConfig(*PRIME_F32_M3)
    eng = make_engine(PRIME_F32_M3, LENGTH)
    p = int(cfg.order) / 2.0 ** (8 * cfg.prng_nbytes)
    attempts = int(LENGTH / (2 * p))
    rows = eng.new_rows(len(seeds))
    rows.fill_(-1)
    words = [mk.unit_draw(s, cfg)[1] for s in seeds]
    with torch.cuda.device(eng.device):
        launched = _hip.MaskExpander().expand(
            b"".join(seeds), rows.data_ptr(), 0, LENGTH, cfg.order, cfg.prng_nbytes, words,
            seed_stride=rows.stride(0), attempts=attempts)
    assert launched > len(seeds) * attempts
    assert_rows_equal(rows, PRIME_F32_M3, seeds, LENGTH)
    # one seed with `attempts`: the same loop from (0, 0)
    one = eng.new_values()
    with torch.cuda.device(eng.device):
        launched = _hip.MaskExpander().expand(
            seeds[1], one.data_ptr(), 0, LENGTH, cfg.order, cfg.prng_nbytes, words[1],
            attempts=attempts)
    assert launched > attempts
    assert_rows_equal(one[None], PRIME_F32_M3, seeds[1:2], LENGTH)


# ---- 5: above the batch rule


def test_above_the_batch_rule_a_batch_is_one_seed():
    length = 300_007  # 2085 candidate workgroups per seed: past the single-workgroup scan
    seeds = seeds_of(SEED_BYTES[:2])
    eng = make_engine(PRIME_F32_M3, length)
    assert eng.batch_size == 1
    rows = eng.derive_mask_values_batch(seeds)
    assert_rows_equal(rows, PRIME_F32_M3, seeds, length)
    assert aggregate_on(eng, seeds) == oracle_wire(PRIME_F32_M3, seeds, length)


# ---- 6: row sum


@pytest.mark.parametrize("cfg_args", [PRIME_F32_M3, PRIME_F32_M6, PRIME_F64_M3, PRIME_F64_B4_M9,
                                      PRIME_I64_BMAX_M12])
def test_add_rows_to_planes_equals_values_to_planes(cfg_args):
    length = 1031  # odd, five 256-thread blocks
    seeds = seeds_of(SEED_BYTES)
    eng = make_engine(cfg_args, length)
    rows = eng.derive_mask_values_batch(seeds)
    start = torch.arange(eng.n_digits * length, dtype=torch.int64, device=eng.device)
    got = start.reshape(eng.n_digits, length).clone()
    want = got.clone()
    eng.add_rows_to_planes(rows, got)
    for s in range(len(seeds)):
        eng.values_to_planes(rows[s], want)
    for d in range(eng.n_digits):
        assert torch.equal(got[d], want[d]), f"plane {d}"
    # one row is the one-row kernel
    eng.add_rows_to_planes(rows[:1], got)
    eng.values_to_planes(rows[0], want)
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        eng.add_rows_to_planes(rows[:, ..., :-1], got)  # rows must be contiguous


# ---- 7: multi-limb orders keep the per-seed loop


def test_multi_limb_config_keeps_the_per_seed_loop():
    from xaynet_amd.ops.sum2 import aggregate_masks

    length = 257
    seeds = seeds_of(SEED_BYTES[:3])
    cfg = mk.MaskConfig(*PRIME_F32_BMAX_M3)
    eng = make_engine(PRIME_F32_BMAX_M3, length)
    assert eng.batch_size == 1
    assert_rows_equal(eng.derive_mask_values_batch(seeds), PRIME_F32_BMAX_M3, seeds, length)
    assert aggregate_masks(seeds, cfg, cfg, length) == oracle_wire(PRIME_F32_BMAX_M3, seeds,
                                                                   length)
