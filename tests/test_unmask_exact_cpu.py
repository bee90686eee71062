"""The exact float unmask without a GPU: the element function of the kernel
(gpu/unmask_round.h) on the host, CpuPlaneAggregator(exact=True) through every
entry form, two gloo ranks, and the settings switch - against the Fraction
reference of tests/unmask_exact_inputs.py, which is pinned to the
exact-rational oracle (_core.mask.Aggregation) here. The CPU twin of
tests/test_gpu_unmask_exact.py."""
import socket
from fractions import Fraction

import numpy as np
import pytest

import unmask_edges as ue
import unmask_exact_inputs as ux
from unmask_exact_inputs import mk

from xaynet_amd import _core


def cpu_engine(rnd):
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    return CpuPlaneAggregator(rnd["vect_cfg"], rnd["unit_cfg"], rnd["n"])


# ------------------------------------------------------- the element function


@pytest.mark.parametrize("entry", ux.CRAFTED, ids=ux.crafted_id)
def test_unmask_round_crafted(entry):
    """ur_round at the config's limb count on the crafted numerators: ties,
    their neighbours, representable quotients, both ends of the range."""
    rnd = ux.craft(*entry)
    n_limbs = ux.LIMBS[entry[0]]
    assert (int(rnd["order"]).bit_length() + 63) // 64 == n_limbs
    out = _core.mask.unmask_round([abs(d) for d in rnd["d"]], [d < 0 for d in rnd["d"]],
                                  rnd["q"], rnd["dtype"], limbs=n_limbs)
    ux.assert_bits_equal(out, rnd["ref"], ux.crafted_id(entry))
    ref = rnd["ref"]
    if entry[1] >= 2**268:  # f32 under a 5-limb order: the subnormal grid is reached
        tiny = np.float32(2.0**-126)
        assert ((np.abs(ref) < tiny) & (ref != 0)).sum() >= 8
        assert (ux.bits(ref) == 0x80000000).any()  # a negative quotient rounded to -0
    if entry[1] == 2**100:
        assert (np.abs(ref) == np.finfo(np.float32).max).sum() >= 8


@pytest.mark.parametrize("n_limbs", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("np_type", [np.float32, np.float64], ids=["f32", "f64"])
def test_unmask_round_random(n_limbs, np_type):
    """A few thousand (mag, q) pairs of every bit length up to the full limb
    width, both signs."""
    pairs = ux.random_pairs(n_limbs, 3000, seed=100 + n_limbs)
    code = ux.DTYPE_CODE[np_type]
    got = np.concatenate([_core.mask.unmask_round([mag], [i & 1], q, code, limbs=n_limbs)
                          for i, (mag, q) in enumerate(pairs)])
    want = np.array([ux.round_exact(Fraction(-mag if i & 1 else mag, q), np_type)
                     for i, (mag, q) in enumerate(pairs)], dtype=np_type)
    # mag == 0 is +0 whatever the sign asked for
    want[[i for i, (mag, _) in enumerate(pairs) if mag == 0]] = 0.0
    ux.assert_bits_equal(got, want, f"L={n_limbs}")


def test_unmask_round_refuses():
    for args in (([1], [False], 0, 0), ([1], [False], -3, 0), ([1], [False], 2**320, 0),
                 ([2**320], [False], 1, 0), ([-1], [False], 1, 0), ([1], [False], 1, 2),
                 ([1, 2], [False], 1, 0)):
        with pytest.raises(ValueError):
            _core.mask.unmask_round(*args)
    with pytest.raises(ValueError):  # two limbs do not hold 2^128
        _core.mask.unmask_round([2**128], [False], 1, 0, limbs=2)
    assert _core.mask.unmask_round([], [], 1, 1).shape == (0,)


def test_round_exact_is_round_once():
    """The reference here is unmask_edges.round_once inside the normal range."""
    rng = np.random.default_rng(7)
    for np_type in (np.float32, np.float64):
        for _ in range(500):
            q = Fraction(int(rng.integers(-2**62, 2**62)), int(rng.integers(1, 2**62)))
            assert ux.bits(np.array([ux.round_exact(q, np_type)]))[0] == \
                ux.bits(np.array([ue.round_once(q, np_type)], dtype=np_type))[0]


# ------------------------------------------------- the reference is the oracle


@pytest.mark.parametrize("cfg_args", [(1, 0, 4, 3), (1, 1, 4, 9), (1, 0, 255, 3)],
                         ids=["f32-b4", "f64-b4", "f32-bmax"])
def test_reference_is_the_oracle(cfg_args):
    """mask_model + Aggregation on real MaskObjects: the rationals the oracle
    unmasks are Fraction(d, Q) with d = t - C and Q = n1 - nb * add_1 * exp_1,
    and _unmask_scalars derives that offset and divisor."""
    n, scalars = 48, ((1, 3), (1, 5), (1, 7))
    cfg = mk.MaskConfig(*cfg_args)
    pair = mk.MaskConfigPair(cfg, cfg)
    order = int(cfg.order)
    add, exp = ux.shifts(cfg_args)
    np_type = ue.NP_DTYPES[cfg_args[1]]
    rng = np.random.default_rng(11)
    agg, mask_agg = mk.Aggregation(pair, n), mk.Aggregation(pair, n)
    for j, (num, den) in enumerate(scalars):
        seed = bytes([j + 1]) * 32
        w = rng.normal(0, 0.5, n).astype(np_type)
        w[:3] = (0.0, 1e-9, -1e-9)
        agg.aggregate(mk.mask_model(seed, mk.Scalar(num, den), w, pair))
        mask_agg.aggregate(mk.derive_mask(seed, n, pair))
    nb = len(scalars)
    c = nb * add * exp
    n1 = (int(agg.object.unit_value) - int(mask_agg.object.unit_value)) % order
    q = n1 - c  # the same config twice: exp_shift / exp_1 == 1
    assert q > 0
    rationals = agg.unmask_rationals(mask_agg.object)
    assert len(rationals) == n
    for i, (num, den) in enumerate(rationals):
        t = (int(agg.object.element(i)) - int(mask_agg.object.element(i))) % order
        assert Fraction(int(num), int(den)) == Fraction(t - c, q), f"element {i}"
    eng = cpu_engine({"vect_cfg": cfg, "unit_cfg": cfg, "n": n})
    eng.unit_acc = int(agg.object.unit_value)
    _, vinfo, _ = eng._unmask_scalars(int(mask_agg.object.unit_value), nb)
    assert (vinfo["offset"], vinfo["exact_divisor"]) == (c, q)


# --------------------------------------------------------- CpuPlaneAggregator


@pytest.mark.parametrize("case", ue.FLOAT_CASES, ids=ue.case_id)
def test_cpu_plane_forged_exact(case):
    """The existing float cases: every entry form with exact=True is the
    once-rounded quotient bit for bit, which the double steps are not."""
    rnd = ux.forged(case)
    if case[0] == (1, 1, 4, 9):
        ux.assert_double_steps_miss(rnd, 0.5)
    else:
        ux.assert_double_steps_miss(rnd, 0.005)
    eng = cpu_engine(rnd)
    outs = ux.unmask_forms(eng, rnd)
    assert set(outs) == {"unmask", "unmask_planes", "shards",
                         "compact_planes" if eng.wide else "unmask_values"}
    for form, out in outs.items():
        ux.assert_bits_equal(out, rnd["ref"], form)
    # default calls are unchanged: with and without the keyword, and they are
    # the double steps (which miss the reference)
    default = ue.unmask_forms(eng, rnd)
    for form, out in ux.unmask_forms(eng, rnd, exact=False).items():
        ux.assert_bits_equal(out, default[form], form)
    assert (ux.bits(default["unmask"]) != ux.bits(rnd["ref"])).any()
    err = np.abs(default["unmask"].astype(np.float64) - rnd["ref"].astype(np.float64))
    assert (err <= ue.float_bound(rnd)).all()


@pytest.mark.parametrize("entry", ux.CRAFTED, ids=ux.crafted_id)
def test_cpu_plane_crafted_exact(entry):
    rnd = ux.craft(*entry)
    eng = cpu_engine(rnd)
    assert eng.n_limbs == ux.LIMBS[entry[0]]
    for form, out in ux.unmask_forms(eng, rnd).items():
        ux.assert_bits_equal(out, rnd["ref"], form)
    eng.unit_acc = rnd["unit_acc"]
    f32 = eng.unmask_f32(ue.values_tensor(eng, rnd["mask"]), rnd["mask_unit"], rnd["nb"],
                         exact=True).numpy()
    want = np.array([ux.round_exact(x, np.float32) for x in rnd["quotients"]], dtype=np.float32)
    ux.assert_bits_equal(f32, want, "unmask_f32")


def test_exact_mode_refusals():
    """ValueError where exact mode does not apply; nothing else changes."""
    # different exp_shift for the vector (F32) and the unit (F64) config
    rnd = ue.forge((1, 0, 4, 3), (1, 1, 4, 3), ue.equal_scalars(3))
    eng = cpu_engine(rnd)
    eng.unit_acc = rnd["unit_acc"]
    assert eng._unmask_scalars(rnd["mask_unit"], rnd["nb"])[1]["exact_divisor"] is None
    with pytest.raises(ValueError, match="exact unmask"):
        ux.unmask_forms(eng, dict(rnd, dtype=0))
    ue.unmask_forms(eng, rnd)  # the default mode still runs

    # a negative scalar sum
    rnd = ux.forged(ue.FLOAT_CASES[0])
    eng = cpu_engine(rnd)
    eng.unit_acc = (rnd["offset"] - 5 + rnd["mask_unit"]) % rnd["order"]
    mask = ue.values_tensor(eng, rnd["mask"])
    with pytest.raises(ValueError, match="exact unmask"):
        eng.unmask(mask, rnd["mask_unit"], nb_models=rnd["nb"], exact=True)

    # an integer model without an exact divisor: only the double steps
    vect, unit, scalars = ue.NO_DIVISOR_CASE
    rnd = ue.forge(vect, unit, scalars)
    eng = cpu_engine(rnd)
    with pytest.raises(ValueError, match="integer model"):
        ux.unmask_forms(eng, dict(rnd, dtype=None))

    # an integer model with one: exact mode is the default path
    cfg, scalars = ue.INTEGER_CASES[0]
    rnd = ue.forge(cfg, cfg, scalars)
    eng = cpu_engine(rnd)
    for form, out in ux.unmask_forms(eng, dict(rnd, dtype=None)).items():
        assert (out == rnd["ref"]).all(), form


def test_unmask_scalars_keeps_the_one_word_divisor():
    """`divisor` stays below 2^64 (integer outputs depend on it);
    `exact_divisor` is the same integer at any size the limbs hold."""
    rnd = ux.craft((1, 0, 255, 3), 2**270, np.float32)
    eng = cpu_engine(rnd)
    eng.unit_acc = rnd["unit_acc"]
    _, vinfo, _ = eng._unmask_scalars(rnd["mask_unit"], rnd["nb"])
    assert vinfo["divisor"] is None and vinfo["exact_divisor"] == 2**270
    rnd = ux.craft((1, 0, 4, 3), 2**20, np.float32)
    eng = cpu_engine(rnd)
    eng.unit_acc = rnd["unit_acc"]
    _, vinfo, _ = eng._unmask_scalars(rnd["mask_unit"], rnd["nb"])
    assert vinfo["divisor"] == vinfo["exact_divisor"] == 2**20


# -------------------------------------------------------------------- sharded

# (config, divisor, output type, length): values-RS on a u64 order, compact
# digits-RS on a wide one, and the all-reduce an odd length falls back to
SHARDED = [
    ((1, 0, 4, 3), 3 * 5**5 * 2**9, np.float32, 1026, "values_rs"),
    ((1, 1, 4, 9), 5 * 2**58, np.float64, 1026, "digits_rs"),
    ((1, 1, 4, 9), 2**60, np.float32, 1027, "all_reduce"),
]


def _gloo_worker(rank: int, world: int, port: int):
    import torch.distributed as dist

    from xaynet_amd.parallel import ShardedAggregation

    dist.init_process_group(
        "gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world
    )
    try:
        for cfg_args, q, np_type, n, strategy in SHARDED:
            rnd = ux.craft(cfg_args, q, np_type, n=n)
            order = rnd["order"]
            eng = cpu_engine(rnd)
            # the masked sums split into two canonical shares, one per rank
            rng = np.random.default_rng(3)
            share0 = [int(x) % order for x in rng.integers(0, 2**62, n)]
            share = share0 if rank == 0 else [(v - a) % order
                                              for v, a in zip(rnd["masked"], share0)]
            eng.values_to_planes(ue.values_tensor(eng, share), eng.acc)
            eng.unit_acc = rnd["unit_acc"]
            sharded = ShardedAggregation(eng, dist, rank, world)
            assert sharded.strategy == strategy
            mask = ue.values_tensor(eng, rnd["mask"])
            # f32 output of the f64 config goes through the engine's dtype
            # default only for the config's own type: the all-reduce case
            # checks the config's type against its own reference
            want = rnd["ref"] if rnd["dtype"] == cfg_args[1] else np.array(
                [ux.round_exact(x, ue.NP_DTYPES[cfg_args[1]]) for x in rnd["quotients"]],
                dtype=ue.NP_DTYPES[cfg_args[1]])
            out = sharded.unmask_global(mask, rnd["mask_unit"], rnd["nb"], exact=True).numpy()
            ux.assert_bits_equal(out, want, f"rank {rank} {strategy}")
            # the single engine on the whole sum gives the same bits
            single = cpu_engine(rnd)
            single.values_to_planes(ue.values_tensor(single, rnd["masked"]), single.acc)
            single.unit_acc = rnd["unit_acc"]
            one = single.unmask(mask, rnd["mask_unit"], nb_models=rnd["nb"], exact=True).numpy()
            ux.assert_bits_equal(out, one, f"rank {rank} {strategy} vs single")
    finally:
        dist.destroy_process_group()


def test_gloo_sharded_exact():
    """Two gloo ranks with exact=True give the single-engine exact result bit
    for bit, through values-RS, digits-RS and all-reduce."""
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_gloo_worker, args=(2, port), nprocs=2, join=True)


# ------------------------------------------------------------------- settings


def test_settings_exact_unmask():
    from xaynet_amd.server.settings import Settings, _apply_env_overrides

    assert Settings().gpu_exact_unmask is False
    assert Settings._from_dict({"gpu": {"enable": True}}).gpu_exact_unmask is False
    assert Settings._from_dict({"gpu": {"exact_unmask": True}}).gpu_exact_unmask is True
    raw = {"gpu": {"enable": True}}
    _apply_env_overrides(raw, {"XAYNET__GPU__EXACT_UNMASK": "true"})
    s = Settings._from_dict(raw)
    assert s.gpu and s.gpu_exact_unmask is True
    raw = {"gpu": {"exact_unmask": True}}
    _apply_env_overrides(raw, {"XAYNET__GPU__EXACT_UNMASK": "false"})
    assert Settings._from_dict(raw).gpu_exact_unmask is False


def test_drivers_take_the_flag():
    """Both drivers expose exact_unmask, off by default (no GPU needed to look)."""
    import inspect

    from xaynet_amd.ops.driver import GpuCoordinatorDriver
    from xaynet_amd.parallel import ShardedAggregation
    from xaynet_amd.parallel.serve import MultiGpuServeDriver, ServePlane

    for cls in (GpuCoordinatorDriver, MultiGpuServeDriver):
        assert inspect.signature(cls.__init__).parameters["exact_unmask"].default is False
    assert inspect.signature(ServePlane.unmask).parameters["exact"].default is False
    assert inspect.signature(ShardedAggregation.unmask_global).parameters["exact"].default is False


def test_serve_plane_exact_and_fallback():
    """One serve-plane round on two CPU workers with exact=True: the exact
    result; and where the engines refuse, the default result with a log line
    in the worker (the round still completes)."""
    from xaynet_amd.parallel.serve import ServePlane

    cfg_args, q, np_type, n = (1, 1, 4, 9), 5 * 2**58, np.float64, 1026
    rnd = ux.craft(cfg_args, q, np_type, n=n)
    eng = cpu_engine(rnd)
    update = eng.pack_wire(ue.values_tensor(eng, rnd["masked"])).numpy().tobytes()
    mask = eng.pack_wire(ue.values_tensor(eng, rnd["mask"])).numpy().tobytes()
    plane = ServePlane(cfg_args, n, 2, "cpu", slots_per_worker=4, batch=2)
    try:
        plane.put_update(update)
        out = plane.unmask(mask, rnd["mask_unit"], rnd["unit_acc"], rnd["nb"], round_id=1,
                           exact=True)
        ux.assert_bits_equal(out, rnd["ref"], "serve plane")
        # a negative scalar sum: exact mode is refused, the default runs
        plane.put_update(update)
        bad_acc = (rnd["offset"] - 10**19 + rnd["mask_unit"]) % rnd["order"]
        out = plane.unmask(mask, rnd["mask_unit"], bad_acc, rnd["nb"], round_id=2, exact=True)
        eng.values_to_planes(ue.values_tensor(eng, rnd["masked"]), eng.acc)
        eng.unit_acc = bad_acc
        want = eng.unmask(ue.values_tensor(eng, rnd["mask"]), rnd["mask_unit"],
                          nb_models=rnd["nb"]).numpy()
        ux.assert_bits_equal(out, want, "serve plane fallback")
    finally:
        plane.stop()
