"""Bmax mask configs (group orders up to 2^320) without a GPU.

The config scalars are exact integers, the CPU plane carries values as
[n_limbs, n] limb rows and unmasks with the exact-offset arithmetic of the GPU
K4, and the world-2 composition shards it. Everything is checked against the
exact-rational oracle (_core.mask.Aggregation)."""
import functools
import socket

import numpy as np
import pytest
import torch

from xaynet_amd import _core

mk = _core.mask

LENGTH = 33
K = 3  # participants, scalar 1/3: the masked scalars sum to 0.9999999999

# (config, bytes per number, limb rows)
ROUND_CASES = [
    ((1, 2, 255, 3), 10, 2),   # Prime/I32/Bmax/M3
    ((1, 3, 255, 3), 14, 2),   # Prime/I64/Bmax/M3
    ((1, 3, 255, 12), 18, 3),  # Prime/I64/Bmax/M12
    ((1, 0, 255, 3), 37, 5),   # Prime/F32/Bmax/M3
    ((2, 0, 255, 12), 40, 5),  # Pow2/F32/Bmax/M12
    ((2, 3, 255, 9), 16, 3),   # Pow2/I64/Bmax/M9: the order is 2^128 itself
]


def test_cfg_scalars_bmax_are_exact_ints():
    from xaynet_amd.ops.base import _cfg_scalars

    expect = {
        0: (10**45, (2**24 - 1) * 2**104),
        2: (10**10, 2**31),
        3: (10**10, 2**63),
    }
    for dtype, (exp, add) in expect.items():
        for group, model in ((1, 3), (2, 12)):
            info = _cfg_scalars(mk.MaskConfig(group, dtype, 255, model))
            for key in ("exp_shift", "exp_shift_u64", "add_shift"):
                assert type(info[key]) is int, (dtype, key)
            assert info["exp_shift"] == info["exp_shift_u64"] == exp
            assert info["add_shift"] == add
    with pytest.raises(ValueError, match="CPU oracle"):
        _cfg_scalars(mk.MaskConfig(1, 1, 255, 3))  # F64 Bmax stays on the oracle
    # the other bounds keep their float forms
    info = _cfg_scalars(mk.MaskConfig(1, 0, 2, 3))
    assert info == {"exp_shift": 1e10, "exp_shift_u64": 10**10, "add_shift": 100.0}
    assert type(info["exp_shift"]) is float and type(info["add_shift"]) is float


def _weights(cfg, length, rng):
    if cfg.dtype == 2:
        return rng.integers(-2**31, 2**31, length).astype(np.int32)
    if cfg.dtype == 3:
        return rng.integers(-2**50, 2**50 + 1, length).astype(np.int64)
    # magnitudes 1e-3 .. 1e30, both signs; element i has the same decade in
    # every update, so the small weights survive the mean
    decade = 10.0 ** np.random.default_rng(length).uniform(-3, 30, length)
    return (rng.choice([-1.0, 1.0], length) * rng.uniform(0.5, 1.0, length) * decade).astype(
        np.float32)


@functools.lru_cache(maxsize=None)
def forge_round(cfg_args, length, k):
    """k CPU-masked updates, their masks and the oracle's unmasked model;
    computed once per shape and shared (read-only) by the tests."""
    cfg = mk.MaskConfig(*cfg_args)
    pair = mk.MaskConfigPair(cfg, cfg)
    order, bpn = int(cfg.order), cfg.bytes_per_number
    rng = np.random.default_rng(11)
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
    return {
        "cfg": cfg, "updates": updates, "masks": masks, "unit_acc": unit_acc,
        "mask_vect": bytes(mask_agg.object.serialize())[8 : 8 + length * bpn],
        "mask_unit": int(mask_agg.object.unit_value),
        "oracle": np.asarray(agg.unmask(mask_agg.object)),
        "elements": [int(agg.object.element(i)) for i in range(length)],
    }


def _as_tensor(wire: bytes) -> torch.Tensor:
    return torch.frombuffer(bytearray(wire), dtype=torch.uint8)


def assert_matches_oracle(cfg, out, oracle):
    """Integer models exactly; f32 within one rounding step of the oracle's
    own f32 (both round a double that is good to ~2^-51)."""
    assert out.dtype == oracle.dtype and out.shape == oracle.shape
    if cfg.dtype in (2, 3):
        assert (out == oracle).all(), f"{(out != oracle).sum()} mismatches vs oracle"
    else:
        assert np.isfinite(out).all()
        err = np.abs(out.astype(np.float64) - oracle.astype(np.float64))
        assert (err <= np.spacing(np.abs(oracle))).all(), err.max()


def _load_engine(rnd, length, which):
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    eng = CpuPlaneAggregator(rnd["cfg"], rnd["cfg"], length)
    pool = eng.alloc_update_pool(len(which))
    for row, p in enumerate(which):
        eng.upload_update(pool, row, rnd["updates"][p])
    eng.aggregate_pool(pool, len(which))
    eng.unit_acc = rnd["unit_acc"]
    return eng


@pytest.mark.parametrize("cfg_args,bpn,n_limbs", ROUND_CASES)
def test_cpu_plane_round_vs_oracle(cfg_args, bpn, n_limbs):
    rnd = forge_round(cfg_args, LENGTH, K)
    cfg = rnd["cfg"]
    eng = _load_engine(rnd, LENGTH, range(K))
    assert (eng.bpn, eng.n_limbs, eng.wide) == (bpn, n_limbs, True)
    assert eng.new_values().shape == (n_limbs, LENGTH)

    # the limb-row layout: canonical values, the wire codec and the mask sum
    canon = eng.canonical()
    assert canon.shape == (n_limbs, LENGTH)
    assert [int(v) for v in eng._ints(canon)] == rnd["elements"]
    assert torch.equal(eng.unpack_wire(eng.pack_wire(canon)), canon)
    mask = eng.new_values(zero=True)
    for m in rnd["masks"]:
        eng.mod_add_values(mask, eng.unpack_wire(_as_tensor(m)))
    assert torch.equal(mask, eng.unpack_wire(_as_tensor(rnd["mask_vect"])))

    out = eng.unmask(mask, rnd["mask_unit"]).numpy()
    oracle = rnd["oracle"]
    if cfg.dtype in (2, 3):
        assert np.abs(oracle).max() > 2**(29 if cfg.dtype == 2 else 47)
    else:
        assert np.abs(oracle).max() > 1e27 and np.abs(oracle).min() < 0.1
    assert_matches_oracle(cfg, out, oracle)


def test_unit_scalars_exact_for_bmax():
    """masked_unit_for and scalar_sum in exact integers: k masked scalars of
    1/k on a Bmax unit config sum to 0.9999999999 (I64) exactly."""
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    cfg = mk.MaskConfig(1, 3, 255, 3)
    eng = CpuPlaneAggregator(cfg, cfg, 4)
    order, mask_unit = int(cfg.order), 0
    for p in range(K):
        seed = bytes([p + 1]) * 32
        eng.unit_acc = (eng.unit_acc + eng.masked_unit_for(seed, 1, K)) % order
        mask_unit = (mask_unit + eng.unit_draw(seed)) % order
    scalar_sum, vinfo, dt = eng._unmask_scalars(mask_unit, K)
    assert scalar_sum == 0.9999999999 and dt == 3
    assert vinfo["offset"] == K * 2**63 * 10**10
    assert vinfo["divisor"] == 9999999999


def _gloo_worker(rank: int, world: int, port: int, cfg_args, length):
    import torch.distributed as dist

    from xaynet_amd.parallel import ShardedAggregation

    dist.init_process_group(
        "gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world
    )
    try:
        rnd = forge_round(cfg_args, length, K)
        cfg = rnd["cfg"]
        mine = list(range(rank, K, world))
        eng = _load_engine(rnd, length, mine)
        assert eng.n_limbs == 5

        sharded = ShardedAggregation(eng, dist, rank, world)
        assert sharded.strategy == ("digits_rs" if length % world == 0 else "all_reduce")

        partial = eng.new_values(zero=True)
        for p in mine:
            eng.mod_add_values(partial, eng.unpack_wire(_as_tensor(rnd["masks"][p])))
        mask_total = sharded.allreduce_mask(partial)
        expect_mask = eng.unpack_wire(_as_tensor(rnd["mask_vect"]))
        assert torch.equal(mask_total, expect_mask), f"rank {rank}: mask all-reduce"

        out = sharded.unmask_global(mask_total, rnd["mask_unit"], K).numpy()
        assert_matches_oracle(cfg, out, rnd["oracle"])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("length", [LENGTH, LENGTH + 1])
def test_gloo_bmax_sharded_round(length):
    """world-2 round of Prime/F32/Bmax/M3 over CPU engines: 33 elements do not
    shard evenly (plane all-reduce), 34 take the compact-digit reduce-scatter
    with its five planes."""
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    world = 2
    mp.spawn(_gloo_worker, args=(world, port, (1, 0, 255, 3), length), nprocs=world, join=True)


def test_compact_digits_multi_limb():
    from xaynet_amd.parallel import choose_reduce_strategy, compact_digits

    for cfg_args, bits in (((1, 3, 255, 12), 138), ((1, 0, 255, 3), 289), ((2, 0, 255, 12), 320)):
        order = int(mk.MaskConfig(*cfg_args).order)
        assert order.bit_length() == bits  # Pow2 M12: 2^319 itself
        for world in (2, 8, 64):
            k, w = compact_digits(order, world)
            assert world * (2**w - 1) < 2**63 and k * w >= order.bit_length()
            assert choose_reduce_strategy(world, world * 8, order, env={}) == "digits_rs"


def test_orders_beyond_320_bits_stay_loud():
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    cfg = mk.MaskConfig(1, 1, 255, 3)  # F64 Bmax: 264 bytes per number
    with pytest.raises(ValueError, match="CPU oracle"):
        CpuPlaneAggregator(cfg, cfg, 8)


def _serve_briefly(settings):
    """Start the daemon, wait until it serves, stop it."""
    import threading

    from xaynet_amd.server import serve

    ready, stop = threading.Event(), threading.Event()
    t = threading.Thread(target=serve, args=(settings, ready, stop), daemon=True)
    t.start()
    try:
        assert ready.wait(20)
    finally:
        stop.set()
        t.join(20)
    assert not t.is_alive()


def bmax_daemon_settings(data_type):
    from xaynet_amd.server import Settings

    s = Settings()
    s.api.bind_address = "127.0.0.1:0"
    s.model_length = 16
    s.mask.data_type, s.mask.bound_type = data_type, "Bmax"
    s.gpu, s.gpu_devices = True, 1
    s.validate()
    return s


def test_server_keeps_f64_bmax_on_the_cpu_plane(caplog):
    """F64 Bmax is the one config the daemon still takes off the GPU plane,
    and the warning says so."""
    settings = bmax_daemon_settings("F64")
    with caplog.at_level("WARNING", logger="xaynet.server"):
        _serve_briefly(settings)
    assert settings.gpu is False
    assert any("F64 Bmax" in r.getMessage() for r in caplog.records)


# ------------------------------------------------------------- binding forms

HI = 0x1000  # a non-null "pointer": len == 0, so it is never dereferenced


def test_binding_forms_up_to_320_bits():
    _hip = pytest.importorskip("xaynet_amd._hip", reason="_hip extension not built")
    top, beyond = str(2**319), str(2**320)
    calls = {
        "canonicalize": lambda o: _hip.canonicalize(0, 0, HI, 0, 10, o),
        "add_to_planes": lambda o: _hip.add_to_planes(0, 0, HI, 0, 10, o),
        "mod_add": lambda o: _hip.mod_add(0, HI, 0, HI, 0, o),
        "recode_planes": lambda o: _hip.recode_planes(0, 0, 0, 10, o, 6, 54),
        "unmask": lambda o: _hip.unmask(0, 0, HI, 0, 0, 10, o, str(10**45), 0.0, 1.0, 0,
                                        offset=str(3 * (2**24 - 1) * 2**104 * 10**45)),
        "mask_weights": lambda o: _hip.mask_weights(
            0, 0, 0, HI, 0, 0, 40, o, 1.0, 3.4e38, str(10**45),
            offset=str((2**24 - 1) * 2**104 * 10**45)),
        "pack": lambda o: _hip.pack(0, HI, 0, 0, 40, o),
        "unpack": lambda o: _hip.unpack(0, 0, HI, 0, 40, o),
        "expand": lambda o: _hip.MaskExpander().expand(b"\0" * 32, 0, HI, 0, o, 40, 0),
    }
    for name, call in calls.items():
        call(top)  # 2^319 with a non-null hi passes the form check
        with pytest.raises(ValueError):
            call(beyond)
    # the width rule is unchanged: hi is non-null iff order >= 2^64
    with pytest.raises(ValueError):
        _hip.canonicalize(0, 0, 0, 0, 10, top)
    # expand: 17..40 draw bytes for such orders
    for nbytes in (16, 41):
        with pytest.raises(ValueError):
            _hip.MaskExpander().expand(b"\0" * 32, 0, HI, 0, top, nbytes, 0)
    # orders >= 2^128 exist only as Bmax configs: no unmask without the offset
    with pytest.raises(ValueError):
        _hip.unmask(0, 0, HI, 0, 0, 10, top, str(10**45), 0.0, 1.0, 0)
    with pytest.raises(ValueError):
        _hip.mask_pack(0, HI, 0, 0, 40, top, 0, 1.0, 1.0, str(10**45))
