"""Bmax mask configs on the GPU: group orders up to 2^320.

Canonical values are [n_limbs, n] rows of u64 limbs (3 rows for the 138-bit
i64 M12 order, 5 for the 289..320-bit f32 orders), the accumulator has 5 or 10
digit planes, and every Bmax config — the narrow i32/i64 ones included —
unmasks through the exact-offset K4. Everything is checked against the CPU
engine or the exact-rational oracle (_core.mask.Aggregation).

Inputs are CPU `mask_model` updates uploaded as wire limbs and masks from
`unpack_wire` of the CPU-derived mask wire; each round is forged once and
shared read-only."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from xaynet_amd import _core  # noqa: E402

mk = _core.mask

pytestmark = pytest.mark.gpu

LENGTH = 1499  # odd, no multiple of any K3 elements-per-thread, 6 workgroups
K = 3          # participants, scalar 1/3: the masked scalars sum to 0.9999999999

PRIME_F32_M3 = (1, 0, 255, 3)    # 289-bit order, bpn 37, acceptance 0.5%
POW2_F32_M12 = (2, 0, 255, 12)   # order 2^319, bpn 40, acceptance 50%
PRIME_I64_M12 = (1, 3, 255, 12)  # 138-bit order, bpn 18, acceptance 0.8%

ROUND_CASES = [
    ((1, 2, 255, 3), 10, 2),   # Prime/I32/Bmax/M3
    ((1, 3, 255, 3), 14, 2),   # Prime/I64/Bmax/M3
    (PRIME_I64_M12, 18, 3),
    (PRIME_F32_M3, 37, 5),
    (POW2_F32_M12, 40, 5),
    ((2, 3, 255, 9), 16, 3),   # Pow2/I64/Bmax/M9: order 2^128 itself, 17-byte draws
]


def make_engine(cfg_args, length):
    from xaynet_amd.ops import GpuMaskedAggregator, gpu_available

    if not gpu_available():
        pytest.fail("GPU expected for -m gpu tests but not available")
    cfg = mk.MaskConfig(*cfg_args)
    return GpuMaskedAggregator(cfg, cfg, length)


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
def forge_round(cfg_args, length=LENGTH, k=K):
    cfg = mk.MaskConfig(*cfg_args)
    pair = mk.MaskConfigPair(cfg, cfg)
    order, bpn = int(cfg.order), cfg.bytes_per_number
    rng = np.random.default_rng(12)
    agg, mask_agg = mk.Aggregation(pair, length), mk.Aggregation(pair, length)
    seeds, weights, updates, unit_acc = [], [], [], 0
    for _ in range(k):
        seed = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        w = _weights(cfg, length, rng)
        masked = mk.mask_model(seed, mk.Scalar(1, k), w, pair)
        agg.aggregate(masked)
        mask_agg.aggregate(mk.derive_mask(seed, length, pair))
        seeds.append(seed)
        weights.append(w)
        updates.append(bytes(masked.serialize())[8 : 8 + length * bpn])
        unit_acc = (unit_acc + int(masked.unit_value)) % order
    return {
        "cfg_args": cfg_args, "cfg": cfg, "length": length, "k": k, "seeds": seeds,
        "weights": weights, "updates": updates, "unit_acc": unit_acc,
        "mask_vect": bytes(mask_agg.object.serialize())[8 : 8 + length * bpn],
        "mask_unit": int(mask_agg.object.unit_value),
        "oracle": np.asarray(agg.unmask(mask_agg.object)),
        "elements": np.array([int(agg.object.element(i)) for i in range(length)], dtype=object),
    }


def load_engine(rnd, which=None):
    """Engine holding the aggregate of the updates in `which` (default all)."""
    eng = make_engine(rnd["cfg_args"], rnd["length"])
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


def limb_rows(wire: bytes, n: int, bpn: int, n_limbs: int) -> np.ndarray:
    """Wire limbs -> the [n_limbs, n] int64 rows the engine keeps."""
    padded = np.zeros((n, 8 * n_limbs), dtype=np.uint8)
    padded[:, :bpn] = np.frombuffer(wire, dtype=np.uint8).reshape(n, bpn)
    return np.ascontiguousarray(padded.view("<u8").T).astype(np.int64)


def to_ints(rows_dev) -> np.ndarray:
    rows = rows_dev.cpu().numpy().view(np.uint64)
    total = np.zeros(rows.shape[1], dtype=object)
    for j in reversed(range(rows.shape[0])):
        total = (total << 64) + rows[j].astype(object)
    return total


def assert_matches_oracle(cfg, out, oracle):
    """Integer models exactly. f32: the double pipeline is good to ~2^-51
    relative, so its f32 rounding is at most one step from the oracle's."""
    assert out.dtype == oracle.dtype and out.shape == oracle.shape
    if cfg.dtype in (2, 3):
        assert (out == oracle).all(), f"{(out != oracle).sum()} mismatches vs oracle"
    else:
        assert np.isfinite(out).all()
        err = np.abs(out.astype(np.float64) - oracle.astype(np.float64))
        assert (err <= np.spacing(np.abs(oracle))).all(), err.max()


# ------------------------------------------------------------------------ K1


@pytest.mark.parametrize("cfg_args,length", [
    (PRIME_F32_M3, 1),     # one value out of ~190 draws
    (PRIME_F32_M3, 257),
    (PRIME_F32_M3, 1499),  # ~280k draws: most candidate workgroups accept nothing
    (POW2_F32_M12, 1499),
    (PRIME_I64_M12, 1499),  # 5-word draws, 3 per thread
])
def test_k1_multi_limb_bit_exact(cfg_args, length):
    eng = make_engine(cfg_args, length)
    seed = bytes(range(7, 39))
    got = eng.derive_mask_values(seed)
    assert got.shape == (eng.n_limbs, length)
    pair = mk.MaskConfigPair(eng.vect_cfg, eng.unit_cfg)
    oracle = mk.derive_mask(seed, length, pair)
    expect = limb_rows(bytes(oracle.vect_bytes), length, eng.bpn, eng.n_limbs)
    assert np.array_equal(got.cpu().numpy(), expect)


def test_k1_attempt_cap_loops():
    """More elements than one capped launch (2^22 attempts) yields at 0.5%
    acceptance: the expander loops, and the values stay the oracle's at the
    launch seams."""
    length = 30_000  # ~5.7M draws, two launches
    eng = make_engine(PRIME_F32_M3, length)
    seed = bytes(range(3, 35))
    got = eng.derive_mask_values(seed).cpu().numpy()
    pair = mk.MaskConfigPair(eng.vect_cfg, eng.unit_cfg)
    oracle = mk.derive_mask(seed, length, pair)
    expect = limb_rows(bytes(oracle.vect_bytes), length, eng.bpn, eng.n_limbs)
    assert np.array_equal(got, expect)


# ------------------------------------------------------------------------ K3


@pytest.mark.parametrize("cfg_args,bpn", [
    (PRIME_I64_M12, 18), (PRIME_F32_M3, 37), ((1, 0, 255, 6), 38), ((1, 0, 255, 9), 39),
    (POW2_F32_M12, 40),
])
def test_k3_planes_vs_cpu_engine(cfg_args, bpn):
    """5 and 10 digit planes of 3 updates of arbitrary limbs, twice (the
    second batch adds to the first)."""
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    eng = make_engine(cfg_args, LENGTH)
    assert eng.bpn == bpn and eng.n_digits == (bpn + 3) // 4
    cpu = CpuPlaneAggregator(eng.vect_cfg, eng.unit_cfg, LENGTH)
    rng = np.random.default_rng(bpn)
    pool_cpu = cpu.alloc_update_pool(K)
    pool_cpu.copy_(torch.from_numpy(rng.integers(0, 256, tuple(pool_cpu.shape), dtype=np.uint8)))
    pool = pool_cpu.to("cuda")
    for _ in range(2):
        eng.aggregate_pool(pool, K)
        cpu.aggregate_pool(pool_cpu, K)
    assert torch.equal(eng.acc.cpu(), cpu.acc)


# ---------------------------------------------------------------- full round


@pytest.mark.parametrize("cfg_args,bpn,n_limbs", ROUND_CASES)
def test_full_round_vs_oracle(cfg_args, bpn, n_limbs):
    """K6 unpack, K3, K2 canonicalize / mod_add / pack and the exact-offset
    K4 on one round."""
    rnd = forge_round(cfg_args)
    eng = load_engine(rnd)
    assert (eng.bpn, eng.n_limbs) == (bpn, n_limbs)

    canon = eng.canonical()
    assert canon.shape == (n_limbs, LENGTH)
    assert (to_ints(canon) == rnd["elements"]).all()
    assert torch.equal(eng.unpack_wire(eng.pack_wire(canon)), canon)

    pair = mk.MaskConfigPair(rnd["cfg"], rnd["cfg"])
    mask = eng.new_values(zero=True)
    for seed in rnd["seeds"]:
        m = bytes(mk.derive_mask(seed, LENGTH, pair).vect_bytes)
        eng.mod_add_values(mask, unpack(eng, m))
    assert torch.equal(mask, unpack(eng, rnd["mask_vect"]))

    out = eng.unmask(mask, rnd["mask_unit"]).cpu().numpy()
    assert_matches_oracle(rnd["cfg"], out, rnd["oracle"])


def test_integer_unmask_without_exact_divisor():
    """Without the exact divisor (here: withheld) integer outputs take the
    double steps of k4_unmask_u128 and equal the CPU plane doing the same."""
    from xaynet_amd.ops.cpu_engine import CpuPlaneAggregator

    rnd = forge_round(PRIME_I64_M12)
    eng = load_engine(rnd)
    cpu = CpuPlaneAggregator(rnd["cfg"], rnd["cfg"], LENGTH)
    cpu.unit_acc = rnd["unit_acc"]
    for e in (eng, cpu):
        scalars = e._unmask_scalars

        def no_divisor(*args, _scalars=scalars):
            scalar_sum, vinfo, dt = _scalars(*args)
            vinfo["divisor"] = None
            return scalar_sum, vinfo, dt

        e._unmask_scalars = no_divisor
    mask = unpack(eng, rnd["mask_vect"])
    out = eng.unmask(mask, rnd["mask_unit"]).cpu().numpy()
    ref = cpu.unmask_planes(eng.acc.cpu(), mask.cpu(), rnd["mask_unit"], K).numpy()
    assert (out == ref).all()
    # doubles decide a truncation only to ~2^-3 at 2^50: off by one at most
    assert np.abs(out - rnd["oracle"]).max() <= 1


# -------------------------------------------------------------------- shards


def test_shard_unmask_equals_full():
    """Two emulated ranks: each recodes its accumulator into the compact digit
    planes, the planes are summed (the reduce-scatter), and each rank unmasks
    its shard against a column slice of the mask rows."""
    from xaynet_amd.parallel import compact_digits

    length = 1500
    rnd = forge_round(PRIME_F32_M3, length)
    full = load_engine(rnd)
    mask = unpack(full, rnd["mask_vect"])
    ref = full.unmask(mask, rnd["mask_unit"])

    k, w = compact_digits(full.order_int, 2)
    assert 2 * (2**w - 1) < 2**63 and k * w >= 289
    ranks = [load_engine(rnd, which) for which in ((0, 2), (1,))]
    compact = [e.recode_planes(torch.full((k, length), -1, dtype=torch.int64, device="cuda"), w)
               for e in ranks]
    for planes in compact:
        assert int(planes.min()) >= 0 and int(planes.max()) < 2**w
    summed = compact[0] + compact[1]
    shard = length // 2
    parts = []
    for r, e in enumerate(ranks):
        lo = r * shard
        parts.append(e.unmask_planes(summed[:, lo : lo + shard].contiguous(),
                                     mask[:, lo : lo + shard], rnd["mask_unit"], K,
                                     digit_bits=w))
    assert torch.equal(torch.cat(parts), ref)
    assert_matches_oracle(rnd["cfg"], ref.cpu().numpy(), rnd["oracle"])

    # the compact planes are the digits of the canonical value
    back = ranks[0].new_values()
    ranks[0].planes_to_values(compact[0], back, digit_bits=w)
    assert torch.equal(back, ranks[0].canonical())
    lifted = torch.zeros(k, length, dtype=torch.int64, device="cuda")
    ranks[0].values_to_planes(back, lifted, digit_bits=w)
    assert torch.equal(lifted, compact[0])


# ----------------------------------------------------------------------- K5w


@pytest.mark.parametrize("cfg_args", [PRIME_F32_M3, (1, 3, 255, 3)])
def test_mask_weights_round(cfg_args):
    """mask_weights on the GPU -> aggregate -> unmask. f32: within 2^-22 *
    max_j |w_j[i]| of the float64 mean (the f32 output rounding plus the one
    double rounding of scalar * w). i64 (|w| < 2^50): scalar * w is off by
    less than 2^-4 per update before the exact floor, so the truncated result
    is within 1 of the oracle's, which masked the exact scalar * w."""
    rnd = forge_round(cfg_args)
    cfg, pair = rnd["cfg"], mk.MaskConfigPair(rnd["cfg"], rnd["cfg"])
    order, bpn = int(cfg.order), cfg.bytes_per_number
    eng = make_engine(cfg_args, LENGTH)
    pool = eng.alloc_update_pool(K)
    mask_agg = mk.Aggregation(pair, LENGTH)
    for row, (seed, w) in enumerate(zip(rnd["seeds"], rnd["weights"])):
        wire = eng.mask_weights(seed, torch.from_numpy(w), 1, K)
        assert len(wire) == 8 + LENGTH * bpn + 4 + bpn
        eng.upload_update(pool, row, wire[8 : 8 + LENGTH * bpn])
        eng.unit_acc = (eng.unit_acc + int.from_bytes(wire[-bpn:], "little")) % order
        mask_agg.aggregate(mk.derive_mask(seed, LENGTH, pair))
    eng.aggregate_pool(pool, K)
    mask_wire = bytes(mask_agg.object.serialize())[8 : 8 + LENGTH * bpn]
    out = eng.unmask(unpack(eng, mask_wire), int(mask_agg.object.unit_value)).cpu().numpy()

    stack = np.stack([w.astype(np.float64) for w in rnd["weights"]])
    mean = stack.sum(axis=0) / K
    if cfg.dtype == 0:
        assert out.dtype == np.float32
        assert (np.abs(out - mean) <= 2.0**-22 * np.abs(stack).max(axis=0)).all()
    else:
        assert out.dtype == np.int64
        assert np.abs(out - rnd["oracle"]).max() <= 1


# --------------------------------------------------------------- coordinator


def test_staged_coordinator_round_f32_bmax():
    """A coordinator configured with F32/Bmax stages its updates for the GPU
    driver and gets the round's model from it (K6 unpack + exact-offset K4):
    the mean of the accepted updaters' models. Every participant trains the
    same model, so the mean is that model whichever updates were accepted."""
    import time

    from xaynet_amd.ops import make_coordinator_driver

    co, sdk = _core.coordinator, _core.sdk
    n, length = 12, 515  # 12: fewer than 3 updaters (a restarted round) in 2% of the draws
    s = co.Settings()
    s.sum_prob = 0.5
    s.update_prob = 1.0
    s.model_length = length
    c = mk.MaskConfig(*PRIME_F32_M3)
    s.mask_cfg = mk.MaskConfigPair(c, c)
    s.set_sum(1, 100, 0.05, 3.0)
    s.set_update(3, 100, 0.05, 3.0)
    s.set_sum2(1, 100, 0.05, 3.0)
    coord = co.Coordinator(s, co.InMemoryStorage(), co.InMemoryModels(), True)  # staged
    driver = make_coordinator_driver(coord, c, c, length, pool_size=4)
    driver.start()
    client = sdk.InProcessClient(coord)
    rng = np.random.default_rng(29)
    participants = [
        sdk.Participant(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), 1, 1, client)
        for _ in range(n)
    ]
    weights = _weights(c, length, rng)
    coord.start()
    t0 = time.time()
    model, updaters = None, set()
    try:
        while time.time() - t0 < 60.0 and model is None:
            for i, p in enumerate(participants):
                p.tick()
                if p.should_set_model:
                    p.set_model(weights)
                    updaters.add(i)
            body = coord.fetch_model()
            if body and body[0] == 1:
                model = np.asarray(sdk.decode_model(body, 0))
            time.sleep(0.002)
    finally:
        coord.stop()
        driver.stop()
    assert model is not None, "no global model published"
    assert driver.rounds_unmasked >= 1, "model did not come from the GPU driver"
    assert model.dtype == np.float32 and len(updaters) >= 3
    expect = weights.astype(np.float64)
    bound = 2.0**-22 * np.abs(expect)  # as test_mask_weights_round
    assert (np.abs(model - expect) <= bound).all()


def test_server_starts_f32_bmax_on_the_gpu_plane(caplog):
    """`python -m xaynet_amd.server` with F32/Bmax and gpu = true: the GPU
    driver starts, without the CPU-fallback warning."""
    from test_bmax_cpu import _serve_briefly, bmax_daemon_settings

    settings = bmax_daemon_settings("F32")
    with caplog.at_level("WARNING", logger="xaynet.server"):
        _serve_briefly(settings)
    assert settings.gpu is True
    assert not [r for r in caplog.records if "CPU aggregation plane" in r.getMessage()]


# --------------------------------------------------------------- error paths


def test_error_paths():
    from xaynet_amd.ops import GpuMaskedAggregator

    f64_bmax = mk.MaskConfig(1, 1, 255, 3)
    with pytest.raises(ValueError, match="CPU oracle"):
        GpuMaskedAggregator(f64_bmax, f64_bmax, 16)
    eng = make_engine(PRIME_F32_M3, 16)
    pool = eng.alloc_update_pool(1)
    with pytest.raises(NotImplementedError, match="Bmax"):
        eng.synth_update(pool, 0, eng.new_values(zero=True), participant=0, scalar=1.0)
