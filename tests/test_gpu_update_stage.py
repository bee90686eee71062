"""K11, masked vectors from device memory into the K3 pool, against plain
Python integers: an element is valid iff int.from_bytes(limb, "little") <
order. Bytes and integers: every assertion is equality."""
import numpy as np
import pytest
import torch

from xaynet_amd import _core, _hip
from xaynet_amd.ops import GpuBox, GpuMaskedAggregator, gpu_available

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not gpu_available(), reason="needs an AMD GPU"),
]

mk, crypto = _core.mask, _core.crypto
SENTINEL = 0xA5


def rule_t(bpn):
    """Smallest T >= 4 whose 64*T elements are whole 1-KiB pieces."""
    return next(t for t in range(4, 21) if t * bpn % 16 == 0)


def engine_for(bpn, length):
    """An engine over the first catalogue config with that many bytes a number."""
    for dtype in (0, 2, 3, 1):
        for bound in (0, 2, 4, 6, 255):
            for model in (3, 6, 9, 12):
                if (dtype, bound) != (1, 255):  # F64 Bmax: beyond the planes
                    cfg = mk.MaskConfig(1, dtype, bound, model)
                    if cfg.bytes_per_number == bpn:
                        return GpuMaskedAggregator(cfg, cfg, length, device="cuda:0")
    pytest.skip(f"no catalogue config has {bpn} bytes a number")


def wire(eng, values, unit, count=None):
    """MaskObject wire bytes: config | count | limbs | unit config | unit limb."""
    cfg = bytes(eng.vect_cfg.to_bytes())
    limbs = b"".join(v.to_bytes(eng.bpn, "little") for v in values)
    return cfg + (len(values) if count is None else count).to_bytes(4, "big") + limbs + \
        cfg + unit.to_bytes(eng.bpn, "little")


def below(rng, order, n):
    return [int.from_bytes(rng.bytes(48), "little") % order for _ in range(n)]


def batch(eng, rng):
    """Eight objects in one buffer of random bytes: (device buffer, offsets,
    avail, limbs an object, units, expected statuses by the integer rule)."""
    order, n, bpn, tile = eng.order_int, eng.length, eng.bpn, 64 * rule_t(eng.bpn)
    vals = [below(rng, order, n) for _ in range(8)]
    vals[1][0] = order
    vals[2][-1] = order
    if tile < n:
        vals[3][tile] = 256**bpn - 1
    vals[4] = [order - 1] * n
    units = below(rng, order, 8)
    wires = [wire(eng, v, u) for v, u in zip(vals, units)]
    wires[5] = wire(eng, vals[5], units[5], count=n + 1)
    wires[6] = bytes([wires[6][0] ^ 1]) + wires[6][1:]
    avail = [len(w) for w in wires]
    avail[7] -= 1
    offsets, at = [], 8
    for w in wires:
        offsets.append(at)
        at += (len(w) + 15) // 16 * 16
    host = rng.integers(0, 256, at + 64, dtype=np.uint8)
    for off, w in zip(offsets, wires):
        host[off:off + len(w)] = np.frombuffer(w, dtype=np.uint8)
    limbs = [w[8:8 + n * bpn] for w in wires]
    want = [2 if any(int.from_bytes(row[i * bpn:(i + 1) * bpn], "little") >= order
                     for i in range(n)) else 0 for row in limbs[:5]] + [1, 1, 1]
    return torch.from_numpy(host).to("cuda:0"), offsets, avail, limbs, units, want


# "span": a block whose waves stream their whole span through the ring (first
# waits, steady state, wrap, drain), then a block with one tile more than waves
@pytest.mark.parametrize("length", ["1", "17", "tile-1", "tile", "tile+1", "3*tile+5", "span"])
@pytest.mark.parametrize("bpn", [3, 7, 8, 10, 16, 18, 40])
def test_stage_and_verdict(bpn, length):
    tile = 64 * rule_t(bpn)
    plan = _hip._stage_plan(1 << 20, bpn, 1)
    n = {"1": 1, "17": 17, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1,
         "3*tile+5": 3 * tile + 5,
         "span": (plan["waves"] * plan["span"] + plan["waves"] + 1) * tile + 5}[length]
    eng = engine_for(bpn, n)
    dev, offsets, avail, limbs, units, want = batch(eng, np.random.default_rng(1100 * bpn + n))
    assert want == [0, 2, 2, 2 if 64 * rule_t(bpn) < n else 0, 0, 1, 1, 1]
    pool = eng.alloc_update_pool(10).fill_(SENTINEL)
    staged = eng.stage_updates(dev, offsets, avail, pool, row=1)
    assert staged.status == want
    valid = [i for i, s in enumerate(want) if s == 0]
    assert (staged.row, staged.rows, staged.valid) == (1, 5, len(valid))
    assert staged.unit_sum == sum(units[i] for i in valid) % eng.order_int
    got = pool.cpu().numpy()
    copied = (n * bpn + 15) // 16 * 16
    for i in range(5):
        expect = limbs[i] if want[i] == 0 else bytes(n * bpn)
        assert got[1 + i, :n * bpn].tobytes() == expect, f"object {i}"
        assert (got[1 + i, copied:] == SENTINEL).all(), f"object {i}: bytes past the copy"
    assert (got[0] == SENTINEL).all() and (got[6:] == SENTINEL).all()


@pytest.mark.parametrize("bpn", [7, 10])
def test_staged_rows_through_k3(bpn):
    n = 3 * 64 * rule_t(bpn) + 5
    eng = engine_for(bpn, n)
    dev, offsets, avail, limbs, units, want = batch(eng, np.random.default_rng(bpn))
    pool = eng.alloc_update_pool(9).fill_(SENTINEL)
    staged = eng.stage_updates(dev, offsets, avail, pool)
    eng.aggregate_staged(pool, staged)
    rows = eng.canonical().cpu().numpy().view(np.uint64).reshape(-1, n)  # u64 limb rows
    got = [sum(int(rows[j, i]) << 64 * j for j in range(rows.shape[0])) for i in range(n)]
    valid = [limbs[i] for i, s in enumerate(want) if s == 0]
    assert got == [sum(int.from_bytes(row[i * bpn:(i + 1) * bpn], "little") for row in valid)
                   % eng.order_int for i in range(n)]
    assert eng.nb_models == staged.valid == len(valid)
    assert eng.unit_acc == staged.unit_sum


def test_open_updates_from_sealed_bytes():
    pk, sk = crypto.box_seed_keypair(b"\x21" * 32)
    seed = b"\x5e" * 32  # the round seed
    spk, ssk = crypto.sign_keypair_from_seed(b"\x11" * 32)
    rng = np.random.default_rng(11)
    eng = engine_for(7, 17)
    good, over = below(rng, eng.order_int, 17), below(rng, eng.order_int, 17)
    over[9] = eng.order_int + 1
    sum_sig = crypto.sign_detached(seed + b"sum", ssk)
    upd_sig = crypto.sign_detached(seed + b"update", ssk)
    seed_dict = (4 + 2 * 112).to_bytes(4, "big") + rng.bytes(2 * 112)

    def message(tag, payload):
        body = spk + pk + (136 + len(payload)).to_bytes(4, "big") + bytes([tag, 0, 0, 0]) + payload
        return crypto.sealbox_seal(crypto.sign_detached(body, ssk) + body, pk)

    sealed = [
        message(2, sum_sig + upd_sig + wire(eng, good, 5) + seed_dict),
        message(2, sum_sig + bytes([upd_sig[0] ^ 1]) + upd_sig[1:] + wire(eng, good, 6) + seed_dict),
        message(2, sum_sig + upd_sig + wire(eng, over, 7) + seed_dict),
        message(1, sum_sig + b"\x44" * 32),
    ]
    pool = eng.alloc_update_pool(5).fill_(SENTINEL)
    flags, staged, index = GpuBox("cuda:0").open_updates(sealed, pk, sk, seed, eng, pool, row=1)
    assert (flags, index, staged.status) == ([7, 3, 7, 3], [0, 2], [0, 2])
    assert (staged.row, staged.rows, staged.valid, staged.unit_sum) == (1, 2, 1, 5)
    got = pool.cpu().numpy()
    assert got[1, :17 * 7].tobytes() == wire(eng, good, 5)[8:8 + 17 * 7]
    assert not got[2, :17 * 7].any()
    assert (got[0] == SENTINEL).all() and (got[3:] == SENTINEL).all()


def test_refusals():
    eng = engine_for(7, 17)
    dev, offsets, avail, *_ = batch(eng, np.random.default_rng(4))
    pool = eng.alloc_update_pool(9).fill_(SENTINEL)
    for args in [(dev, offsets, avail, pool, 2),           # eight objects, seven rows left
                 (dev.view(torch.int8), offsets, avail, pool, 0),
                 (dev, offsets, avail[:7], pool, 0)]:
        with pytest.raises(ValueError):
            eng.stage_updates(*args)
    assert (pool == SENTINEL).all()
    staged = eng.stage_updates(dev, [offsets[0] + 4], [avail[0]], pool)
    assert (staged.status, staged.rows, staged.valid) == ([1], 0, 0)
