"""K12, masked vectors that lie in pieces gathered into the K3 pool, against
plain Python: the row is b"".join of the pieces, an element is valid iff
int.from_bytes(limb, "little") < order. Every assertion is equality."""
import numpy as np
import pytest
import torch

from test_gpu_update_stage import SENTINEL, below, engine_for, rule_t
from xaynet_amd import _core, _hip
from xaynet_amd.ops import GpuBox, gpu_available

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not gpu_available(), reason="needs an AMD GPU"),
]

crypto = _core.crypto


def engine_of(bpn, length):
    """engine_for; no catalogue config has 3 bytes a number, so there the
    6-byte engine with its vector narrowed to bpn bytes below 2^(8 bpn) - 3
    (the unit keeps its config)."""
    if bpn != 3:
        return engine_for(bpn, length)
    eng = engine_for(6, length)
    eng.bpn, eng.order_int, eng.order = bpn, 256**bpn - 3, str(256**bpn - 3)
    return eng


def wire(eng, values, unit):
    """MaskObject wire bytes: config | count | limbs | unit config | unit limb."""
    cfg = bytes(eng.vect_cfg.to_bytes())
    return cfg + len(values).to_bytes(4, "big") + \
        b"".join(v.to_bytes(eng.bpn, "little") for v in values) + \
        cfg + unit.to_bytes(eng.unit_cfg.bytes_per_number, "little")


def cut(rng, nbytes, layout):
    """Piece lengths of an object of nbytes."""
    if layout == "one":
        return [nbytes]
    sizes = []
    while sum(sizes) < nbytes:
        sizes.append(int(rng.integers(1, 301)) if layout == "ragged" else int(layout))
    sizes[-1] -= sum(sizes) - nbytes
    return sizes


def scatter(rng, wires, layout):
    """The wires cut into pieces that lie at random byte offsets, in shuffled
    order, in a buffer of random bytes: (device buffer, pieces an object)."""
    cuts, objects = [], [[] for _ in wires]
    for i, w in enumerate(wires):
        sizes = cut(rng, len(w), layout)
        cuts += [(i, j, int(at), n) for j, (at, n) in enumerate(zip(np.cumsum([0] + sizes), sizes))]
        objects[i] = [None] * len(sizes)
    place, at = [], 8  # "one": the limbs, 8 bytes in, start on a 16-byte boundary
    for c in rng.permutation(len(cuts)):
        i, j, src, n = cuts[c]
        at += 0 if layout == "one" else int(rng.integers(0, 8))
        place.append((at, wires[i][src:src + n]))
        objects[i][j] = (at, n)
        at += n if layout != "one" else (n + 15) // 16 * 16
    host = rng.integers(0, 256, (at + 67) // 4 * 4, dtype=np.uint8)
    for off, data in place:
        host[off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
    return torch.from_numpy(host).to("cuda:0"), objects


def five(eng, rng):
    """The five objects of a case: (values, units, expected statuses)."""
    order, n, tile = eng.order_int, eng.length, 64 * rule_t(eng.bpn)
    vals = [below(rng, order, n) for _ in range(5)]
    vals[1][0] = order
    vals[2][-1] = order
    if tile < n:
        vals[3][tile] = 256**eng.bpn - 1
    vals[4] = [order - 1] * n
    return vals, below(rng, order, 5), [0, 2, 2, 2 if tile < n else 0, 0]


@pytest.mark.parametrize("layout", ["one", "3904", "137", "13", "ragged"])
@pytest.mark.parametrize("length", ["17", "tile+1", "span"])
@pytest.mark.parametrize("bpn", [3, 7, 10, 16, 40])
def test_gather_and_verdict(bpn, length, layout):
    tile = 64 * rule_t(bpn)
    plan = _hip._gather_plan(1 << 20, bpn, 1, 1)
    assert plan["tile_elems"] == tile
    # "span": a block's whole span, then a block with one tile more than waves
    n = {"17": 17, "tile+1": tile + 1,
         "span": (plan["waves"] * plan["span"] + plan["waves"] + 1) * tile + 5}[length]
    eng = engine_of(bpn, n)
    rng = np.random.default_rng(1200 * bpn + n)
    vals, units, want = five(eng, rng)
    wires = [wire(eng, v, u) for v, u in zip(vals, units)]
    dev, objects = scatter(rng, wires, layout)
    host = dev.cpu().numpy()
    rows = [b"".join(host[o:o + m].tobytes() for o, m in obj)[8:8 + n * bpn] for obj in objects]
    assert rows == [w[8:8 + n * bpn] for w in wires]
    assert want == [2 if any(int.from_bytes(r[i * bpn:(i + 1) * bpn], "little") >= eng.order_int
                             for i in range(n)) else 0 for r in rows]
    pool = eng.alloc_update_pool(7).fill_(SENTINEL)
    staged = eng.stage_segments(dev, objects, pool, row=1)
    assert staged.status == want
    valid = [i for i, s in enumerate(want) if s == 0]
    assert (staged.row, staged.rows, staged.valid) == (1, 5, len(valid))
    assert staged.unit_sum == sum(units[i] for i in valid) % int(eng.unit_cfg.order)
    got = pool.cpu().numpy()
    copied = (n * bpn + 15) // 16 * 16
    for i in range(5):
        expect = rows[i] if want[i] == 0 else bytes(n * bpn)
        assert got[1 + i, :n * bpn].tobytes() == expect, f"object {i}"
        assert not got[1 + i, n * bpn:copied].any(), f"object {i}: zeros up to the boundary"
        assert (got[1 + i, copied:] == SENTINEL).all(), f"object {i}: bytes past the copy"
    assert (got[0] == SENTINEL).all() and (got[6:] == SENTINEL).all()


@pytest.mark.parametrize("bpn", [7, 10])
def test_gathered_rows_through_k3(bpn):
    n = 3 * 64 * rule_t(bpn) + 5
    eng = engine_for(bpn, n)
    rng = np.random.default_rng(bpn)
    vals, units, want = five(eng, rng)
    dev, objects = scatter(rng, [wire(eng, v, u) for v, u in zip(vals, units)], "ragged")
    pool = eng.alloc_update_pool(5).fill_(SENTINEL)
    staged = eng.stage_segments(dev, objects, pool)
    eng.aggregate_staged(pool, staged)
    limbs = eng.canonical().cpu().numpy().view(np.uint64).reshape(-1, n)  # u64 limb rows
    got = [sum(int(limbs[j, i]) << 64 * j for j in range(limbs.shape[0])) for i in range(n)]
    valid = [vals[i] for i, s in enumerate(want) if s == 0]
    assert got == [sum(v[i] for v in valid) % eng.order_int for i in range(n)]
    assert eng.nb_models == staged.valid == len(valid)
    assert eng.unit_acc == staged.unit_sum == sum(units[i] for i in (0, 4)) % eng.order_int


def test_open_update_sets_from_sealed_bytes():
    pk, sk = crypto.box_seed_keypair(b"\x21" * 32)
    seed = b"\x5e" * 32  # the round seed
    spk, ssk = crypto.sign_keypair_from_seed(b"\x11" * 32)
    rng = np.random.default_rng(12)
    eng = engine_for(7, 17)
    good, over = below(rng, eng.order_int, 17), below(rng, eng.order_int, 17)
    over[9] = eng.order_int + 1
    sum_sig = crypto.sign_detached(seed + b"sum", ssk)
    upd_sig = crypto.sign_detached(seed + b"update", ssk)
    flipped = bytes([upd_sig[0] ^ 1]) + upd_sig[1:]
    seed_dict = (4 + 112).to_bytes(4, "big") + rng.bytes(112)

    def message(flags, payload):
        body = spk + pk + (136 + len(payload)).to_bytes(4, "big") + bytes([2, flags, 0, 0]) + payload
        return crypto.sealbox_seal(crypto.sign_detached(body, ssk) + body, pk)

    def chunks(mid, payload):  # 150 data bytes a chunk: 382 bytes are three chunks
        data = [payload[at:at + 150] for at in range(0, len(payload), 150)]
        return [message(1, c.to_bytes(2, "big") + mid.to_bytes(2, "big") +
                        bytes([c == len(data) - 1, 0, 0, 0]) + d) for c, d in enumerate(data)]

    a = chunks(1, sum_sig + upd_sig + wire(eng, good, 5) + seed_dict)
    b = chunks(2, sum_sig + upd_sig + wire(eng, good, 6) + seed_dict)
    c = chunks(3, sum_sig + flipped + wire(eng, good, 7) + seed_dict)
    d = chunks(4, sum_sig + upd_sig + wire(eng, over, 8) + seed_dict)
    single = message(0, sum_sig + upd_sig + wire(eng, good, 9) + seed_dict)
    assert len(a) == 3
    #          0     1     2     3     4     5     6     7     8     9    10    11    12
    sealed = [a[2], a[0], b[0], a[0], c[0], c[1], c[2], a[1], b[2], d[1], d[0], d[2], single]
    pool = eng.alloc_update_pool(5).fill_(SENTINEL)
    flags, staged, index, pending, host_sets = GpuBox("cuda:0").open_update_sets(
        sealed, pk, sk, seed, eng, pool, row=1)
    assert flags == [1] * 12 + [7]
    assert (index, pending, host_sets) == ([[3, 7, 0], [10, 9, 11], [12]], [2, 8], [])
    assert staged.status == [0, 2, 0]
    assert (staged.row, staged.rows, staged.valid, staged.unit_sum) == (1, 3, 2, 14)
    got = pool.cpu().numpy()
    want = wire(eng, good, 5)[8:8 + 17 * 7]
    assert got[1, :17 * 7].tobytes() == want and got[3, :17 * 7].tobytes() == want
    assert not got[2, :17 * 7].any()
    assert (got[0] == SENTINEL).all() and (got[4:] == SENTINEL).all()


def test_refusals():
    eng = engine_for(7, 17)
    rng = np.random.default_rng(4)
    vals, units, _ = five(eng, rng)
    dev, objects = scatter(rng, [wire(eng, v, u) for v, u in zip(vals, units)], "13")
    pool = eng.alloc_update_pool(6).fill_(SENTINEL)
    past = [objects[0][:-1] + [(dev.numel() - 5, 13)]] + objects[1:]
    for args in [(dev, past, pool, 0),           # a piece past the buffer
                 (dev, objects, pool, 2),        # five objects, four rows left
                 (dev.view(torch.int8), objects, pool, 0)]:
        with pytest.raises(ValueError):
            eng.stage_segments(*args)
    assert (pool == SENTINEL).all()
    staged = eng.stage_segments(dev, [objects[0][:-1], [(0, 0)]], pool)
    assert (staged.status, staged.rows, staged.valid) == ([1, 1], 0, 0)
    assert (pool == SENTINEL).all()
