"""Tile-streaming K3 kernel (ept 401 / 402): the host plan, and bit-exact
digit planes against numpy on the GPU.

The plan tests need no GPU: _hip._k3_tile_plan is the function the launcher
itself uses to split a row into full tiles and a remainder.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from xaynet_amd import _hip  # noqa: E402
from xaynet_amd.ops.base import MaskedAggregatorBase  # noqa: E402

# every bytes-per-number value K3 is instantiated for
K3_BPNS = tuple(range(1, 17)) + (18, 37, 38, 39, 40)
# the ones with a tile kernel: the headline (7), the wide u128 order (10), a
# narrow one, and 5 and 10 digit planes
TILE_BPNS = (3, 7, 10, 18, 40)
CODES = (401, 402, 0)


def row_stride(length, bpn):
    return MaskedAggregatorBase.row_stride(SimpleNamespace(length=length, bpn=bpn))


def plan_of(length, bpn):
    return _hip._k3_tile_plan(length, bpn, row_stride(length, bpn))


def rule_t(bpn):
    """Smallest T >= 4 whose 64*T elements are whole 1-KiB pieces."""
    return next(t for t in range(4, 21) if t * bpn % 16 == 0)


# ------------------------------------------------------------- plan (CPU)


@pytest.mark.parametrize("bpn", K3_BPNS)
def test_tile_plan_partitions_the_row(bpn):
    tile = plan_of(25_000_000, bpn)["tile_elems"]
    assert (tile > 0) == (bpn in TILE_BPNS)
    lengths = {1, 3, 4099, 25_000_000}
    if tile:
        assert tile == 64 * rule_t(bpn)
        assert tile * bpn % 1024 == 0
        lengths |= {tile - 1, tile, tile + 1}
    for length in sorted(lengths):
        stride = row_stride(length, bpn)
        p = _hip._k3_tile_plan(length, bpn, stride)
        if not tile:
            assert (p["n_tiles"], p["rem_start"], p["max_byte"]) == (0, 0, -1)
            continue
        assert p["tile_elems"] == tile and p["depth"] >= 2 and p["waves"] >= 1
        # full tiles [0, rem_start) and the remainder [rem_start, len)
        assert p["n_tiles"] == length // tile
        assert p["rem_start"] == p["n_tiles"] * tile <= length
        assert length - p["rem_start"] < tile
        # the last byte the tile kernel reads is the last byte of the last tile
        assert p["max_byte"] == p["rem_start"] * bpn - 1 < stride
        assert p["max_byte"] < length * bpn
        # a stride that breaks 16-byte alignment of the rows: no tiles
        q = _hip._k3_tile_plan(length, bpn, stride + 4)
        assert (q["n_tiles"], q["rem_start"], q["max_byte"]) == (0, 0, -1)


def test_tile_plan_rejects_short_rows():
    """A row that cannot hold len elements and 16 bytes of padding gets no
    tiles; one that just can, does."""
    for stride in (4096 * 7 - 16, 4096 * 7):
        p = _hip._k3_tile_plan(4096, 7, stride)
        assert (p["n_tiles"], p["rem_start"], p["max_byte"]) == (0, 0, -1)
    assert _hip._k3_tile_plan(4096, 7, 4096 * 7 + 16)["n_tiles"] == 4


# -------------------------------------------------------------- GPU, exact


def case_lengths(bpn):
    p = plan_of(1 << 20, bpn)
    tile, waves = p["tile_elems"], p["waves"]
    # one tile; one tile + 1; a full block, a partial block and a tail;
    # remainder only
    return (tile, tile + 1, (waves + 1) * tile + 3, 3)


def case_rows(bpn):
    d = plan_of(1 << 20, bpn)["depth"]
    # prologue shorter than the ring, exactly the ring, the wrap, the drain
    return sorted({1, d - 1, d, d + 1, 2 * d + 1})


@lru_cache(maxsize=None)
def tile_inputs(bpn, length, lead=0):
    """(flat bytes, stride, prior planes, expected planes after r rows for
    every r): row 0 all 0xFF, row 1 zero, row 2 (offset mod 251), the rest
    random, padding included; digit d of element i is the little-endian
    integer of bytes [i*bpn + 4d, i*bpn + min(4d + 4, bpn))."""
    rows = max(case_rows(bpn))
    rng = np.random.default_rng(7000 * bpn + length + lead)
    stride = row_stride(length, bpn)
    flat = rng.integers(0, 256, lead + rows * stride, dtype=np.uint8)
    pool = flat[lead:].reshape(rows, stride)
    pool[0], pool[1] = 0xFF, 0
    pool[2] = np.arange(stride) % 251
    n_digits = (bpn + 3) // 4
    prior = rng.integers(0, 2**40, (n_digits, length), dtype=np.uint64)
    limbs = pool[:, : length * bpn].reshape(rows, length, bpn).astype(np.uint64)
    digits = np.zeros((rows, n_digits, length), dtype=np.uint64)
    for d in range(n_digits):
        for b in range(4 * d, min(4 * d + 4, bpn)):
            digits[:, d] += limbs[:, :, b] << np.uint64(8 * (b - 4 * d))
    expect = prior[None] + np.cumsum(digits, axis=0)  # expect[r - 1]: r rows
    for a in (flat, prior, expect):
        a.setflags(write=False)
    return flat, stride, prior, expect


def run_k3(dev, lead, stride, prior_dev, rows, length, bpn, code):
    acc = prior_dev.clone()
    _hip.aggregate_batch(acc.data_ptr(), dev.data_ptr() + lead, stride, rows, length, bpn, code)
    torch.cuda.synchronize()
    return acc.cpu().numpy().view(np.uint64)


def require_gpu():
    from xaynet_amd.ops import gpu_available

    if not gpu_available():
        pytest.fail("GPU expected for -m gpu tests but not available")


@pytest.mark.gpu
@pytest.mark.parametrize("bpn", TILE_BPNS)
def test_tile_kernel_vs_numpy(bpn):
    """Codes 401, 402 and 0 add exactly the byte-gathered digits into a
    pre-filled accumulator, at every length class and ring phase."""
    require_gpu()
    for length in case_lengths(bpn):
        flat, stride, prior, expect = tile_inputs(bpn, length)
        dev = torch.tensor(flat).cuda()
        prior_dev = torch.tensor(prior.view(np.int64)).cuda()
        assert dev.data_ptr() % 16 == 0
        for rows in case_rows(bpn):
            for code in CODES:
                got = run_k3(dev, 0, stride, prior_dev, rows, length, bpn, code)
                bad = np.argwhere(got != expect[rows - 1])
                assert bad.size == 0, (f"bpn {bpn} code {code} n {length} rows {rows}: "
                                       f"{len(bad)} wrong, first (digit, element) "
                                       f"{bad[:4].tolist()}")


@pytest.mark.gpu
def test_tile_request_on_misaligned_pool():
    """Code 401 on a pool whose base is 4 bytes past a 16-byte boundary: the
    launcher falls back to the generic kernel, with the same result."""
    require_gpu()
    bpn, lead = 7, 4
    length = case_lengths(bpn)[2]
    rows = max(case_rows(bpn))
    flat, stride, prior, expect = tile_inputs(bpn, length, lead)
    dev = torch.tensor(flat).cuda()
    assert (dev.data_ptr() + lead) % 16 == 4
    prior_dev = torch.tensor(prior.view(np.int64)).cuda()
    got = run_k3(dev, lead, stride, prior_dev, rows, length, bpn, 401)
    assert (got == expect[rows - 1]).all()
