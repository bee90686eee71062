"""Loader-wave K3 kernel (ept 411 / 412): the host plan, and bit-exact digit
planes against numpy on the GPU.

The plan tests need no GPU: _hip._k3_loader_plan is the function the launcher
itself uses, on top of the tile plan of the tile-streaming kernel.
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
# the ones with a loader kernel: CONS * pieces * (D - 2) loads fit one wave's
# counter of 64 (18 and 40 do not)
LOADER_BPNS = (3, 7, 10)
CODES = (411, 412)
# where ept 0 means 411
DEFAULT_BPNS = (7,)
NO_BLOCKS = {"consumers": 0, "depth": 0, "tile_blocks": 0, "has_remainder": False,
             "n_tiles": 0, "rem_start": 0, "max_byte": -1}


def row_stride(length, bpn):
    return MaskedAggregatorBase.row_stride(SimpleNamespace(length=length, bpn=bpn))


def loader_plan(length, bpn):
    return _hip._k3_loader_plan(length, bpn, row_stride(length, bpn))


# ------------------------------------------------------------- plan (CPU)


@pytest.mark.parametrize("bpn", K3_BPNS)
def test_loader_plan_follows_the_tile_plan(bpn):
    tile = _hip._k3_tile_plan(25_000_000, bpn, row_stride(25_000_000, bpn))["tile_elems"]
    lengths = {1, 3, 4099, 25_000_000}
    if tile:
        lengths |= {tile - 1, tile, tile + 1}
    for length in sorted(lengths):
        stride = row_stride(length, bpn)
        t = _hip._k3_tile_plan(length, bpn, stride)
        p = _hip._k3_loader_plan(length, bpn, stride)
        if bpn not in LOADER_BPNS or t["n_tiles"] == 0:
            assert p == NO_BLOCKS, (bpn, length)
            continue
        for key in ("n_tiles", "rem_start", "max_byte"):
            assert p[key] == t[key], (bpn, length, key)
        assert p["consumers"] >= 1 and p["depth"] >= 2
        # one wave tracks 64 loads: all but two ring slots in flight
        pieces = tile * bpn // 1024
        assert p["consumers"] * pieces * (p["depth"] - 2) <= 63
        assert p["tile_blocks"] == -(-t["n_tiles"] // p["consumers"])
        assert p["has_remainder"] == (t["rem_start"] < length)
        # a stride that breaks 16-byte alignment of the rows: no blocks
        assert _hip._k3_loader_plan(length, bpn, stride + 4) == NO_BLOCKS


# -------------------------------------------------------------- GPU, exact


def geometry(bpn):
    """(tile elements, consumers, ring depth) of the loader kernel."""
    length = 1 << 20
    p = loader_plan(length, bpn)
    tile = _hip._k3_tile_plan(length, bpn, row_stride(length, bpn))["tile_elems"]
    return tile, p["consumers"], p["depth"]


def case_lengths(bpn):
    tile, cons, _ = geometry(bpn)
    # one consumer working and the others at the barriers only; the same with
    # a remainder; one full group and no remainder block; a full group, a
    # group with one valid tile and the remainder; a group with CONS - 1 valid
    # tiles; remainder only (falls back)
    return (tile, tile + 1, cons * tile, (cons + 1) * tile + 3, (2 * cons - 1) * tile, 3)


def case_rows(bpn):
    d = geometry(bpn)[2]
    # prologue shorter than the ring, exactly the ring, the wrap, the drain
    return sorted({1, d - 1, d, d + 1, 2 * d + 1})


@lru_cache(maxsize=None)
def loader_inputs(bpn, length, lead=0):
    """(flat bytes, stride, prior planes, expected planes after r rows for
    every r): row 0 all 0xFF, row 1 zero, row 2 (offset mod 251), the rest
    random, padding included; digit d of element i is the little-endian
    integer of bytes [i*bpn + 4d, i*bpn + min(4d + 4, bpn))."""
    rows = max(case_rows(bpn))
    rng = np.random.default_rng(9000 * bpn + length + lead)
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
def test_loader_kernel_one_tile_one_row():
    """The narrowest launch: bpn 7, one tile, one row. One consumer works,
    the others only attend the barrier, the loader issues one row and drains."""
    require_gpu()
    bpn = 7
    length = geometry(bpn)[0]
    flat, stride, prior, expect = loader_inputs(bpn, length)
    dev = torch.tensor(flat).cuda()
    prior_dev = torch.tensor(prior.view(np.int64)).cuda()
    got = run_k3(dev, 0, stride, prior_dev, 1, length, bpn, 411)
    assert (got == expect[0]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("bpn", LOADER_BPNS)
def test_loader_kernel_vs_numpy(bpn):
    """Codes 411 and 412, and 0 where it means 411, add exactly the
    byte-gathered digits into a pre-filled accumulator, at every length class
    and ring phase."""
    require_gpu()
    codes = CODES + ((0,) if bpn in DEFAULT_BPNS else ())
    for length in case_lengths(bpn):
        flat, stride, prior, expect = loader_inputs(bpn, length)
        dev = torch.tensor(flat).cuda()
        prior_dev = torch.tensor(prior.view(np.int64)).cuda()
        assert dev.data_ptr() % 16 == 0
        for rows in case_rows(bpn):
            for code in codes:
                got = run_k3(dev, 0, stride, prior_dev, rows, length, bpn, code)
                bad = np.argwhere(got != expect[rows - 1])
                assert bad.size == 0, (f"bpn {bpn} code {code} n {length} rows {rows}: "
                                       f"{len(bad)} wrong, first (digit, element) "
                                       f"{bad[:4].tolist()}")


@pytest.mark.gpu
def test_loader_request_on_misaligned_pool():
    """Code 411 on a pool whose base is 4 bytes past a 16-byte boundary: the
    launcher falls back to the generic kernel, with the same result."""
    require_gpu()
    bpn, lead = 7, 4
    length = case_lengths(bpn)[3]
    rows = max(case_rows(bpn))
    flat, stride, prior, expect = loader_inputs(bpn, length, lead)
    dev = torch.tensor(flat).cuda()
    assert (dev.data_ptr() + lead) % 16 == 4
    prior_dev = torch.tensor(prior.view(np.int64)).cuda()
    got = run_k3(dev, lead, stride, prior_dev, rows, length, bpn, 411)
    assert (got == expect[rows - 1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("bpn", LOADER_BPNS)
def test_loader_kernel_writes_nothing_past_a_plane(bpn):
    """The planes sit in the middle of a larger pre-filled buffer whose every
    plane is followed by a guard of one tile: after a run with a partial group
    and a remainder, the guards and the rest of the buffer are as before."""
    require_gpu()
    tile = geometry(bpn)[0]
    length = case_lengths(bpn)[3]
    rows = max(case_rows(bpn))
    flat, stride, prior, expect = loader_inputs(bpn, length)
    n_digits = prior.shape[0]
    # the kernel addresses plane d at acc + d * length: give it a buffer of
    # n_digits * length words between two guards, pre-filled throughout
    rng = np.random.default_rng(bpn)
    whole = rng.integers(0, 2**40, tile + n_digits * length + tile, dtype=np.uint64)
    whole[tile: tile + n_digits * length] = prior.reshape(-1)
    want = whole.copy()
    want[tile: tile + n_digits * length] = expect[rows - 1].reshape(-1)
    dev = torch.tensor(flat).cuda()
    buf = torch.tensor(whole.view(np.int64)).cuda()
    clone = buf.clone()
    _hip.aggregate_batch(clone.data_ptr() + 8 * tile, dev.data_ptr(), stride, rows, length, bpn,
                         411)
    torch.cuda.synchronize()
    got = clone.cpu().numpy().view(np.uint64)
    assert (got == want).all()
