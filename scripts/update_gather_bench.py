"""K12 against its baselines (profiles/r22_update_gather.md): gathering the
masked vectors of multipart updates from their chunks into the K3 pool.

An object is `--elements` elements of random limbs whose top byte is zero (all
below the order). Its wire form lies in one device buffer twice: contiguous,
for K11 and the copy, and cut into chunk data of `--piece` bytes, each behind
the 144 bytes a chunk message has in front of its data, for K12. Per (bytes a
number, objects):

  k12     device events around _hip._gather_run: the upload of the piece
          tables, bases and cleared `bad` words, k12_gather, k11_wipe
  k11     device events around _hip._stage_run on the contiguous bytes
  copy    device events around dst.copy_(src) of the bytes K11 moves
  call    host clock around stage_segments, device synchronised
  host    host clock around the path without K12: the chunks device-to-host,
          b"".join, MaskObject.deserialize and is_valid, upload_update

k12, k11 and copy are taken alternately, `--rounds` times; the median and the
range are printed, milliseconds. A warm-up call checks statuses and rows.
"""
import argparse
import json
import statistics
import time

import numpy as np
import torch

from xaynet_amd import _core, _hip
from xaynet_amd.ops import GpuMaskedAggregator

CONFIGS = {7: (1, 0, 0, 6), 10: (1, 0, 0, 12)}


def events(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def stat(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f}..{max(xs):.3f})"


def measure(bpn, n, objects, piece, rounds, host_rounds):
    cfg = _core.mask.MaskConfig(*CONFIGS[bpn])
    eng = GpuMaskedAggregator(cfg, cfg, n, device="cuda:0")
    rng = np.random.default_rng(bpn)
    limbs = rng.integers(0, 256, (n, bpn), dtype=np.uint8)
    limbs[:, -1] = 0
    head = np.frombuffer(bytes(cfg.to_bytes()) + n.to_bytes(4, "big"), dtype=np.uint8)
    tail = np.frombuffer(bytes(cfg.to_bytes()) + (5).to_bytes(bpn, "little"), dtype=np.uint8)
    wire = np.concatenate([head, limbs.reshape(-1), tail])
    # contiguous: the limbs on a 16-byte boundary
    flat = (len(wire) + 8 + 15) // 16 * 16
    whole = np.zeros(flat * objects + 16, dtype=np.uint8)
    offsets = [flat * i + 8 for i in range(objects)]
    # chunked: 144 bytes of message in front of every `piece` bytes of data
    cuts = list(range(0, len(wire), piece))
    step = (144 + piece + 15) // 16 * 16
    chunked = np.zeros(step * len(cuts) * objects + 16, dtype=np.uint8)
    pieces = []
    for i in range(objects):
        whole[offsets[i]:offsets[i] + len(wire)] = wire
        base = step * len(cuts) * i
        pieces.append([(base + step * j + 144, min(piece, len(wire) - at))
                       for j, at in enumerate(cuts)])
        for (off, m), at in zip(pieces[i], cuts):
            chunked[off:off + m] = wire[at:at + m]
    whole_d, chunked_d = torch.from_numpy(whole).cuda(), torch.from_numpy(chunked).cuda()
    pool = eng.alloc_update_pool(objects)
    limb_bytes = n * bpn

    staged = eng.stage_segments(chunked_d, pieces, pool)  # warm-up, checked
    assert staged.status == [0] * objects and staged.unit_sum == 5 * objects % int(cfg.order)
    want = torch.from_numpy(limbs.reshape(-1)).cuda()
    assert all(torch.equal(pool[i, :limb_bytes], want) for i in range(objects))
    pool.zero_()
    assert eng.stage_updates(whole_d, offsets, [len(wire)] * objects, pool).status == [0] * objects
    assert all(torch.equal(pool[i, :limb_bytes], want) for i in range(objects))

    # the tables stage_segments hands to _gather_run, built once
    src, end = [], []
    for obj in pieces:
        at = 0
        for off, m in obj:
            a, b = max(at, 8), min(at + m, 8 + limb_bytes)
            if b > a:
                src.append(off + a - at)
                end.append(b - 8)
            at += m
    counts = [len(src) // objects] * objects
    src, end = np.array(src, dtype=np.uint64), np.array(end, dtype=np.uint64)
    plan12 = _hip._gather_plan(n, bpn, objects, len(src))
    plan11 = _hip._stage_plan(n, bpn, objects)
    work = torch.empty(max(plan12["work_bytes"], plan11["work_bytes"]), dtype=torch.uint8,
                       device="cuda:0")
    tail_args = (n, bpn, eng.order, pool.data_ptr(), pool.numel(), pool.stride(0), 0,
                 work.data_ptr(), work.numel())
    a, b = torch.empty(objects * plan11["copy_bytes"], dtype=torch.uint8, device="cuda:0"), \
        torch.empty(objects * plan11["copy_bytes"], dtype=torch.uint8, device="cuda:0")
    runs = {
        "k12": lambda: _hip._gather_run(chunked_d.data_ptr(), chunked_d.numel(), src, end, counts,
                                        *tail_args),
        "k11": lambda: _hip._stage_run(whole_d.data_ptr(), whole_d.numel(),
                                       [o + 8 for o in offsets], *tail_args),
        "copy": lambda: a.copy_(b),
    }
    times = {k: [] for k in runs}
    for r in range(rounds + 1):  # round 0 warms up
        for k, fn in runs.items():
            t = events(fn)
            if r:
                times[k].append(t)
    times["call"] = [clock(lambda: eng.stage_segments(chunked_d, pieces, pool))
                     for _ in range(rounds)]

    def host_path():
        host = chunked_d.cpu().numpy()
        for i, obj in enumerate(pieces):
            body = b"".join(host[off:off + m].tobytes() for off, m in obj)
            mo = _core.mask.MaskObject.deserialize(body)
            assert mo.is_valid()
            eng.upload_update(pool, i, mo.vect_bytes)

    times["host"] = [clock(host_path) for _ in range(host_rounds)]
    row = {"bpn": bpn, "elements": n, "objects": objects, "piece": piece, "pieces": len(src)}
    row.update({k: stat(v) for k, v in times.items() if v})
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--elements", type=int, default=25_000_000)
    ap.add_argument("--bpn", type=int, nargs="+", default=[7, 10], choices=sorted(CONFIGS))
    ap.add_argument("--objects", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--piece", type=int, default=3904)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=1)
    args = ap.parse_args()
    for bpn in args.bpn:
        for objects in args.objects:
            measure(bpn, args.elements, objects, args.piece, args.rounds, args.host_rounds)


if __name__ == "__main__":
    main()
