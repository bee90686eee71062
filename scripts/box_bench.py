#!/usr/bin/env python3
"""K8 benchmark: sealed boxes opened and sealed on the GPU (ops/box.py) next
to the CPU box of `_core.crypto` on the same machine.

Shapes: one 175 MB update, 64 multipart chunks of 8 MiB, 4096 chunks of 4 KiB.
Per shape and direction, after one warm-up call:
  kernel_ms  device events around the K8 launches of a call (descriptor upload
             included), median of --reps
  call_ms    host clock around the whole call, device synchronised: key
             agreement per box, packing through pinned memory, the copy in,
             the kernels (the copy back is not part of it: the payload stays
             on the device for K3)
  cpu_ms     sealbox_open / sealbox_seal of the same boxes, one thread
Opened and sealed bytes are compared with the CPU's before anything is timed.
One JSON line per shape and direction.

Usage (GPU box): python scripts/box_bench.py [--reps 5] [--shapes 1x175000000,64x8388608]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from xaynet_amd import _core  # noqa: E402
from xaynet_amd.ops import GpuBox  # noqa: E402

cr = _core.crypto


def timed(fn, reps):
    walls = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    return walls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="1x175000000,64x8388608,4096x4096")
    args = ap.parse_args()

    box = GpuBox("cuda:0", time_kernels=True)
    pk, sk = cr.box_seed_keypair(b"\x42" * 32)
    rng = np.random.default_rng(18)
    for shape in args.shapes.split(","):
        count, size = (int(x) for x in shape.split("x"))
        msgs = [rng.bytes(size) for _ in range(count)]
        sealed = [bytes(cr.sealbox_seal(m, pk)) for m in msgs]
        total_mb = count * size / 1e6

        # correctness first, which is also the warm-up
        opened, ok = box.sealbox_open_batch(sealed, pk, sk)
        assert bool(ok.all()) and all(bytes(t.cpu().numpy()) == m for t, m in zip(opened, msgs))
        resealed = box.sealbox_seal_batch(msgs, pk)
        assert all(cr.sealbox_open(bytes(t.cpu().numpy()), pk, sk) == m
                   for t, m in zip(resealed, msgs))
        del opened, resealed

        for name, gpu, cpu in (
            ("open", lambda: box.sealbox_open_batch(sealed, pk, sk),
             lambda: [cr.sealbox_open(s, pk, sk) for s in sealed]),
            ("seal", lambda: box.sealbox_seal_batch(msgs, pk),
             lambda: [cr.sealbox_seal(m, pk) for m in msgs]),
        ):
            kernel, calls = [], []
            for _ in range(args.reps):
                calls += timed(gpu, 1)
                kernel.append(box.kernel_ms)
            t0 = time.perf_counter()
            cpu()
            cpu_ms = (time.perf_counter() - t0) * 1e3
            k, c = statistics.median(kernel), statistics.median(calls)
            print(json.dumps({
                "op": name, "boxes": count, "bytes_per_box": size, "reps": args.reps,
                "kernel_ms": round(k, 3), "kernel_ms_min_max": [round(min(kernel), 3),
                                                                round(max(kernel), 3)],
                "kernel_GB_per_s": round(total_mb / k, 1),
                "call_ms": round(c, 2), "call_ms_min_max": [round(min(calls), 2),
                                                            round(max(calls), 2)],
                "call_MB_per_s": round(total_mb / c * 1e3, 1),
                "cpu_ms_one_thread": round(cpu_ms, 2),
                "cpu_MB_per_s": round(total_mb / cpu_ms * 1e3, 1),
            }), flush=True)


if __name__ == "__main__":
    main()
