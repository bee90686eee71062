#!/usr/bin/env python3
"""Time k3_aggregate variants on MI355X: the generic kernel's EPT values, the
LDS-staged kernels (201 / 202), the tile-streaming kernel (401 nontemporal,
402 default loads) and its loader-wave form (411 nontemporal, 412 default).

Usage: python scripts/k3_sweep.py [--length 25000000] [--pool 300] [--bpn 7]
           [--epts 0,4,401,402,411,412] [--ceiling] [--check]
Prints ms/dispatch and effective read TB/s per variant. --ceiling first times a
trivial coalesced 16-byte-per-lane read of the same pool, with default and
nontemporal loads: the rate K3 is held against. --check compares every
variant's digit planes with the first one's.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from xaynet_amd import _core, _hip
from xaynet_amd.ops import GpuMaskedAggregator

# bytes per number with an engine config: 7 = Prime/F32/B0/M6 (headline),
# 10 = Prime/F64/B0/M3 (wide u128 order); any other K3 bpn runs on raw bytes
ENGINE_CONFIGS = {7: (1, 0, 0, 6), 10: (1, 1, 0, 3)}
K3_BPNS = list(range(1, 17)) + [18, 37, 38, 39, 40]


def row_stride(length, bpn):
    return (length * bpn + 16 * bpn + 15) // 16 * 16


def make_pool(args):
    """(accumulator planes, pool [rows, stride], bytes per number)."""
    dev = "cuda:0"
    if args.bpn in ENGINE_CONFIGS:
        mk = _core.mask
        cfg = mk.MaskConfig(*ENGINE_CONFIGS[args.bpn])
        eng = GpuMaskedAggregator(cfg, cfg, args.length, device=dev)
        pool = eng.alloc_update_pool(args.pool)
        if eng.wide:
            # random bytes are fine for a bandwidth sweep (digit-plane adds are
            # value-independent)
            for p in range(args.pool):
                pool[p].copy_(torch.randint(0, 256, pool.shape[1:], dtype=torch.uint8, device=dev))
        else:
            scratch = torch.empty(args.length, dtype=torch.int64, device=dev)
            for p in range(args.pool):
                seed = (p + 1).to_bytes(32, "little")
                if p < 8:
                    eng.derive_mask_values(seed, out=scratch)
                eng.synth_update(pool, p, scratch, participant=p, scalar=1.0 / args.pool)
        eng.reset()
        return eng.acc, pool, eng.bpn
    pool = torch.empty(args.pool, row_stride(args.length, args.bpn), dtype=torch.uint8, device=dev)
    for p in range(args.pool):
        pool[p].copy_(torch.randint(0, 256, pool.shape[1:], dtype=torch.uint8, device=dev))
    acc = torch.zeros((args.bpn + 3) // 4, args.length, dtype=torch.int64, device=dev)
    return acc, pool, args.bpn


def timed(fn, reps):
    fn()  # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=25_000_000)
    ap.add_argument("--pool", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--epts", type=str, default="0,4,8,16,401,402,411,412")
    ap.add_argument("--bpn", type=int, default=7, choices=K3_BPNS)
    ap.add_argument("--ceiling", action="store_true",
                    help="time a plain coalesced read of the pool first")
    ap.add_argument("--check", action="store_true",
                    help="compare each variant's planes with the first variant's")
    args = ap.parse_args()

    acc, pool, bpn = make_pool(args)
    torch.cuda.synchronize()
    plan = _hip._k3_tile_plan(args.length, bpn, pool.stride(0))
    print(f"bpn={bpn} length={args.length} pool={args.pool} stride={pool.stride(0)} "
          f"tile plan: {plan}")

    if args.ceiling:
        sink = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        nbytes = pool.numel()
        for nt in (False, True):
            ms = timed(lambda: _hip._read_ceiling(pool.data_ptr(), nbytes, nt, sink.data_ptr()),
                       args.reps)
            print(f"ceiling {'nontemporal' if nt else 'default    '}: {ms:8.3f} ms  "
                  f"{nbytes / 1e9 / ms:6.2f} TB/s")

    gb = args.pool * args.length * bpn / 1e9
    first = None
    for ept in (int(x) for x in args.epts.split(",")):
        def run():
            _hip.aggregate_batch(acc.data_ptr(), pool.data_ptr(), pool.stride(0),
                                 args.pool, args.length, bpn, ept)
        ms = timed(run, args.reps)
        note = ""
        if args.check:
            acc.zero_()
            run()
            torch.cuda.synchronize()
            if first is None:
                first = acc.clone()
            else:
                note = "  planes equal" if torch.equal(acc, first) else "  PLANES DIFFER"
        print(f"ept={ept:3d}: {ms:8.3f} ms/dispatch  {gb / ms:6.2f} TB/s effective{note}")


if __name__ == "__main__":
    main()
