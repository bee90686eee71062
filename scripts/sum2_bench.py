#!/usr/bin/env python3
"""Time the sum2 task (ops/sum2.aggregate_masks_on) end to end on one GPU.

Shapes: S = 1024 seeds at n = 10k, 100k and 1M, and S = 64 seeds at n = 25M,
for Prime/F32/B0/M6 (u64 order) and Prime/F64/B0/M3 (u128 order). The engine
and its value tensors are kept across calls, as ParticipantAccel keeps them;
a call ends with the wire bytes on the host, so the clock stops after the
device has finished. Every shape is warmed up once, then timed `--reps`
times; the table gives the median and the min..max spread.

  --budgets 64,1024   sweep the workspace budget (MiB) of the batched path
  --single            also time derive_mask_values for one seed per shape
  --json PATH         append one JSON line per measurement

The script runs unchanged on a tree without the batched path (no budget
argument, no batch size): that is the per-seed baseline.
"""
import argparse
import hashlib
import inspect
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from xaynet_amd import _core  # noqa: E402
from xaynet_amd.ops import GpuMaskedAggregator  # noqa: E402
from xaynet_amd.ops.sum2 import aggregate_masks_on  # noqa: E402

CONFIGS = {"f32_m6": (1, 0, 0, 6), "f64_m3": (1, 1, 0, 3)}
SHAPES = [(10_000, 1024), (100_000, 1024), (1_000_000, 1024), (25_000_000, 64)]


def seeds_for(n):
    return [hashlib.sha256(b"sum2-bench-%d" % i).digest() for i in range(n)]


def timed(fn, reps):
    fn()  # warm-up: code objects, workspace growth
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budgets", default="", help="comma-separated MiB; default: the engine's")
    ap.add_argument("--max-n", type=int, default=25_000_000)
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    has_budget = "sum2_budget_bytes" in inspect.signature(GpuMaskedAggregator.__init__).parameters
    budgets = [int(b) << 20 for b in args.budgets.split(",") if b] if has_budget else []
    mk = _core.mask
    records = []
    print(f"{'config':8} {'n':>9} {'seeds':>5} {'budget':>7} {'batch':>5} {'group':>5} "
          f"{'median ms':>10} {'min':>9} {'max':>9} {'us/seed':>8}")
    for name, cfg_args in CONFIGS.items():
        cfg = mk.MaskConfig(*cfg_args)
        for n, s in SHAPES:
            if n > args.max_n:
                continue
            seeds = seeds_for(s)
            for budget in budgets or [None]:
                kw = {} if budget is None else {"sum2_budget_bytes": budget}
                eng = GpuMaskedAggregator(cfg, cfg, n, device="cuda:0", **kw)
                total, scratch = eng.new_values(), eng.new_values()
                ms = timed(lambda: aggregate_masks_on(eng, total, scratch, seeds), args.reps)
                rec = {
                    "what": "aggregate_masks", "config": name, "n": n, "seeds": s,
                    "budget_mib": getattr(eng, "sum2_budget_bytes", 0) >> 20,
                    "batch": getattr(eng, "batch_size", 1), "group": getattr(eng, "sum2_group", 1),
                    "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
                }
                records.append(rec)
                print(f"{name:8} {n:9d} {s:5d} {rec['budget_mib']:7d} {rec['batch']:5d} "
                      f"{rec['group']:5d} {rec['median_ms']:10.3f} {rec['min_ms']:9.3f} "
                      f"{rec['max_ms']:9.3f} {1e3 * rec['median_ms'] / s:8.1f}", flush=True)
                del eng, total, scratch
                torch.cuda.empty_cache()
            if args.single:
                eng = GpuMaskedAggregator(cfg, cfg, n, device="cuda:0")
                out = eng.new_values()
                k = 64 if n < 25_000_000 else 8

                def loop():
                    for seed in seeds[:k]:
                        eng.derive_mask_values(seed, out=out)

                ms = [t / k for t in timed(loop, args.reps)]
                rec = {"what": "derive_mask_values", "config": name, "n": n, "seeds": 1,
                       "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}
                records.append(rec)
                print(f"{name:8} {n:9d} {'one':>5} {'':7} {'':5} {'':5} {rec['median_ms']:10.4f} "
                      f"{rec['min_ms']:9.4f} {rec['max_ms']:9.4f}", flush=True)
                del eng, out
                torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "a") as fh:
            for rec in records:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
