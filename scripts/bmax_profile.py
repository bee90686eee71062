#!/usr/bin/env python3
"""Time the multi-limb (Bmax) kernel family at benchmark size, next to the
widest u128 config: K1 ms/mask, K3 effective read bandwidth, K4 ms.

  python scripts/bmax_profile.py [--length 25000000] [--pool 8] [--out FILE]

Correctness of these kernels is pinned by tests/test_gpu_bmax.py at small
size; this script only generates load. Update rows are random bytes with the
top byte of every element cleared, so each is a canonical value (< order) as a
real update is and the finalize kernels reduce sums of `pool` of them.

K1 is timed with a host clock (expand ends in a device-to-host read of the
accepted count), K3 and K4 with device events.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from xaynet_amd import _core  # noqa: E402
from xaynet_amd.ops import GpuMaskedAggregator  # noqa: E402

CONFIGS = {
    "Prime/F32/Bmax/M3": (1, 0, 255, 3),    # bpn 37, 5 limbs, acceptance 0.5%
    "Prime/I64/Bmax/M12": (1, 3, 255, 12),  # bpn 18, 3 limbs, acceptance 0.8%
    "Prime/F64/B6/M12": (1, 1, 6, 12),      # bpn 16, u128: the comparison
}


def timed_ms(fn, reps):
    """Median, min and max of `reps` device-event timings of fn()."""
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def profile(name, cfg_args, length, pool_rows, k1_reps, reps, log):
    cfg = _core.mask.MaskConfig(*cfg_args)
    eng = GpuMaskedAggregator(cfg, cfg, length)
    bpn = eng.bpn
    res = {"config": name, "bpn": bpn, "n_limbs": eng.n_limbs, "length": length,
           "pool": pool_rows}

    # K1
    mask = eng.new_values()
    eng.derive_mask_values(b"\x01" * 32, out=mask)  # warm-up: code objects, workspace
    torch.cuda.synchronize()
    k1 = []
    for i in range(k1_reps):
        t0 = time.perf_counter()
        eng.derive_mask_values(bytes([i + 2]) * 32, out=mask)
        torch.cuda.synchronize()
        k1.append((time.perf_counter() - t0) * 1e3)
    k1.sort()
    res["k1_ms_per_mask"] = [k1[len(k1) // 2], k1[0], k1[-1]]
    log(res)

    # K3
    pool = eng.alloc_update_pool(pool_rows)
    pool.random_(0, 256)
    pool[:, : length * bpn].view(pool_rows, length, bpn)[:, :, bpn - 1] = 0
    torch.cuda.synchronize()
    eng.aggregate_pool(pool, pool_rows)  # warm-up
    med, lo, hi = timed_ms(lambda: eng.aggregate_pool(pool, pool_rows), reps)
    res["k3_ms"] = [med, lo, hi]
    res["k3_read_GBps"] = pool_rows * length * bpn / (med * 1e-3) / 1e9
    log(res)

    # K4 on the sum of one pool
    eng.reset()
    eng.aggregate_pool(pool, pool_rows)
    order = int(cfg.order)
    mask_unit = 0
    for p in range(pool_rows):
        seed = bytes([p + 1]) * 32
        eng.unit_acc = (eng.unit_acc + eng.masked_unit_for(seed, 1, pool_rows)) % order
        mask_unit = (mask_unit + eng.unit_draw(seed)) % order
    out = eng.unmask(mask, mask_unit)  # warm-up
    med, lo, hi = timed_ms(lambda: eng.unmask(mask, mask_unit), reps)
    res["k4_ms"] = [med, lo, hi]
    res["k4_out"] = [str(out.dtype), bool(torch.isfinite(out.double()).all())]
    log(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=25_000_000)
    ap.add_argument("--pool", type=int, default=8)
    ap.add_argument("--k1-reps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    def log(res):
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for name, cfg_args in CONFIGS.items():
        profile(name, cfg_args, args.length, args.pool, args.k1_reps, args.reps, log)


if __name__ == "__main__":
    main()
