#!/usr/bin/env python3
"""Update masking, exact mode against the double-precision mode, at 25M
elements: Prime/F32/B0/M6 (u64 order), Prime/F64/B0/M3 (u128) and
Prime/F32/Bmax/M3 (five limbs). Both modes alternate in one process, warmed.
Two figures per config and mode, median [min, max]:
  - the K5w kernel alone: one `_hip.mask_weights` launch on prepared mask
    values between two device events (3 warm-up launches, 15 timed), for the
    scalars 1/1 (the exact kernel then skips its division) and 1/3;
  - the whole `eng.mask_weights` call from a host tensor (H2D + K1 + K5w +
    D2H + wire assembly), host clock, scalar 1/3 (2 warm-up calls, 7 timed).
Run: python scripts/mask_exact_bench.py [n_elements]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from xaynet_amd import _core, _hip
from xaynet_amd.ops import GpuMaskedAggregator
from xaynet_amd.ops.base import _cfg_scalars

mk = _core.mask
N = int(sys.argv[1]) if len(sys.argv) > 1 else 25_000_000
SEED = b"\x07" * 32
MODES = ("double", "exact")


def spread(ts):
    ts = sorted(ts)
    return f"{ts[len(ts) // 2]:.1f} [{ts[0]:.1f}, {ts[-1]:.1f}]"


def kernel_us(eng, w_dev, dt, mask, out, p, q, mode):
    """One K5w launch between two device events, in microseconds."""
    lo, hi, n = eng._vals(mask)
    vinfo = _cfg_scalars(eng.vect_cfg)
    kw = {"scalar_num": p, "scalar_den": q} if mode == "exact" else \
        {"offset": str(vinfo["add_shift"] * vinfo["exp_shift_u64"]) if eng.bmax else ""}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    _hip.mask_weights(w_dev.data_ptr(), dt, lo, hi, out.data_ptr(), n, eng.bpn, eng.order, p / q,
                      float(vinfo["add_shift"]), str(vinfo["exp_shift_u64"]), **kw)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


print(f"| config | mode | K5w kernel, scalar 1/1 (us) | K5w kernel, scalar 1/3 (us) | "
      f"whole call, scalar 1/3 (ms) |")
print("|---|---|---|---|---|")
for cfg_args, np_dt in (((1, 0, 0, 6), torch.float32), ((1, 1, 0, 3), torch.float64),
                        ((1, 0, 255, 3), torch.float32)):
    cfg = mk.MaskConfig(*cfg_args)
    eng = GpuMaskedAggregator(cfg, cfg, N)
    dt = eng._WEIGHT_DTYPES[np_dt]
    gen = torch.Generator().manual_seed(5)
    w_host = (torch.rand(N, generator=gen, dtype=torch.float64) * 2 - 1).to(np_dt)
    w_dev = w_host.to(eng.device)
    mask = eng.derive_mask_values(SEED)
    out = torch.empty(N * eng.bpn, dtype=torch.uint8, device=eng.device)

    kern = {}
    for p, q in ((1, 1), (1, 3)):
        times = {m: [] for m in MODES}
        for rep in range(18):
            for m in MODES:
                t = kernel_us(eng, w_dev, dt, mask, out, p, q, m)
                if rep >= 3:
                    times[m].append(t)
        kern[(p, q)] = times
    del out, mask

    call = {m: [] for m in MODES}
    for rep in range(9):
        for m in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wire = eng.mask_weights(SEED, w_host, 1, 3, exact=(m == "exact"))
            t = (time.perf_counter() - t0) * 1e3  # the call ends in a synchronous D2H
            if rep >= 2:
                call[m].append(t)
    del wire
    for m in MODES:
        print(f"| {cfg_args} bpn {eng.bpn} | {m} | {spread(kern[(1, 1)][m])} | "
              f"{spread(kern[(1, 3)][m])} | {spread(call[m])} |", flush=True)
    del eng, w_dev
    torch.cuda.empty_cache()
