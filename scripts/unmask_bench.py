#!/usr/bin/env python3
"""K4 unmask time at 1M elements, i64 configs: a u64 order (Prime/I64/B2/M3)
and a wide one (Prime/I64/B6/M3), 3 participants of scalar 1/3, i64 and f32
outputs. One `eng.unmask` call between two events, 5 warm-up calls and 30
timed ones, so the figure includes the host path of the call.
Run: python scripts/unmask_bench.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from xaynet_amd import _core
from xaynet_amd.ops import GpuMaskedAggregator

mk = _core.mask
N, K = 1_000_000, 3

for cfg_args in ((1, 3, 2, 3), (1, 3, 6, 3)):
    cfg = mk.MaskConfig(*cfg_args)
    eng = GpuMaskedAggregator(cfg, cfg, N)
    order = int(cfg.order)
    mask_unit = 0
    for p in range(K):
        seed = bytes([p + 1]) * 32
        eng.unit_acc = (eng.unit_acc + eng.masked_unit_for(seed, 1, K)) % order
        mask_unit = (mask_unit + eng.unit_draw(seed)) % order
    mask = eng.derive_mask_values(b"\x07" * 32)
    eng.acc.copy_(torch.randint(0, 2**32, eng.acc.shape, dtype=torch.int64, device="cuda") * K)
    for dtype, name in ((3, "i64"), (0, "f32")):
        for _ in range(5):
            out = eng.unmask(mask, mask_unit, nb_models=K, dtype=dtype)
        torch.cuda.synchronize()
        times = []
        for _ in range(30):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = eng.unmask(mask, mask_unit, nb_models=K, dtype=dtype)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        times.sort()
        print(f"cfg {cfg_args} bpn {eng.bpn} out {name}: median {times[15]:.1f} us, "
              f"min {times[0]:.1f} us, max {times[-1]:.1f} us per unmask of {N} elements",
              flush=True)
