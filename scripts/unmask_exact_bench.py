#!/usr/bin/env python3
"""The unmask kernel alone, default mode against exact mode, at 25M elements:
Prime/F32/B0/M6 (u64 order, k4_unmask -> k4_unmask_exact<float, 1>),
Prime/F64/B0/M3 (u128, k4_unmask_u128 -> k4_unmask_exact<double, 2>) and
Prime/F32/Bmax/M3 (five limbs, k4_unmask_offset -> k4_unmask_exact<float, 5>).
One `eng.unmask` call on prepared planes and mask values between two device
events; the modes interleave in one process (default, exact, exact, default),
3 warm-up rounds and 12 timed ones, so 24 timings per mode. The default
kernel is the parent commit's, unchanged, so it is the baseline of the same
session. Figures are median [min, max] in milliseconds, the bytes the kernel
moves (planes and mask rows in, weights out) over the median, and the share
of a round of `--round-ms` (the headline round of bench.py).
Run: python scripts/unmask_exact_bench.py [n_elements] [--round-ms 36.7]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from xaynet_amd import _core
from xaynet_amd.ops import GpuMaskedAggregator
from xaynet_amd.ops.base import _cfg_scalars

mk = _core.mask
args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 25_000_000
ROUND_MS = float(sys.argv[sys.argv.index("--round-ms") + 1]) if "--round-ms" in sys.argv else 36.7
NB = 1000  # participants of scalar 1/1000: the scalar sum is exactly 1
ORDER = ("default", "exact", "exact", "default")


def spread(ts):
    ts = sorted(ts)
    return f"{ts[len(ts) // 2]:.3f} [{ts[0]:.3f}, {ts[-1]:.3f}]"


def prepare(eng, gen):
    """Planes of a plausible aggregate: t = C + d with |d| below exp_shift
    (weights in (-1, 1) against a scalar sum of 1), plus a random mask, as
    canonical values lifted into the accumulator planes; the unit sum that
    makes the divisor exp_shift."""
    info = _cfg_scalars(eng.vect_cfg)
    exp, add = int(info["exp_shift_u64"]), int(info["add_shift"])
    c = NB * add * exp
    order = eng.order_int
    # canonical value rows: low limbs random (they carry d and the mask), the
    # top limbs of (C + mask) mod order from a handful of exact host values
    mask = eng.new_values(zero=True)
    vals = eng.new_values(zero=True)
    lo = torch.randint(0, 2**62, (N,), generator=gen, dtype=torch.int64)
    d = torch.randint(-min(exp, 2**62) + 1, min(exp, 2**62), (N,), generator=gen,
                      dtype=torch.int64)
    if not eng.wide:
        m = lo % order
        mask.copy_(m)
        vals.copy_((m + (c % order) + d) % order)  # order < 2^62 here: no overflow
    else:
        # mask = lo (one limb), t = C + d: t + mask is formed limb-wise on the host
        # for one period of 4096 elements and tiled; the kernels are data-independent
        # but for the handful of ml_mod steps, which every element takes alike here
        period = 4096
        rows_m = [[0] * period for _ in range(eng.n_limbs)]
        rows_v = [[0] * period for _ in range(eng.n_limbs)]
        for i in range(period):
            mi = int(lo[i])
            vi = (c + int(d[i]) + mi) % order
            for j in range(eng.n_limbs):
                rows_m[j][i] = (mi >> (64 * j)) & (2**64 - 1)
                rows_v[j][i] = (vi >> (64 * j)) & (2**64 - 1)

        def signed(rows):
            return torch.tensor([[x - 2**64 if x >= 2**63 else x for x in r] for r in rows],
                                dtype=torch.int64)

        reps = -(-N // period)
        mask.copy_(signed(rows_m).repeat(1, reps)[:, :N])
        vals.copy_(signed(rows_v).repeat(1, reps)[:, :N])
    eng.acc.zero_()
    eng.values_to_planes(vals, eng.acc)
    eng.nb_models = NB
    mask_unit = 12345
    eng.unit_acc = (c + exp + mask_unit) % int(eng.unit_cfg.order)  # n1 = C + exp: Q = exp
    return mask, mask_unit


def unmask_ms(eng, mask, mask_unit, exact):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = eng.unmask(mask, mask_unit, nb_models=NB, exact=exact)
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


print(f"n = {N}, {NB} participants, round = {ROUND_MS} ms")
print("| config | mode | unmask kernel (ms) | GB/s at the median | share of the round |")
print("|---|---|---|---|---|")
for cfg_args in ((1, 0, 0, 6), (1, 1, 0, 3), (1, 0, 255, 3)):
    cfg = mk.MaskConfig(*cfg_args)
    eng = GpuMaskedAggregator(cfg, cfg, N)
    mask, mask_unit = prepare(eng, torch.Generator().manual_seed(5))
    _, vinfo, dt = eng._unmask_scalars(mask_unit, NB)
    assert vinfo["exact_divisor"] == int(_cfg_scalars(cfg)["exp_shift_u64"])
    times = {"default": [], "exact": []}
    outs = {}
    for rep in range(15):
        for mode in ORDER:
            t, out = unmask_ms(eng, mask, mask_unit, mode == "exact")
            if rep >= 3:
                times[mode].append(t)
            outs[mode] = out
    # the modes agree to the default mode's error bound: a sanity check of the inputs
    diff = (outs["default"].double() - outs["exact"].double()).abs().max().item()
    moved = N * 8 * (eng.n_digits + (eng.n_limbs if eng.wide else 1)) + N * outs["exact"].element_size()
    for mode in ("default", "exact"):
        med = sorted(times[mode])[len(times[mode]) // 2]
        print(f"| {cfg_args} bpn {eng.bpn} L {eng.n_limbs} | {mode} | {spread(times[mode])} | "
              f"{moved / med / 1e6:.0f} | {100 * med / ROUND_MS:.1f} % |", flush=True)
    print(f"  max |default - exact| = {diff:.3g}", flush=True)
    del eng, mask, outs, out
    torch.cuda.empty_cache()
