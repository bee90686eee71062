#!/usr/bin/env python3
"""Unmasked weights on the device -> host-visible Option<Model> bincode body,
two ways, at 1M and 25M f32 and 25M f64 weights drawn from U(-1, 1):
  cpu  the former path: out.cpu().numpy() + _core.sdk.encode_model (16 threads)
  gpu  eng.encode_model(out): K7 kernels + one D2H into pinned memory
Both run in one process, alternating, each timed region between two device
synchronises on the host clock (3 warm-up rounds, 11 timed); median [min, max].
The gpu path is also split: the kernels (count, scan, the 8-byte read-back of
the total, emit: one _hip._model_encode call on prepared buffers), the D2H
copy, and the host copy supply_unmasked_model makes of the pinned view (and,
for the cpu path, of the bytes object). Kernel traffic is the body written
plus the weights read twice, against the 6.29 TB/s copy rate of the HBM.

Run: python scripts/model_encode_bench.py [--out FILE]
The table replaces the text between the `table:begin` / `table:end` markers
of FILE (default profiles/r11_model_encode.md)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from xaynet_amd import _core, _hip
from xaynet_amd.ops import GpuMaskedAggregator

mk, co, sdk = _core.mask, _core.coordinator, _core.sdk
WARM, REPS = 3, 11
HBM_COPY_TBS = 6.29
CASES = ((1_000_000, torch.float32), (25_000_000, torch.float32), (25_000_000, torch.float64))
BEGIN, END = "<!-- table:begin -->", "<!-- table:end -->"


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(ts):
    med, lo, hi = stats(ts)
    return f"{med:.2f} [{lo:.2f}, {hi:.2f}]"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def staged_coordinator(n):
    s = co.Settings()
    s.model_length = n
    c = mk.MaskConfig(1, 0, 0, 3)
    s.mask_cfg = mk.MaskConfigPair(c, c)
    return co.Coordinator(s, co.InMemoryStorage(), co.InMemoryModels(), True)


def run_case(eng, n, dtype, lines):
    gen = torch.Generator().manual_seed(11)
    out = (torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1).to(dtype).to(eng.acc.device)
    dt = eng._WEIGHT_DTYPES[dtype]
    name = f"{n // 1_000_000}M {'f32' if dtype == torch.float32 else 'f64'}"

    paths = {"cpu": lambda: sdk.encode_model(out.cpu().numpy()),
             "gpu": lambda: eng.encode_model(out)}
    t = {k: [] for k in paths}
    for rep in range(WARM + REPS):
        for k, fn in paths.items():
            ms, body = timed(fn)
            if rep >= WARM:
                t[k].append(ms)
            if rep == 0:
                if k == "cpu":
                    ref = np.frombuffer(body, dtype=np.uint8)
                else:
                    assert np.array_equal(ref, body), "GPU body differs from the CPU encoder's"
                    del ref
            del body
    nbytes = len(eng.encode_model(out))

    # the gpu path's parts, on the engine's own cached buffers
    work, dev, pin = eng._enc_work, eng._enc_dev, eng._enc_pin[: 3 + nbytes]
    parts = {"kernels": lambda: _hip._model_encode(out.data_ptr(), dt, n, work.data_ptr(),
                                                   dev.data_ptr(), dev.numel()),
             "d2h": lambda: pin.copy_(dev[: 3 + nbytes])}
    coord = staged_coordinator(n)
    view = pin.numpy()[3:]
    as_bytes = sdk.encode_model(out.cpu().numpy())
    parts["supply(view)"] = lambda: coord.supply_unmasked_model(view)
    parts["supply(bytes)"] = lambda: coord.supply_unmasked_model(as_bytes)
    p = {k: [] for k in parts}
    for rep in range(WARM + REPS):
        for k, fn in parts.items():
            ms, _ = timed(fn)
            if rep >= WARM:
                p[k].append(ms)
    del coord, as_bytes, view

    traffic = nbytes + 2 * n * out.element_size()
    kern_tbs = traffic / (stats(p["kernels"])[0] * 1e-3) / 1e12
    d2h_gbs = nbytes / (stats(p["d2h"])[0] * 1e-3) / 1e9
    lines.append(f"| {name} | {nbytes / 1e6:.1f} | {fmt(t['cpu'])} | {fmt(t['gpu'])} | "
                 f"{fmt(p['kernels'])} | {fmt(p['d2h'])} | {fmt(p['supply(view)'])} | "
                 f"{fmt(p['supply(bytes)'])} | {kern_tbs:.2f} ({100 * kern_tbs / HBM_COPY_TBS:.0f}%) | "
                 f"{d2h_gbs:.1f} |")
    print(lines[-1], flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_model_encode.md"))
    args = ap.parse_args()
    cfg = mk.MaskConfig(1, 0, 0, 3)
    eng = GpuMaskedAggregator(cfg, cfg, 16, device="cuda:0")  # encode_model takes any length
    lines = ["| weights | body (MB) | cpu path (ms) | gpu path (ms) | gpu: kernels (ms) | "
             "gpu: D2H (ms) | supply, pinned view (ms) | supply, bytes (ms) | "
             "kernel traffic (TB/s, of 6.29) | D2H (GB/s) |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    verdict = None
    for n, dtype in CASES:
        t = run_case(eng, n, dtype, lines)
        if (n, dtype) == (25_000_000, torch.float32):
            (cm, cl, ch), (gm, gl, gh) = stats(t["cpu"]), stats(t["gpu"])
            wins = cm - gm > (ch - cl) + (gh - gl)
            verdict = (f"25M f32: gpu median {gm:.1f} ms against cpu median {cm:.1f} ms; the "
                       f"difference {cm - gm:.1f} ms is {'above' if wins else 'NOT above'} the "
                       f"spread of both ({ch - cl:.1f} + {gh - gl:.1f} ms): the driver "
                       f"{'uses' if wins else 'does not use'} the GPU encoder.")
    lines += ["", verdict]
    print(verdict, flush=True)
    table = "\n".join(lines)
    text = open(args.out).read() if os.path.exists(args.out) else f"{BEGIN}\n{END}\n"
    if BEGIN in text and END in text:
        text = text[: text.index(BEGIN) + len(BEGIN)] + "\n" + table + "\n" + text[text.index(END):]
    else:
        text += f"\n{BEGIN}\n{table}\n{END}\n"
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
