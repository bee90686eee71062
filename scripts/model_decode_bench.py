#!/usr/bin/env python3
"""Option<Model> bincode body on the host -> weights, two ways, at 1M and 25M
f32, f64 and i32 weights and at 10k f32 (floats from U(-1, 1), integers over the whole i32
range):
  cpu  the former path: _core.sdk.decode_model (16 threads for f32/f64, the
       rational path for i32), the result left on the host as before
  gpu  eng.decode_model(body): the body across PCIe once, the K7d kernels, the
       weights left on the device
Both run in one process in cpu, gpu, gpu, cpu order per round (1 warm-up round,
3 timed), each timed region between two device synchronises on the host clock;
median [min, max]. The gpu path runs once per way of getting a `bytes` body
across (engine._upload_body): a pageable copy, a copy through the cached pinned
buffer, and _hip.host_register on the body for the copy. It is also split: the
upload alone per way, and the kernels alone (one _hip._model_decode call on the
uploaded body: block maps, resolve, emit and the status read-back). The i32
cpu path is measured at 1M only; its 25M figure is 25 times that, marked `~`.

Run: python scripts/model_decode_bench.py [--out FILE] [--small]
The table replaces the text between the `table:begin` / `table:end` markers
of FILE (default profiles/r13_model_decode.md)."""
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

mk, sdk = _core.mask, _core.sdk
WARM, REPS = 1, 3
WAYS = ("pageable", "pinned", "register")
CASES = ((10_000, "float32"), (1_000_000, "float32"), (25_000_000, "float32"), (1_000_000, "float64"),
         (25_000_000, "float64"), (1_000_000, "int32"), (25_000_000, "int32"))
CODE = {"float32": 0, "float64": 1, "int32": 2}
BEGIN, END = "<!-- table:begin -->", "<!-- table:end -->"


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(ts, mark=""):
    if not ts:
        return "failed"
    med, lo, hi = stats(ts)
    return f"{mark}{med:.2f} [{lo:.2f}, {hi:.2f}]"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def weights(n, name):
    rng = np.random.default_rng(13)
    if name == "int32":
        return rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
    return rng.uniform(-1, 1, n).astype(name)


def run_case(eng, n, name, lines, cpu_1m):
    code = CODE[name]
    w = weights(n, name)
    body = sdk.encode_model(w)
    nbytes = len(body)
    src = np.frombuffer(body, dtype=np.uint8)
    measure_cpu = name != "int32" or n <= 1_000_000
    bits = np.uint32 if w.itemsize == 4 else np.uint64

    t = {"cpu": [], **{way: [] for way in WAYS}}
    broken = set()
    for rep in range(WARM + REPS):
        order = ["cpu", *WAYS, *WAYS, "cpu"]
        for k in order:
            if k == "cpu":
                if not measure_cpu:
                    continue
                ms, got = timed(lambda: sdk.decode_model(body, code))
                ok = np.array_equal(got.view(bits), w.view(bits))
            elif k in broken:
                continue
            else:
                eng._DEC_STAGING = k
                try:
                    ms, got = timed(lambda: eng.decode_model(body, code))
                except RuntimeError as e:  # a way this machine does not offer
                    print(f"{k}: {e}", flush=True)
                    broken.add(k)
                    t[k] = []
                    continue
                ok = got is not None and (rep > 0 or np.array_equal(
                    got.cpu().numpy().view(bits), w.view(bits)))
            assert ok, (n, name, k)
            if rep >= WARM:
                t[k].append(ms)
            del got
    if not measure_cpu:
        t["cpu"] = [25 * x for x in cpu_1m]

    # the parts, on the engine's own cached buffers
    dev, work, out = eng._dec_dev, eng._dec_work, eng._dec_out
    p = {f"h2d {way}": [] for way in WAYS}
    p["kernels"] = []
    for rep in range(WARM + REPS):
        for way in WAYS:
            if way in broken:
                continue
            ms, _ = timed(lambda: eng._upload_body(src, dev, way))
            if rep >= WARM:
                p[f"h2d {way}"].append(ms)
        ms, rejected = timed(lambda: _hip._model_decode(dev.data_ptr() + 3, nbytes, code, n,
                                                        work.data_ptr(), out.data_ptr()))
        assert rejected == 0
        if rep >= WARM:
            p["kernels"].append(ms)

    best = min((way for way in WAYS if way not in broken), key=lambda way: stats(t[way])[0])
    label = f"{n // 1_000_000}M {name}" if n >= 1_000_000 else f"{n // 1000}k {name}"
    lines.append(f"| {label} | {nbytes / 1e6:.1f} | {fmt(t['cpu'], '' if measure_cpu else '~')} | "
                 + " | ".join(fmt(t[way]) for way in WAYS) + " | "
                 + " | ".join(fmt(p[f'h2d {way}']) for way in WAYS)
                 + f" | {fmt(p['kernels'])} | {best} | "
                 f"{stats(t['cpu'])[0] / stats(t[best])[0]:.1f}x |")
    print(lines[-1], flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_model_decode.md"))
    ap.add_argument("--small", action="store_true", help="the 1M cases only")
    args = ap.parse_args()
    cfg = mk.MaskConfig(1, 0, 0, 3)
    eng = GpuMaskedAggregator(cfg, cfg, 16, device="cuda:0")  # decode_model takes any length
    lines = ["| weights | body (MB) | cpu decode (ms) | gpu, pageable (ms) | gpu, pinned (ms) | "
             "gpu, registered (ms) | H2D pageable (ms) | H2D pinned (ms) | H2D registered (ms) | "
             "kernels (ms) | fastest | cpu / fastest gpu |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    cpu_1m = {}
    for n, name in CASES:
        if args.small and n > 1_000_000:
            continue
        t = run_case(eng, n, name, lines, cpu_1m.get(name))
        if n == 1_000_000:
            cpu_1m[name] = t["cpu"]
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
