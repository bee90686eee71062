#!/usr/bin/env python3
"""Digit planes on the device -> host-visible Option<Model> body, the rational
mode (K7r) against the default path, at 1M and 25M weights for L = 1
(Prime/F32/B0/M6, the benchmark's config) and L = 5 (Prime/F32/Bmax/M3):
  rational   eng.encode_model_rational: k7r_words, scan, k7r_emit, one D2H
  default    eng.encode_model(eng.unmask(...)): K4 + K7, one D2H
  cpu        Aggregation.unmask + encode_option_model, the CPU plane's producer
             of the rational bytes (1M only: the BigInt gcd takes seconds)
The round is three participants of scalar 1 with weights from U(-1, 1): Q = 3 *
exp_shift and d the sum of three quantised weights, on a pattern of 65536
elements built in Python integers and tiled on the device. Paths alternate in
one process, each timed region between two device synchronises on the host
clock (3 warm-up rounds, 11 timed); median [min, max] in ms. The kernels of the
rational path are also timed alone (one _hip._model_encode_rational call on
prepared buffers).

Run: python scripts/model_encode_ratio_bench.py [--out FILE] [--sizes 1,25]
The table replaces the text between the `table:begin` / `table:end` markers
of FILE (default profiles/r17_model_encode_rational.md)."""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from xaynet_amd import _core, _hip
from xaynet_amd.ops import GpuMaskedAggregator

mk, sdk = _core.mask, _core.sdk
WARM, REPS = 3, 11
PATTERN = 65536
CONFIGS = {1: ((1, 0, 0, 6), 10**10, 1), 5: ((1, 0, 255, 3), 10**45, (2**24 - 1) << 104)}
BEGIN, END = "<!-- table:begin -->", "<!-- table:end -->"


def fmt(ts):
    ts = sorted(ts)
    return f"{ts[len(ts) // 2]:.2f} [{ts[0]:.2f}, {ts[-1]:.2f}]"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def rows(ints, count):
    """Python ints -> [count, n] int64 rows of 64-bit limbs."""
    return torch.from_numpy(np.stack([
        np.array([(v >> (64 * j)) & (2**64 - 1) for v in ints], dtype=np.uint64)
        for j in range(count)]).view(np.int64))


def planes32(ints, count):
    return torch.from_numpy(np.stack([
        np.array([(v >> (32 * j)) & 0xFFFFFFFF for v in ints], dtype=np.uint64)
        for j in range(count)]).view(np.int64))


def tile(t, n):
    reps = -(-n // t.shape[-1])
    return t.repeat(*([1] * (t.dim() - 1)), reps)[..., :n].contiguous().cuda()


def build_round(n_limbs, n):
    cfg_args, exp, add = CONFIGS[n_limbs]
    cfg = mk.MaskConfig(*cfg_args)
    order, nb = int(cfg.order), 3
    c, q = nb * add * exp, nb * exp
    rng = random.Random(17 + n_limbs)
    d = [sum(int(rng.uniform(-1, 1) * exp) for _ in range(nb)) for _ in range(PATTERN)]
    mask = [rng.randrange(order) for _ in range(PATTERN)]
    masked = [(c + v + m) % order for v, m in zip(d, mask)]
    eng = GpuMaskedAggregator(cfg, cfg, n, device="cuda:0")
    assert eng.n_limbs == n_limbs
    eng.acc.copy_(tile(planes32(masked, eng.n_digits), n))
    mask_t = tile(rows(mask, n_limbs), n) if eng.wide else tile(rows(mask, 1)[0], n)
    vals_t = tile(rows(masked, n_limbs), n) if eng.wide else tile(rows(masked, 1)[0], n)
    mask_unit = rng.randrange(order)
    eng.unit_acc = (q + c + mask_unit) % order
    return eng, cfg, mask_t, vals_t, mask_unit, nb, (d, q)


def run_case(n_limbs, n, lines):
    eng, cfg, mask, vals, mu, nb, (d, q) = build_round(n_limbs, n)
    name = f"L={n_limbs} {n // 1_000_000}M"
    paths = {"rational": lambda: eng.encode_model_rational(mask, mu, nb_models=nb),
             "default": lambda: eng.encode_model(eng.unmask(mask, mu, nb_models=nb))}
    if n <= 1_000_000:
        pair = mk.MaskConfigPair(cfg, cfg)
        agg, mask_agg = mk.Aggregation(pair, n), mk.Aggregation(pair, n)
        agg.set(mk.MaskObject.deserialize(eng.wire_object(eng.pack_wire(vals), eng.unit_acc)), nb)
        mask_agg.set(mk.MaskObject.deserialize(eng.wire_object(eng.pack_wire(mask), mu)), nb)
        paths["cpu"] = lambda: agg.unmask_body(mask_agg.object)
    t = {k: [] for k in paths}
    sizes = {}
    for rep in range(WARM + REPS):
        for k, fn in paths.items():
            if k == "cpu" and rep >= 3:  # seconds a run: three runs, all timed
                continue
            ms, body = timed(fn)
            if rep >= WARM or k == "cpu":
                t[k].append(ms)
            if rep == 0:
                sizes[k] = len(body)
                if k == "rational":
                    head = sdk.model_codec_encode_ratio(
                        [v < 0 for v in d], [abs(v) for v in d], q, limbs=n_limbs)
                    m = min(n, PATTERN)
                    want = np.frombuffer(head, dtype=np.uint8)
                    if n <= PATTERN:
                        assert np.array_equal(body, want), "rational body differs"
                    else:  # the pattern repeats: the first tile's elements, then again
                        assert np.array_equal(body[9:len(want)], want[9:]), "first tile differs"
                        assert np.array_equal(body[len(want):2 * len(want) - 9], want[9:]), \
                            "second tile differs"
                        rem = d[: n % PATTERN]
                        tail = sdk.model_codec_encode_ratio(
                            [v < 0 for v in rem], [abs(v) for v in rem], q, limbs=n_limbs)[9:]
                        assert len(body) == 9 + (n // m) * (len(want) - 9) + len(tail)
                        if tail:  # past every block base of the scan
                            assert bytes(body[-len(tail):]) == tail, "last tile differs"
                if k == "cpu":
                    assert bytes(body) == eng.encode_model_rational(mask, mu, nb_models=nb).tobytes()
            del body

    # the rational path's kernels alone, on the engine's cached buffers
    eng.encode_model_rational(mask, mu, nb_models=nb)
    _, vinfo, _ = eng._unmask_scalars(mu, nb)
    lo, hi, _ = eng._vals(mask)
    args = (eng.acc.data_ptr(), lo, hi, n, eng.n_digits, eng.order, 32, str(vinfo["offset"]),
            str(vinfo["exact_divisor"]))
    work = eng._enc_buffer("_enc_work", _hip._model_ratio_plan(n, eng.order)["work_bytes"])
    kt = []
    for rep in range(WARM + REPS):
        ms, _ = timed(lambda: _hip._model_encode_rational(
            *args, work.data_ptr(), eng._enc_dev.data_ptr(), eng._enc_dev.numel()))
        if rep >= WARM:
            kt.append(ms)
    cells = fmt(kt)
    lines.append(f"| {name} | {sizes['rational'] / n:.1f} | {sizes['default'] / n:.1f} | "
                 f"{fmt(t['rational'])} | {fmt(t['default'])} | "
                 f"{fmt(t['cpu']) if t.get('cpu') else '-'} | {cells} |")
    print(lines[-1], flush=True)
    del eng, mask, vals
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_model_encode_rational.md"))
    ap.add_argument("--sizes", default="1,25", help="millions of weights, comma separated")
    args = ap.parse_args()
    kcols = ["kernels (ms)"]
    lines = ["| round | rational body (B/weight) | default body (B/weight) | rational (ms) | "
             "default K4 + K7 (ms) | cpu producer (ms) | " + " | ".join(kcols) + " |",
             "|---|---|---|---|---|---|" + "---|" * len(kcols)]
    print("\n".join(lines), flush=True)
    for n_limbs in (1, 5):
        for m in (int(x) for x in args.sizes.split(",")):
            run_case(n_limbs, m * 1_000_000, lines)
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
