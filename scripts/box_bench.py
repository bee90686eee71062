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

--device-keys measures K9 instead: per shape (default 4096 x 4 KiB and the seed
dicts 1024 x 32 B and 10240 x 32 B) and direction, `device_keys=True` (X25519,
key and nonce on the device), `device_keys=False` (the ladders on the host) and
the CPU box are taken alternately, --reps rounds, after a warm-up call that
compares every byte; medians with min..max. --seed-sweep times
GpuBox.open_seeds / seal_seed (host bytes in and out) against the CPU loop over
batch sizes, which is what GpuBox.SEEDS_MIN_BATCH is read from, and
x25519_batch against `_core.crypto.x25519`.

--verify measures K10: GpuBox.verify_batch over 64 .. 65536 signatures (powers
of four) of 38-byte and 4 KiB messages against `_core.crypto.verify_detached`
on one core (timed up to 4096 signatures), and GpuBox.open_messages against
`sealbox_open_batch(device_keys=True)` followed by a CPU verify loop over the
plaintexts copied back. Rounds alternate after a warm-up that compares every
result with the CPU's.

Usage (GPU box): python scripts/box_bench.py [--reps 5] [--shapes 1x175000000,64x8388608]
                 python scripts/box_bench.py --device-keys [--seed-sweep]
                 python scripts/box_bench.py --verify
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


def spread(v):
    return {"median": round(statistics.median(v), 3), "min_max": [round(min(v), 3),
                                                                  round(max(v), 3)]}


def device_keys_bench(args):
    box = GpuBox("cuda:0", time_kernels=True)
    pk, sk = cr.box_seed_keypair(b"\x42" * 32)
    rng = np.random.default_rng(19)
    for shape in (args.shapes or "4096x4096,1024x32,10240x32").split(","):
        count, size = (int(x) for x in shape.split("x"))
        msgs = [rng.bytes(size) for _ in range(count)]
        sealed = [bytes(cr.sealbox_seal(m, pk)) for m in msgs]
        # warm-up, every byte compared
        opened, ok = box.sealbox_open_batch(sealed, pk, sk, device_keys=True)
        assert bool(ok.all()) and all(bytes(t.cpu().numpy()) == m for t, m in zip(opened, msgs))
        resealed = box.sealbox_seal_batch(msgs, pk, device_keys=True)
        assert all(cr.sealbox_open(bytes(t.cpu().numpy()), pk, sk) == m
                   for t, m in zip(resealed, msgs))
        box.sealbox_open_batch(sealed, pk, sk)
        box.sealbox_seal_batch(msgs, pk)
        del opened, resealed
        for name, gpu, cpu in (
            ("open", lambda dk: box.sealbox_open_batch(sealed, pk, sk, device_keys=dk),
             lambda: [cr.sealbox_open(s, pk, sk) for s in sealed]),
            ("seal", lambda dk: box.sealbox_seal_batch(msgs, pk, device_keys=dk),
             lambda: [cr.sealbox_seal(m, pk) for m in msgs]),
        ):
            t = {"dev_kernel": [], "dev_call": [], "host_kernel": [], "host_call": [], "cpu": []}
            for _ in range(args.reps):
                t["dev_call"] += timed(lambda: gpu(True), 1)
                t["dev_kernel"].append(box.kernel_ms)
                t["host_call"] += timed(lambda: gpu(False), 1)
                t["host_kernel"].append(box.kernel_ms)
                t["cpu"] += timed(cpu, 1)
            print(json.dumps({"op": name, "boxes": count, "bytes_per_box": size,
                              "reps": args.reps,
                              "device_keys_kernel_ms": spread(t["dev_kernel"]),
                              "device_keys_call_ms": spread(t["dev_call"]),
                              "host_keys_kernel_ms": spread(t["host_kernel"]),
                              "host_keys_call_ms": spread(t["host_call"]),
                              "cpu_ms_one_thread": spread(t["cpu"])}), flush=True)
    if not args.seed_sweep:
        return
    GpuBox.SEEDS_MIN_BATCH = 0
    for n in (4, 16, 64, 256, 1024, 4096, 16384, 65536):
        seeds = [rng.bytes(32) for _ in range(n)]
        enc = [bytes(cr.sealbox_seal(s, pk)) for s in seeds]
        pks = [cr.x25519_base(s) for s in seeds]
        assert box.open_seeds(enc, pk, sk) == seeds
        assert box.x25519_batch(seeds[:64], pks[:64]) == \
            [cr.x25519(a, b) for a, b in zip(seeds[:64], pks[:64])]
        box.seal_seed(seeds[0], pks)
        t = {"open_gpu": [], "open_cpu": [], "seal_gpu": [], "seal_cpu": [], "x25519_gpu": [],
             "x25519_cpu": []}
        for _ in range(args.reps):
            t["open_gpu"] += timed(lambda: box.open_seeds(enc, pk, sk), 1)
            t["open_cpu"] += timed(lambda: [cr.sealbox_open(e, pk, sk) for e in enc], 1)
            t["seal_gpu"] += timed(lambda: box.seal_seed(seeds[0], pks), 1)
            t["seal_cpu"] += timed(lambda: [cr.sealbox_seal(seeds[0], k) for k in pks], 1)
            t["x25519_gpu"] += timed(lambda: box.x25519_batch(seeds, pks), 1)
            if n <= 4096:
                t["x25519_cpu"] += timed(lambda: [cr.x25519(a, b) for a, b in zip(seeds, pks)],
                                         1)
        print(json.dumps({"seeds": n, "reps": args.reps,
                          **{k + "_ms": spread(v) for k, v in t.items() if v}}), flush=True)


def verify_bench(args):
    box = GpuBox("cuda:0", time_kernels=True)
    rng = np.random.default_rng(20)
    spk, ssk = cr.sign_keypair_from_seed(b"\x43" * 32)
    for size in (38, 4096):
        msgs = [rng.bytes(size) for _ in range(65536)]
        sigs = [cr.sign_detached(m, ssk) for m in msgs]
        for j in range(0, 65536, 5):  # every fifth signature is wrong
            sigs[j] = sigs[j][:40] + bytes([sigs[j][40] ^ 1]) + sigs[j][41:]
        for n in (64, 256, 1024, 4096, 16384, 65536):
            g, m = sigs[:n], msgs[:n]
            got = box.verify_batch(g, m, spk)
            assert got == [j % 5 != 0 for j in range(n)]
            if n <= 4096:
                assert got == [cr.verify_detached(a, b, spk) for a, b in zip(g, m)]
            t = {"kernel": [], "call": [], "cpu": []}
            for _ in range(args.reps):
                t["call"] += timed(lambda: box.verify_batch(g, m, spk), 1)
                t["kernel"].append(box.kernel_ms)
                if n <= 4096:
                    t["cpu"] += timed(lambda: [cr.verify_detached(a, b, spk)
                                               for a, b in zip(g, m)], 1)
            print(json.dumps({"op": "verify_batch", "signatures": n, "bytes_per_message": size,
                              "reps": args.reps,
                              **{k + "_ms": spread(v) for k, v in t.items() if v}}), flush=True)
    # update messages of 4 KiB: three signatures each
    pk, sk = cr.box_seed_keypair(b"\x42" * 32)
    seed = b"\x5e" * 32
    tasks = cr.sign_detached(seed + b"sum", ssk) + cr.sign_detached(seed + b"update", ssk)
    for n in (64, 1024, 4096):
        sealed = []
        for _ in range(n):
            body = spk + pk + (4096).to_bytes(4, "big") + bytes([2, 0, 0, 0]) + tasks + \
                rng.bytes(4096 - 264)
            sealed.append(bytes(cr.sealbox_seal(cr.sign_detached(body, ssk) + body, pk)))

        def host_path():
            box.sealbox_open_batch(sealed, pk, sk, device_keys=True)
            host = box.opened_buffer.cpu().numpy()
            out = []
            for off in box.opened_offsets:
                p = host[off:off + 4096].tobytes()
                out.append(cr.verify_detached(p[:64], p[64:], p[64:96]) +
                           2 * cr.verify_detached(p[136:200], seed + b"sum", p[64:96]) +
                           4 * cr.verify_detached(p[200:264], seed + b"update", p[64:96]))
            return out

        assert box.open_messages(sealed, pk, sk, round_seed=seed)[1] == host_path() == [7] * n
        t = {"open_messages": [], "open_then_cpu_verify": []}
        for _ in range(args.reps):
            t["open_messages"] += timed(lambda: box.open_messages(sealed, pk, sk, seed), 1)
            t["open_then_cpu_verify"] += timed(host_path, 1)
        print(json.dumps({"op": "open_messages", "messages": n, "bytes_per_message": 4096,
                          "reps": args.reps, **{k + "_ms": spread(v) for k, v in t.items()}}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--device-keys", action="store_true")
    ap.add_argument("--seed-sweep", action="store_true")
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    if args.verify:
        return verify_bench(args)
    if args.device_keys:
        return device_keys_bench(args)
    args.shapes = args.shapes or "1x175000000,64x8388608,4096x4096"

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
