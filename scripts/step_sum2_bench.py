#!/usr/bin/env python3
"""Time one sum2 tick of an in-process participant, with and without gpu_seeds.

A sum participant is restored in its Sum2 phase with a seed dict of `--seeds`
80-byte sealed seeds (1024 by default) for a model of `--length` weights
(Prime/F32/B0/M6). Its tick fetches the dict, opens every seed, sums the masks
and builds its Sum2 message; the transport is local and swallows the message.
The host clock is around that tick, the device synchronised before it stops.
Both variants use the accelerator's batched mask sum (the sum2 hook); they
differ in who opens the seeds: `_core.crypto.sealbox_open` in the participant's
own loop, or GpuBox.open_seeds through the open-seeds hook. Alternated, median
of `--reps` with min..max, after one warm-up tick each; the warm-up ticks also
compare the two variants' Sum2 masks byte for byte.
"""
import argparse
import hashlib
import os
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from xaynet_amd import _core  # noqa: E402
from xaynet_amd.ops.accel import ParticipantAccel  # noqa: E402

co, mk, sdk, crypto = _core.coordinator, _core.mask, _core.sdk, _core.crypto
SIGN_SEED = b"\x07" * 32


def round_params(length):
    s = co.Settings()
    s.model_length = length
    c = mk.MaskConfig(1, 0, 0, 6)
    s.mask_cfg = mk.MaskConfigPair(c, c)
    coord = co.Coordinator(s, co.InMemoryStorage(), co.InMemoryModels(), False)
    coord.start()  # the parameters exist once the first round has begun
    body = b""
    while not body:
        time.sleep(0.01)
        body = bytes(coord.fetch_round_params())
    coord.stop()
    return body


def sum2_state(params, ephm_pk, ephm_sk):
    """Participant.save()'s layout: a sum participant about to run its sum2 step."""
    return (bytes([1, 4, 1, 1]) + struct.pack("<Q", len(params)) + params + bytes(128)
            + ephm_pk + ephm_sk + struct.pack("<I", 0))


def seed_dict(n, ephm_pk):
    out = b"\x01" + struct.pack("<Q", n)
    for i in range(n):
        seed = hashlib.sha256(b"step-sum2-%d" % i).digest()
        out += hashlib.sha256(b"updater-%d" % i).digest() + struct.pack("<Q", 80) \
            + bytes(crypto.sealbox_seal(seed, ephm_pk))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seeds", type=int, default=1024)
    ap.add_argument("--length", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    ephm_pk, ephm_sk = crypto.box_seed_keypair(b"\x21" * 32)
    bodies = {"params": round_params(args.length), "seeds": seed_dict(args.seeds, ephm_pk)}
    state = sum2_state(bodies["params"], ephm_pk, ephm_sk)
    accels = {"cpu opens": ParticipantAccel(), "gpu_seeds": ParticipantAccel(gpu_seeds=True)}
    masks = {}

    def tick(name):
        client = sdk.PyTransportClient(lambda path, pk: bodies.get(path), lambda msg: True)
        p = sdk.Participant.restore(state, client, SIGN_SEED)
        accel = accels[name]
        accel.attach(p)

        def sum2(seeds, length, cfg):
            masks[name] = accel.aggregate_masks(seeds, length, cfg)
            return masks[name]

        p.set_sum2_hook(sum2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p.tick()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if p.phase_id != 1 or masks.get(name) is None:
            raise SystemExit(f"{name}: the sum2 step did not finish on the accelerator")
        return ms

    for name in accels:
        tick(name)  # warm-up: code objects, engines, workspace growth
    if masks["cpu opens"] != masks["gpu_seeds"]:
        raise SystemExit("the two variants' Sum2 masks differ")
    times = {name: [] for name in accels}
    for _ in range(args.reps):
        for name in accels:
            times[name].append(tick(name))
    print(f"step_sum2, {args.seeds} seeds, {args.length} weights; the Sum2 masks are equal")
    print(f"{'variant':10} {'median ms':>10} {'min':>9} {'max':>9}")
    for name, ms in times.items():
        print(f"{name:10} {statistics.median(ms):10.3f} {min(ms):9.3f} {max(ms):9.3f}")


if __name__ == "__main__":
    main()
