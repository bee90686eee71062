"""Participant-side GPU accelerator: wires the MI355X kernels into the SDK's
update-masking and sum2 mask-aggregation hot loops.

Usage:
    accel = ParticipantAccel()          # auto-configures per round
    accel.attach(participant)           # sets both hooks
    # or: xaynet_sdk.Participant(url, gpu=True) / spawn_participant(gpu=True)
    # ParticipantAccel(exact=True) / spawn_participant(gpu=True, gpu_exact=True):
    # the masked update equals the CPU masker's byte for byte

The hooks receive the round's mask config + model length from the SDK and
lazily build (and cache) one engine per (config, length). They fall back to
the CPU path (return None) on any error, so a GPU-less box or an
out-of-range config degrades cleanly. Replaces: Masker::mask
(masking.rs:358-404) via K1+K5w and the sum2 derive+aggregate loop
(xaynet-sdk sum2.rs:170-190) via batched K1 and a row sum into digit planes
(ops/sum2.py)."""
from __future__ import annotations

import logging
import threading

import numpy as np

LOG = logging.getLogger("xaynet.accel")

_NP_DTYPES = {0: np.float32, 1: np.float64, 2: np.int32, 3: np.int64}


class ParticipantAccel:
    def __init__(self, device: str = "cuda:0", scalar_num: int = 1, scalar_den: int = 1,
                 exact: bool = False):
        """exact=False masks with the constructor's scalar through the
        double-precision K5w kernel. exact=True masks with the scalar the hook
        hands over (the participant's own) in exact mode: the update is the
        CPU masker's, byte for byte."""
        import torch

        self.torch = torch
        self.device = device
        self.scalar_num = scalar_num
        self.scalar_den = scalar_den
        self.exact = exact
        # one accelerator may be shared by many participants (threads): the
        # engines + scratch are serialized under a lock
        self._mu = threading.Lock()
        self._engines = {}  # (cfg8, length) -> (engine, total, scratch)

    def _engine_for(self, cfg8, length: int):
        key = (tuple(cfg8), length)
        ent = self._engines.get(key)
        if ent is None:
            from xaynet_amd import _core

            from .engine import GpuMaskedAggregator

            mk = _core.mask
            eng = GpuMaskedAggregator(mk.MaskConfig(*cfg8[:4]), mk.MaskConfig(*cfg8[4:]), length,
                                      device=self.device)
            ent = (eng, eng.new_values(), eng.new_values())
            self._engines[key] = ent
        return ent

    # ---- hooks ----

    def mask_model(self, seed: bytes, dtype: int, raw: bytes, n: int, cfg8,
                   scalar_num: int | None = None, scalar_den: int | None = None):
        """scalar_num/scalar_den: the participant's scalar, as the SDK hook
        passes it; used in exact mode only. A scalar the exact kernel cannot
        take (a term of 2^63 or more) gives None, the CPU fallback."""
        with self._mu:
            try:
                eng = self._engine_for(cfg8, n)[0]
                w = np.frombuffer(raw, dtype=_NP_DTYPES[dtype])
                t = self.torch.from_numpy(w.copy())
                if self.exact:
                    if scalar_num is None or scalar_den is None:
                        raise ValueError("exact mode needs the participant's scalar")
                    if not (0 <= scalar_num < 2**63 and 0 < scalar_den < 2**63):
                        LOG.info("scalar past 2^63: update masking stays on the CPU")
                        return None
                    return eng.mask_weights(seed, t, int(scalar_num), int(scalar_den),
                                            exact=True)
                return eng.mask_weights(seed, t, self.scalar_num, self.scalar_den)
            except Exception:  # noqa: BLE001 — CPU fallback
                LOG.exception("GPU mask_model hook failed; falling back to CPU")
                return None

    def aggregate_masks(self, seeds, length: int, cfg8):
        with self._mu:
            try:
                from .sum2 import aggregate_masks_on

                return aggregate_masks_on(*self._engine_for(cfg8, length), seeds)
            except Exception:  # noqa: BLE001
                LOG.exception("GPU sum2 hook failed; falling back to CPU")
                return None

    def attach(self, participant) -> None:
        participant.set_mask_model_hook(self.mask_model)
        participant.set_sum2_hook(self.aggregate_masks)
