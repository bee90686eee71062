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
(ops/sum2.py). decode_model is no hook: the SDK wrapper's
global_model_tensor() calls it to decode the fetched global model on the
device (K7d), with the CPU decoder behind it for bodies the kernels reject."""
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
        self._dec_engine = None  # decode_model's own, where no round has built one

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

    # Bodies shorter than this stay on the CPU decoder in decode_model. 0: the
    # kernel path is 4.7x ahead at 1M f32 weights and 5.5x at 25M, and at 10k
    # it is 0.06 ms behind, less than the upload the CPU result would still
    # need (scripts/model_decode_bench.py, profiles/r13_model_decode.md).
    DECODE_MIN_BYTES = 0

    def _decode_engine(self):
        """Decoding does not depend on the mask config: any cached engine
        serves, else a small dedicated one."""
        if self._engines:
            return next(iter(self._engines.values()))[0]
        if self._dec_engine is None:
            from xaynet_amd import _core

            from .engine import GpuMaskedAggregator

            cfg = _core.mask.MaskConfig(1, 0, 0, 3)
            self._dec_engine = GpuMaskedAggregator(cfg, cfg, 16, device=self.device)
        return self._dec_engine

    def decode_model(self, body, dtype: int):
        """The global model of an Option<Model> body as a tensor of
        mask::DataType code `dtype` on this accelerator's device: the values
        _core.sdk.decode_model gives, or None where it gives None. A body in
        the coordinator's own (canonical, dyadic) form is decoded by the K7d
        kernels; any other goes through the CPU decoder and is uploaded. The
        tensor is the caller's own."""
        from xaynet_amd import _core

        with self._mu:
            try:
                if memoryview(body).nbytes >= self.DECODE_MIN_BYTES:
                    t = self._decode_engine().decode_model(body, dtype)
                    if t is not None:
                        return t.clone()  # the engine's buffer is reused by the next call
            except Exception:  # noqa: BLE001 — CPU fallback
                LOG.exception("GPU decode_model failed; falling back to CPU")
            arr = _core.sdk.decode_model(body, dtype)
            if arr is None:
                return None
            return self.torch.from_numpy(arr).to(self.device)

    def attach(self, participant) -> None:
        participant.set_mask_model_hook(self.mask_model)
        participant.set_sum2_hook(self.aggregate_masks)


_SHARED = {}  # exact flag -> the process-wide ParticipantAccel
_SHARED_MU = threading.Lock()


def shared_accel(exact: bool = False) -> ParticipantAccel:
    """The process-wide accelerator of the SDK's gpu=True participants, one per
    flag value (its engines are cached per round config)."""
    exact = bool(exact)
    with _SHARED_MU:
        if exact not in _SHARED:
            _SHARED[exact] = ParticipantAccel(exact=exact)
        return _SHARED[exact]
