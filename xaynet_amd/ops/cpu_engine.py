"""CPU digit-plane aggregation engine (test/dev analog of the GPU engine).

Mirrors the `GpuMaskedAggregator` API with numpy so the multi-process serve
plane and the gloo world>1 tests can run the EXACT same composition code
(`xaynet_amd.parallel.ShardedAggregation`, worker loop, ingest ring) on boxes
without a GPU. Production deployments use the HIP engine; this class exists
so the distributed path is provable in CPU CI.

u64 orders use vectorised numpy u64 math. Wide orders (2^64 <= order <
2^320, bpn 9..40) use the GPU engine's layouts — canonical values as
[n_limbs, length] int64 rows of u64 limbs (lo/hi up to 2^128), compact digit
planes of `digit_bits`-wide digits — and Python-int/object math internally: a
test vehicle, not a hot path.

Semantics are pinned to the reference math (masking.rs:190-231, 292-316):
plane arithmetic is the same deferred-modular scheme as kernels.hip, and the
unmask formula matches the K4 kernels (including their float order of
operations) so CPU- and GPU-plane results agree on integer dtypes.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import torch

from xaynet_amd import _core

from .base import DEFAULT_SUM2_BUDGET_BYTES, MaskedAggregatorBase

_U64 = np.uint64
_M64 = (1 << 64) - 1


def _bmax_int_weight(d: int, exp: int, scalar_sum: float) -> float:
    """Integer-dtype weight from the signed offset-free value d, in the
    exact-offset K4's order of operations: exact quotient and remainder of
    |d| by E, double(q) + double(r)/double(E), sign, / scalar_sum."""
    q, r = divmod(abs(d), exp)
    y = float(q) + float(r) / float(exp)
    return (-y if d < 0 else y) / scalar_sum


class CpuPlaneAggregator(MaskedAggregatorBase):
    """Digit-plane aggregation of wire-format masked updates on the CPU."""

    _NP_DTYPES = {0: np.float32, 1: np.float64, 2: np.int32, 3: np.int64}
    _MODEL_DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64)

    def __init__(self, vect_cfg, unit_cfg, length: int, device: str = "cpu",
                 sum2_budget_bytes: int = DEFAULT_SUM2_BUDGET_BYTES):
        super().__init__(vect_cfg, unit_cfg, length, "cpu", sum2_budget_bytes)

    # ---------------- value tensors <-> python ints ----------------

    def _ints(self, vals: torch.Tensor) -> np.ndarray:
        """Canonical value tensor ([n], or wide [n_limbs, n] limb rows) ->
        object ints."""
        if self.wide:
            total = np.zeros(vals.shape[1], dtype=object)
            for j in reversed(range(vals.shape[0])):
                total = (total << 64) + vals[j].numpy().view(_U64).astype(object)
            return total
        return vals.numpy().view(_U64).astype(object)

    def _values(self, ints: np.ndarray) -> torch.Tensor:
        """Object ints -> canonical value tensor (inverse of _ints)."""
        if self.wide:
            rows = [np.array([(int(v) >> (64 * j)) & _M64 for v in ints], dtype=_U64)
                    for j in range(self.n_limbs)]
            return torch.from_numpy(np.stack(rows).astype(np.int64))
        return torch.from_numpy(np.array([int(v) for v in ints], dtype=_U64).astype(np.int64))

    @staticmethod
    def _ret(t: torch.Tensor, out: torch.Tensor | None) -> torch.Tensor:
        if out is None:
            return t
        out.copy_(t)
        return out

    # ---------------- limb <-> value ----------------

    def _limb_word(self, limbs: np.ndarray, first: int, last: int) -> np.ndarray:
        """Little-endian bytes [first, last) of [..., bpn] limbs -> u64."""
        word = np.zeros(limbs.shape[:-1], dtype=_U64)
        for b in range(first, min(last, self.bpn)):
            word |= limbs[..., b].astype(_U64) << _U64(8 * (b - first))
        return word

    def _rows_to_values(self, rows: np.ndarray) -> np.ndarray:
        """uint8 [n, >=length*bpn] -> u64 [n, length] little-endian limbs."""
        n = rows.shape[0]
        limbs = rows[:, : self.length * self.bpn].reshape(n, self.length, self.bpn)
        return self._limb_word(limbs, 0, 8)

    def _limbs_to_tensor(self, limbs: np.ndarray) -> torch.Tensor:
        """uint8 [length, bpn] -> canonical value tensor."""
        lo = self._limb_word(limbs, 0, 8)
        if self.wide:
            lo = np.stack([lo] + [self._limb_word(limbs, 8 * j, 8 * j + 8)
                                  for j in range(1, self.n_limbs)])
        return torch.from_numpy(lo.astype(np.int64))

    def unpack_wire(self, packed: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        limbs = packed.numpy()[: self.length * self.bpn].reshape(self.length, self.bpn)
        return self._ret(self._limbs_to_tensor(limbs), out)

    def pack_wire(self, values: torch.Tensor) -> torch.Tensor:
        words = values.numpy().view(_U64).reshape(-1, self.length)  # [n_limbs, length]
        out = np.zeros(self.length * self.bpn, dtype=np.uint8)
        limbs = out.reshape(self.length, self.bpn)
        for b in range(self.bpn):
            limbs[:, b] = ((words[b // 8] >> _U64(8 * (b % 8))) & _U64(0xFF)).astype(np.uint8)
        return torch.from_numpy(out)

    # ---------------- mask expansion ----------------

    def derive_mask_values(self, seed: bytes, out: torch.Tensor | None = None) -> torch.Tensor:
        pair = _core.mask.MaskConfigPair(self.vect_cfg, self.unit_cfg)
        obj = _core.mask.derive_mask(seed, self.length, pair)
        limbs = np.frombuffer(obj.vect_bytes, dtype=np.uint8).reshape(self.length, self.bpn)
        return self._ret(self._limbs_to_tensor(limbs), out)

    @property
    def batch_size(self) -> int:
        """There is no launch to share here: the rows of one sum pass, and 1
        for multi-limb orders as on the GPU."""
        return 1 if self.n_limbs > 2 else self.sum2_group

    def derive_mask_values_batch(self, seeds, out: torch.Tensor | None = None) -> torch.Tensor:
        seeds = [bytes(s) for s in seeds]
        out = self.new_rows(len(seeds)) if out is None else out
        if out.shape[0] != len(seeds):
            raise ValueError("derive_mask_values_batch: one row per seed")
        for s, seed in enumerate(seeds):
            self.derive_mask_values(seed, out=out[s])
        return out

    def add_rows_to_planes(self, rows: torch.Tensor, planes: torch.Tensor):
        for row in rows:
            self.values_to_planes(row, planes)

    # ---------------- aggregation ----------------

    def aggregate_pool(self, pool: torch.Tensor, n_updates: int, unit_sum: int = 0):
        self._check_headroom(n_updates)
        rows = pool[:n_updates].numpy()
        acc = self.acc.numpy().view(_U64)
        if self.wide:
            limbs = rows[:, : self.length * self.bpn].reshape(n_updates, self.length, self.bpn)
            for d in range(self.n_digits):
                acc[d] += self._limb_word(limbs, 4 * d, 4 * d + 4).sum(axis=0, dtype=_U64)
        else:
            vals = self._rows_to_values(rows)
            for d in range(self.n_digits):
                acc[d] += ((vals >> _U64(32 * d)) & _U64(0xFFFFFFFF)).sum(axis=0, dtype=_U64)
        self.nb_models += n_updates
        self.unit_acc = (self.unit_acc + unit_sum) % int(self.unit_cfg.order)

    # ---------------- finalize / unmask ----------------

    def _check_digits(self, digit_bits: int):
        if not 1 <= digit_bits <= 63:
            raise ValueError("digit_bits must be in 1..63")
        if not self.wide and digit_bits != 32:
            raise ValueError("u64-order digit planes are 32 bits wide")

    def _planes_to_ints(self, planes: torch.Tensor, digit_bits: int = 32) -> np.ndarray:
        """Recombine digit planes mod order (object math: digits may carry)."""
        self._check_digits(digit_bits)
        self._check_window(planes.shape[0], digit_bits)
        arr = planes.numpy().view(_U64)
        total = np.zeros(arr.shape[1], dtype=object)
        for d in reversed(range(planes.shape[0])):
            total = (total << digit_bits) + arr[d].astype(object)
        return total % self.order_int

    def _add_ints_to_planes(self, ints: np.ndarray, planes: torch.Tensor, digit_bits: int):
        self._check_digits(digit_bits)
        acc = planes.numpy().view(_U64)
        digit_mask = (1 << digit_bits) - 1
        for d in range(planes.shape[0]):
            acc[d] += np.array([(int(v) >> (digit_bits * d)) & digit_mask for v in ints],
                               dtype=_U64)

    def canonical(self, out: torch.Tensor | None = None) -> torch.Tensor:
        return self._ret(self._values(self._planes_to_ints(self.acc)), out)

    def mod_add_values(self, a: torch.Tensor, b: torch.Tensor):
        if self.wide:
            a.copy_(self._values((self._ints(a) + self._ints(b)) % self.order_int))
            return
        av = a.numpy().view(_U64)
        bv = b.numpy().view(_U64)
        order = _U64(self.order_int)
        s = av + bv  # safe: order < 2^63 on this path
        np.copyto(av, np.where(s >= order, s - order, s))

    def values_to_planes(self, vals: torch.Tensor, planes: torch.Tensor, digit_bits: int = 32):
        """Add canonical values into [k, n] planes of digit_bits-wide digits."""
        if self.wide:
            self._add_ints_to_planes(self._ints(vals), planes, digit_bits)
            return
        self._check_digits(digit_bits)
        v = vals.numpy().view(_U64)
        acc = planes.numpy().view(_U64)
        for d in range(planes.shape[0]):
            acc[d] += (v >> _U64(32 * d)) & _U64(0xFFFFFFFF)

    def planes_to_values(self, planes: torch.Tensor, out: torch.Tensor, digit_bits: int = 32):
        out.copy_(self._values(self._planes_to_ints(planes, digit_bits)))

    def recode_planes(self, out_planes: torch.Tensor, digit_bits: int) -> torch.Tensor:
        """Write the accumulator's value mod order into compact [k, length]
        planes of digit_bits-wide digits (wide orders)."""
        if not self.wide:
            raise NotImplementedError("compact digit planes cover wide (u128) orders; "
                                      "u64 orders reduce canonical values or 32-bit planes")
        out_planes.zero_()
        self._add_ints_to_planes(self._planes_to_ints(self.acc), out_planes, digit_bits)
        return out_planes

    def _finalize(self, masked: np.ndarray, mask_values: torch.Tensor, mask_unit: int, nb: int,
                  dtype: int | None, exact: bool = False) -> torch.Tensor:
        """masked: object-int array of canonical values."""
        scalar_sum, vinfo, dt = self._unmask_scalars(mask_unit, nb, dtype)
        q = self.exact_divisor(vinfo, dt) if exact else None
        order = self.order_int
        t = (masked + order - self._ints(mask_values)) % order
        exp = vinfo["exp_shift_u64"]
        n_add = nb * vinfo["add_shift"]
        # the exact-offset K4: d = t - nb*add*E as a signed integer
        d = [int(v) - vinfo["offset"] for v in t]
        if q is not None:
            # exact mode, float outputs: d / Q rounded once, by the element
            # function the kernel compiles (gpu/unmask_round.h)
            return torch.from_numpy(_core.mask.unmask_round(
                [abs(v) for v in d], [v < 0 for v in d], q, dt, limbs=self.n_limbs))
        if dt in (2, 3) and vinfo["divisor"] and (self.bmax or self.exact_integers(vinfo, dt)):
            # exact truncated quotient, never through doubles; the low 64
            # bits wrap into the output type as the kernel's casts do
            div = vinfo["divisor"]
            exact = [-(-v // div) if v < 0 else v // div for v in d]
            wrapped = np.array([q & _M64 for q in exact], dtype=_U64).astype(np.int64)
            return torch.from_numpy(wrapped.astype(self._NP_DTYPES[dt]))
        if self.bmax:
            # no exact divisor: the same double steps as the kernel
            if dt in (2, 3):
                outf = np.array([_bmax_int_weight(v, exp, scalar_sum) for v in d],
                                dtype=np.float64)
            else:
                scale = float(1 / (exp * Fraction(scalar_sum)))
                outf = np.array([math.copysign(float(abs(v)) * scale, v) for v in d],
                                dtype=np.float64)
        else:
            # the double steps of k4_unmask, k4_unmask_values and
            # k4_unmask_u128 alike: double(t / E) + double(t % E) / double(E),
            # minus nb*add_shift, over scalar_sum
            outf = np.array([(float(int(v) // exp) + float(int(v) % exp) / float(exp) - n_add)
                             / scalar_sum for v in t], dtype=np.float64)
        np_dt = self._NP_DTYPES[dt]
        if dt in (2, 3):
            outf = np.trunc(outf)
        return torch.from_numpy(outf.astype(np_dt))

    def unmask(self, mask_values: torch.Tensor, mask_unit: int,
               nb_models: int | None = None, dtype: int | None = None,
               exact: bool = False) -> torch.Tensor:
        nb = self.nb_models if nb_models is None else nb_models
        return self._finalize(self._planes_to_ints(self.acc), mask_values, mask_unit, nb, dtype,
                              exact)

    def unmask_f32(self, mask_values: torch.Tensor, mask_unit: int,
                   nb_models: int | None = None, exact: bool = False) -> torch.Tensor:
        return self.unmask(mask_values, mask_unit, nb_models=nb_models, dtype=0, exact=exact)

    def unmask_values(self, vals: torch.Tensor, mask_values: torch.Tensor, mask_unit: int,
                      nb_models: int, dtype: int | None = None,
                      exact: bool = False) -> torch.Tensor:
        if self.wide:
            raise NotImplementedError("values unmask covers u64 orders")
        masked = vals.numpy().view(_U64).astype(object) % self.order_int
        return self._finalize(masked, mask_values, mask_unit, nb_models, dtype, exact)

    def unmask_planes(self, planes: torch.Tensor, mask_values: torch.Tensor, mask_unit: int,
                      nb_models: int, dtype: int | None = None,
                      digit_bits: int = 32, exact: bool = False) -> torch.Tensor:
        return self._finalize(self._planes_to_ints(planes, digit_bits), mask_values, mask_unit,
                              nb_models, dtype, exact)

    # ---------------- wire format ----------------

    def wire_object(self, limbs: torch.Tensor, unit_value: int) -> bytes:
        """MaskObject wire bytes (MaskVect || MaskUnit) from packed limbs and
        the unit value."""
        ubpn = self.unit_cfg.bytes_per_number
        return (bytes(self.vect_cfg.to_bytes()) + (limbs.numel() // self.bpn).to_bytes(4, "big")
                + limbs.numpy().tobytes() + bytes(self.unit_cfg.to_bytes())
                + int(unit_value).to_bytes(ubpn, "little"))

    def encode_model(self, weights: torch.Tensor) -> np.ndarray:
        """The Option<Model> bincode body of unmasked weights (a contiguous
        1-D f32/f64/i32/i64 CPU tensor; ValueError otherwise) as a uint8
        array: the bytes the GPU engine's encode_model returns."""
        if not isinstance(weights, torch.Tensor) or weights.dim() != 1 \
                or not weights.is_contiguous() or weights.device.type != "cpu" \
                or weights.dtype not in self._MODEL_DTYPES:
            raise ValueError("encode_model takes a contiguous 1-D f32/f64/i32/i64 CPU tensor")
        return np.frombuffer(_core.sdk.encode_model(weights.numpy()), dtype=np.uint8)

    def decode_model(self, body, dtype: int, tile_blocks: int = 0):
        """The weights of an Option<Model> bincode body as a CPU tensor of
        mask::DataType code `dtype`, or None unless the body is exactly what
        encode_model writes for some weights of that dtype: the GPU engine's
        contract, through the same element functions on the host. `body` is
        any C-contiguous 1-D buffer (ValueError otherwise)."""
        if dtype not in (0, 1, 2, 3):
            raise ValueError("dtype must be 0..3")
        try:
            mv = memoryview(body)
        except TypeError as e:
            raise ValueError("decode_model takes a C-contiguous 1-D buffer") from e
        if mv.ndim != 1 or not mv.c_contiguous:
            raise ValueError("decode_model takes a C-contiguous 1-D buffer")
        arr = _core.sdk.model_codec_decode(mv, dtype)
        return None if arr is None else torch.from_numpy(arr)
