"""MI355X masked-aggregation engine (single GPU; multi-GPU composition in
xaynet_amd.parallel).

Data layout (see csrc/gpu/kernels.hip):
  - updates: wire-format packed limb rows, uint8 [n][stride] device tensor
  - accumulator: u64 digit planes, int64 [n_digits32][len] device tensor
    (plain integer sums; modular reduction deferred to finalize — this is
    what makes cross-GPU RCCL int64 all-reduce valid)
  - canonical values (masks, finalized sums): int64 [n] for orders < 2^64,
    [n_limbs, n] rows of u64 limbs for wide orders: lo/hi rows [2, n] up to
    2^128, 3..5 rows for the f32 and i64 Bmax orders (`new_values`)

Every method hands `_hip` the values as a (lo, hi) pointer pair and the order
as a decimal string; the extension picks the u64, the u128 or the multi-limb
kernel from the order. Lengths come from the tensors, so every value/plane
method also works on a shard.

Memory is owned by torch (device tensors); kernels launch on the null
stream, which serializes with torch's default stream.

Fails loudly if the _hip extension or a GPU is unavailable — there is no
silent CPU fallback on a GPU box. Orders below 2^320 are supported; only the
f64 Bmax orders (2112..2143 bits) are routed to the CPU oracle by the caller.
"""
import os
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from xaynet_amd import _core

from .base import DEFAULT_SUM2_BUDGET_BYTES, MaskedAggregatorBase, _cfg_scalars

try:
    from xaynet_amd import _hip
except ImportError as e:  # pragma: no cover
    _hip = None
    _hip_err = e


def gpu_available() -> bool:
    return _hip is not None and _hip.device_count() > 0


def _require_gpu():
    if _hip is None:
        raise RuntimeError(f"xaynet_amd._hip extension not built: {_hip_err}")
    if _hip.device_count() == 0:
        raise RuntimeError("no AMD GPU visible (xaynet_amd._hip loaded, hipGetDeviceCount=0)")


class GpuMaskedAggregator(MaskedAggregatorBase):
    """Digit-plane aggregation of wire-format masked updates on one GPU."""

    _WEIGHT_DTYPES = {torch.float32: 0, torch.float64: 1, torch.int32: 2, torch.int64: 3}

    def __init__(self, vect_cfg, unit_cfg, length: int, device: str = "cuda",
                 sum2_budget_bytes: int = DEFAULT_SUM2_BUDGET_BYTES):
        _require_gpu()
        super().__init__(vect_cfg, unit_cfg, length, device, sum2_budget_bytes)
        with torch.cuda.device(self.device):
            self._expander = _hip.MaskExpander()
        self._wire_pin = None  # cached pinned staging buffer of wire_object
        # encode_model: cached workspace, device body and pinned staging buffer
        self._enc_work = self._enc_dev = self._enc_pin = None
        # decode_model: cached workspace, device body, output and pinned staging buffer
        self._dec_work = self._dec_dev = self._dec_out = self._dec_pin = None

    # ---------------- tensor forms ----------------

    def _vals(self, t: torch.Tensor):
        """Canonical value tensor -> (lo_ptr, hi_ptr, n), the form every
        `_hip` call takes: int64 [n] (hi_ptr 0) for u64 orders, [n_limbs, n]
        limb rows for wide ones (lo/hi up to 2^128). lo and hi point at rows 0
        and 1; the extension finds row j at lo + j*(hi - lo) and takes the row
        count from the order. Rows must be dense; a column slice t[:, a:b] of
        an [n_limbs, n] tensor is."""
        if t.dtype != torch.int64 or t.dim() != 1 + self.wide or t.stride(-1) != 1 \
                or (self.wide and t.shape[0] != self.n_limbs):
            raise ValueError("canonical values must be " + (
                f"[{self.n_limbs}, n] int64 limb rows" if self.wide else "an [n] int64 tensor")
                + " with unit element stride")
        if self.wide:
            return t[0].data_ptr(), t[1].data_ptr(), t.shape[1]
        return t.data_ptr(), 0, t.shape[0]

    def _planes(self, planes: torch.Tensor, n: int, read_bits: int | None = None):
        """Digit-plane tensor -> (ptr, k): contiguous int64 [k, n] planes for
        values of n elements; u64 orders have exactly n_digits planes. Planes
        that a kernel reads back into one integer pass their digit width as
        read_bits: their shape must lie inside the reduction window
        (plane_window_ok)."""
        if planes.dtype != torch.int64 or planes.dim() != 2 or not planes.is_contiguous() \
                or planes.shape[1] != n:
            raise ValueError(f"planes must be a contiguous [k, {n}] int64 tensor")
        if not self.wide and planes.shape[0] != self.n_digits:
            raise ValueError(f"u64-order planes are [{self.n_digits}, n]")
        if read_bits is not None and 1 <= read_bits <= 63:  # other widths: _hip refuses
            self._check_window(planes.shape[0], read_bits)
        return planes.data_ptr(), planes.shape[0]

    # ---------------- mask expansion (K1) ----------------

    def derive_mask_values(self, seed: bytes, out: torch.Tensor | None = None) -> torch.Tensor:
        """Expand seed -> canonical mask values (vect part only; unit handled
        on CPU). Bit-exact with _core.mask.derive_mask."""
        out = self.new_values() if out is None else out
        lo, hi, n = self._vals(out)
        _, unit_words = _core.mask.unit_draw(seed, self.unit_cfg)
        self._expander.expand(seed, lo, hi, n, self.order, self.prng_nbytes, unit_words)
        return out

    @property
    def batch_size(self) -> int:
        """Seeds derive_mask_values_batch expands per launch: as many as keep
        their value rows and candidate planes within sum2_budget_bytes; 1 for
        multi-limb orders and where one seed's launch is past the
        single-workgroup scan (the rule is MaskExpander's)."""
        return _hip.MaskExpander._batch_size(self.length, self.order, self.prng_nbytes,
                                             self.sum2_budget_bytes)

    def _rows(self, rows: torch.Tensor):
        """[S, n] / [S, n_limbs, n] value rows -> (lo_ptr, hi_ptr, n, S,
        row stride in elements)."""
        if rows.dim() != 2 + self.wide or not rows.is_contiguous() or rows.shape[0] < 1:
            raise ValueError("value rows must be a contiguous [S, "
                             + (f"{self.n_limbs}, " if self.wide else "") + "n] int64 tensor")
        lo, hi, n = self._vals(rows[0])
        return lo, hi, n, rows.shape[0], rows.stride(0)

    def derive_mask_values_batch(self, seeds, out: torch.Tensor | None = None) -> torch.Tensor:
        """Expand every seed: row s of the result is derive_mask_values(seeds[s]),
        bit for bit. batch_size seeds share one candidates -> scan -> scatter
        pass, one copy of keys in and one of accepted counts out."""
        seeds = [bytes(s) for s in seeds]
        out = self.new_rows(len(seeds)) if out is None else out
        lo, hi, n, rows, stride = self._rows(out)
        if rows != len(seeds):
            raise ValueError("derive_mask_values_batch: one row per seed")
        words = [_core.mask.unit_draw(s, self.unit_cfg)[1] for s in seeds]
        step = self.batch_size
        for i in range(0, rows, step):
            off = 8 * i * stride
            self._expander.expand(b"".join(seeds[i:i + step]), lo + off, hi + off if hi else 0,
                                  n, self.order, self.prng_nbytes, words[i:i + step],
                                  seed_stride=stride)
        return out

    def add_rows_to_planes(self, rows: torch.Tensor, planes: torch.Tensor):
        """Add every row of an [S, n] / [S, n_limbs, n] value tensor into a
        contiguous [k, n] tensor of 32-bit digit planes: the rows' digits are
        summed in registers and the planes touched once."""
        lo, hi, n, s, stride = self._rows(rows)
        ptr, k = self._planes(planes, n)
        _hip.add_to_planes(ptr, lo, hi, n, k, self.order, 32, rows=s, row_stride=stride)

    # ---------------- aggregation (K3) ----------------

    def aggregate_pool(self, pool: torch.Tensor, n_updates: int, unit_sum: int = 0):
        """Accumulate n_updates packed rows into the digit planes."""
        self._check_headroom(n_updates)
        _hip.aggregate_batch(
            self.acc.data_ptr(), pool.data_ptr(), pool.stride(0), n_updates, self.length,
            self.bpn, int(os.environ.get("XAYNET_K3_EPT", "0"))
        )
        self.nb_models += n_updates
        self.unit_acc = (self.unit_acc + unit_sum) % int(self.unit_cfg.order)

    # ---------------- finalize / unmask (K2, K4) ----------------

    def canonical(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """Accumulator digit planes -> canonical values mod order."""
        out = self.new_values() if out is None else out
        self.planes_to_values(self.acc, out)
        return out

    def mod_add_values(self, a: torch.Tensor, b: torch.Tensor):
        """a = (a + b) mod order, canonical tensors of equal length."""
        a_lo, a_hi, n = self._vals(a)
        b_lo, b_hi, nb = self._vals(b)
        if n != nb:
            raise ValueError("mod_add_values: lengths differ")
        _hip.mod_add(a_lo, a_hi, b_lo, b_hi, n, self.order)

    def values_to_planes(self, vals: torch.Tensor, planes: torch.Tensor, digit_bits: int = 32):
        """Add canonical values into a contiguous [k, n] plane tensor of
        digit_bits-wide digits (u64 orders: n_digits planes of 32 bits)."""
        lo, hi, n = self._vals(vals)
        ptr, k = self._planes(planes, n)
        _hip.add_to_planes(ptr, lo, hi, n, k, self.order, digit_bits)

    def planes_to_values(self, planes: torch.Tensor, out: torch.Tensor, digit_bits: int = 32):
        """Canonicalize a contiguous [k, n] plane tensor mod order (the
        inverse layout of values_to_planes)."""
        lo, hi, n = self._vals(out)
        ptr, k = self._planes(planes, n, read_bits=digit_bits)
        _hip.canonicalize(ptr, lo, hi, n, k, self.order, digit_bits)

    def recode_planes(self, out_planes: torch.Tensor, digit_bits: int) -> torch.Tensor:
        """Write (not add) the accumulator's value mod order into the compact
        [k, length] planes of digit_bits-wide digits — the wide-order input of
        the cross-rank reduce-scatter (xaynet_amd.parallel.compact_digits)."""
        if not self.wide:
            raise NotImplementedError("compact digit planes cover wide (u128) orders; "
                                      "u64 orders reduce canonical values or 32-bit planes")
        ptr, k = self._planes(out_planes, self.length)
        _hip.recode_planes(self.acc.data_ptr(), ptr, self.length, self.n_digits, self.order,
                           k, digit_bits)
        return out_planes

    def unmask(self, mask_values: torch.Tensor, mask_unit: int,
               nb_models: int | None = None, dtype: int | None = None,
               exact: bool = False) -> torch.Tensor:
        """Unmask the aggregate into model weights (reference unmask math,
        masking.rs:190-231). dtype follows mask::DataType (default: the vect
        config's data type); integers truncate toward zero. Float outputs
        carry the double roundings of K4 (tests/unmask_edges.float_bound);
        exact=True returns the exact rational weight rounded once to the
        output type instead (k4_unmask_exact), for every order the engine
        covers - ValueError where exp_shift * scalar_sum is no positive
        integer that fits the order's limbs, or where an integer dtype would
        only get the double steps (`exact_divisor`)."""
        nb = self.nb_models if nb_models is None else nb_models
        return self.unmask_planes(self.acc, mask_values, mask_unit, nb, dtype, exact=exact)

    def unmask_f32(self, mask_values: torch.Tensor, mask_unit: int,
                   nb_models: int | None = None, exact: bool = False) -> torch.Tensor:
        return self.unmask(mask_values, mask_unit, nb_models=nb_models, dtype=0, exact=exact)

    def unmask_values(self, vals: torch.Tensor, mask_values: torch.Tensor, mask_unit: int,
                      nb_models: int, dtype: int | None = None,
                      exact: bool = False) -> torch.Tensor:
        """Unmask a u64 tensor of (possibly cross-rank summed) canonical
        values — the reduce-scatter path. Valid while nb_ranks*order < 2^64.
        exact as for unmask."""
        if self.wide:
            raise NotImplementedError("values unmask covers u64 orders")
        v_ptr, _, n = self._vals(vals)
        lo, hi, nm = self._vals(mask_values)
        if n != nm:
            raise ValueError("unmask_values: lengths differ")
        scalar_sum, vinfo, dt = self._unmask_scalars(mask_unit, nb_models, dtype)
        q = self.exact_divisor(vinfo, dt) if exact else None
        out = torch.empty(n, dtype=self._TORCH_DTYPES[dt], device=vals.device)
        if q is not None:  # a float output in exact mode
            _hip.unmask_values(v_ptr, lo, hi, out.data_ptr(), n, self.order,
                               str(vinfo["exp_shift_u64"]), 0.0, scalar_sum, dt,
                               offset=str(vinfo["offset"]), divisor=str(q))
            return out
        offset = self.exact_integers(vinfo, dt)
        _hip.unmask_values(v_ptr, lo, hi, out.data_ptr(), n, self.order,
                           str(vinfo["exp_shift_u64"]), nb_models * vinfo["add_shift"],
                           scalar_sum, dt, offset=str(vinfo["offset"]) if offset else "",
                           divisor=str(vinfo["divisor"]) if offset else "")
        return out

    def unmask_planes(self, planes: torch.Tensor, mask_values: torch.Tensor, mask_unit: int,
                      nb_models: int, dtype: int | None = None,
                      digit_bits: int = 32, exact: bool = False) -> torch.Tensor:
        """Unmask a contiguous [k, n] digit-plane tensor (e.g. this rank's
        reduce-scattered shard) against matching mask values, which may be a
        slice mask[lo:lo+n] / mask[:, lo:lo+n]. Wide orders take planes of
        digit_bits-wide digits. exact as for unmask."""
        lo, hi, n = self._vals(mask_values)
        ptr, k = self._planes(planes, n, read_bits=digit_bits)
        scalar_sum, vinfo, dt = self._unmask_scalars(mask_unit, nb_models, dtype)
        q = self.exact_divisor(vinfo, dt) if exact else None
        out = torch.empty(n, dtype=self._TORCH_DTYPES[dt], device=planes.device)
        if q is not None:
            # a float output in exact mode: offset and divisor as integers,
            # the quotient rounded once in the kernel
            _hip.unmask(ptr, lo, hi, out.data_ptr(), n, k, self.order,
                        str(vinfo["exp_shift_u64"]), 0.0, scalar_sum, dt, digit_bits,
                        offset=str(vinfo["offset"]), divisor=str(q))
            return out
        if self.bmax or self.exact_integers(vinfo, dt):
            # nb*add_shift is subtracted as the exact integer offset, not as
            # a double: Bmax weights would vanish against it, and integer
            # outputs of the other bounds are the exact truncated quotient
            # (the divisor is theirs: given one, a float output runs exact mode)
            divisor = str(vinfo["divisor"] or "") if dt in (2, 3) else ""
            _hip.unmask(ptr, lo, hi, out.data_ptr(), n, k, self.order,
                        str(vinfo["exp_shift_u64"]), 0.0, scalar_sum, dt, digit_bits,
                        offset=str(vinfo["offset"]), divisor=divisor)
            return out
        _hip.unmask(ptr, lo, hi, out.data_ptr(), n, k, self.order, str(vinfo["exp_shift_u64"]),
                    nb_models * vinfo["add_shift"], scalar_sum, dt, digit_bits)
        return out

    # ---------------- synthetic updates (K5, bench/test-drive) ----------------

    def synth_update(self, pool: torch.Tensor, row: int, mask_values: torch.Tensor,
                     participant: int, scalar: float):
        if self.bmax:
            raise NotImplementedError(
                "synthetic update rows (K5, benchmark only) do not cover Bmax configs; "
                "mask real weights with mask_weights or the CPU masker")
        lo, hi, n = self._vals(mask_values)
        if n * self.bpn > pool.shape[1]:
            raise ValueError("synth_update: mask values longer than a pool row")
        vinfo = _cfg_scalars(self.vect_cfg)
        _hip.mask_pack(lo, hi, pool[row].data_ptr(), n, self.bpn, self.order, participant,
                       scalar, vinfo["add_shift"], str(vinfo["exp_shift_u64"]))

    def mask_weights(self, seed: bytes, weights: torch.Tensor,
                     scalar_num: int = 1, scalar_den: int = 1, exact: bool = False) -> bytes:
        """Mask a REAL weight tensor (the participant's update task): K1
        expand + K5w quantize+mask+pack; returns the full MaskObject wire
        bytes (MaskVect || MaskUnit). Replaces the CPU fast masker's hot
        loop (reference Masker::mask, masking.rs:358-404) for GPU clients.
        Quantization deviates from the exact-rational path by at most a few
        1/exp_shift quanta (double rounding before an exact mulshift).
        exact=True quantises in integers instead, for every config the engine
        covers: the bytes are the rational masker's (mask_model_oracle). The
        scalar, clamped to the unit config's bound and reduced, must then have
        numerator and denominator below 2^63 (ValueError otherwise)."""
        if weights.numel() != self.length:
            raise ValueError("weights length != model length")
        dt = self._WEIGHT_DTYPES[weights.dtype]
        if exact:
            p, q = self.clamped_scalar(scalar_num, scalar_den)
            if p >= 2**63 or q >= 2**63:
                raise ValueError("exact masking takes a scalar whose reduced numerator and "
                                 "denominator are below 2^63")
        w_dev = weights.to(self.device).contiguous()
        mask_vals = self.derive_mask_values(seed)  # named: must outlive the kernel launch
        lo, hi, n = self._vals(mask_vals)
        vinfo = _cfg_scalars(self.vect_cfg)
        out = torch.empty(n * self.bpn, dtype=torch.uint8, device=self.device)
        if exact:
            _hip.mask_weights(w_dev.data_ptr(), dt, lo, hi, out.data_ptr(), n, self.bpn,
                              self.order, p / q, float(vinfo["add_shift"]),
                              str(vinfo["exp_shift_u64"]), scalar_num=p, scalar_den=q)
            # masked_unit_for assumes scalar <= add_shift: hand it the clamped one
            return self.wire_object(out, self.masked_unit_for(seed, p, q))
        # Bmax: add_shift (a dtype extreme, exact as a double) clamps; the
        # shift itself is added as the integer add_shift * exp_shift
        offset = str(vinfo["add_shift"] * vinfo["exp_shift_u64"]) if self.bmax else ""
        _hip.mask_weights(w_dev.data_ptr(), dt, lo, hi, out.data_ptr(), n, self.bpn, self.order,
                          scalar_num / scalar_den, float(vinfo["add_shift"]),
                          str(vinfo["exp_shift_u64"]), offset=offset)
        # masked unit (scalar clamp + quantize + unit mask), exact on CPU
        return self.wire_object(out, self.masked_unit_for(seed, scalar_num, scalar_den))

    # ---------------- wire format (K6) ----------------

    def unpack_wire(self, packed: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        out = self.new_values() if out is None else out
        lo, hi, n = self._vals(out)
        if packed.numel() < n * self.bpn:
            raise ValueError("unpack_wire: packed limbs shorter than the values")
        _hip.unpack(packed.data_ptr(), lo, hi, n, self.bpn, self.order)
        return out

    def pack_wire(self, values: torch.Tensor) -> torch.Tensor:
        lo, hi, n = self._vals(values)
        out = torch.empty(n * self.bpn, dtype=torch.uint8, device=self.device)
        _hip.pack(lo, hi, out.data_ptr(), n, self.bpn, self.order)
        return out

    def wire_object(self, limbs_dev: torch.Tensor, unit_value: int) -> bytes:
        """MaskObject wire bytes (MaskVect || MaskUnit) from packed device
        limbs and the unit value. Assembled in ONE host buffer: a single D2H
        lands the limbs directly in place (a 25M-param update is ~175 MB;
        intermediate bytes/bytearray copies dominate otherwise)."""
        nlimb = limbs_dev.numel()
        ubpn = self.unit_cfg.bytes_per_number
        wire = bytearray(8 + nlimb + 4 + ubpn)
        wire[0:4] = bytes(self.vect_cfg.to_bytes())
        wire[4:8] = (nlimb // self.bpn).to_bytes(4, "big")
        # stage through a cached PINNED buffer: a direct D2H into pageable
        # memory runs at ~2 GB/s in chunked staging copies (rocprof:
        # __amd_rocclr_copyBuffer dominated the wall time), pinned runs at
        # PCIe line rate and the host-side memcpy at memory speed
        if self._wire_pin is None or self._wire_pin.numel() < nlimb:
            self._wire_pin = torch.empty(nlimb, dtype=torch.uint8, pin_memory=True)
        pin = self._wire_pin[:nlimb]
        pin.copy_(limbs_dev)
        np.frombuffer(wire, dtype=np.uint8, count=nlimb, offset=8)[:] = pin.numpy()
        off = 8 + nlimb
        wire[off : off + 4] = bytes(self.unit_cfg.to_bytes())
        wire[off + 4 :] = int(unit_value).to_bytes(ubpn, "little")
        return bytes(wire)

    # ---------------- model body (K7) ----------------

    # a first guess at the body's bytes per weight (zero 28, a typical f32 32,
    # a typical f64 36..40); a longer body grows the buffers and runs again
    _ENC_GUESS = {0: 36, 1: 48, 2: 36, 3: 40}

    def encode_model(self, weights: torch.Tensor) -> np.ndarray:
        """The Option<Model> bincode body of unmasked weights, encoded on the
        GPU (K7): byte for byte what _core.sdk.encode_model gives for the same
        values. `weights` is a contiguous 1-D f32/f64/i32/i64 tensor on this
        engine's device, of any length (ValueError otherwise, before any
        launch). Returns a uint8 numpy view of a cached pinned staging buffer,
        valid until the next call on this engine."""
        dt = self._WEIGHT_DTYPES.get(weights.dtype) if isinstance(weights, torch.Tensor) else None
        if dt is None or weights.dim() != 1 or not weights.is_contiguous() \
                or weights.device != self.acc.device:
            raise ValueError("encode_model takes a contiguous 1-D f32/f64/i32/i64 tensor on "
                             f"{self.acc.device}")
        n = weights.numel()
        if n == 0:
            return np.frombuffer(b"\x01" + bytes(8), dtype=np.uint8)
        with torch.cuda.device(self.acc.device):
            work = self._enc_buffer("_enc_work", _hip._model_plan(n)["work_bytes"])
            out = self._enc_buffer("_enc_dev", 3 + 9 + n * self._ENC_GUESS[dt])
            body = _hip._model_encode(weights.data_ptr(), dt, n, work.data_ptr(),
                                      out.data_ptr(), out.numel())
            if 3 + body > out.numel():  # nothing was written: grow, run again
                out = self._enc_buffer("_enc_dev", 3 + body)
                body = _hip._model_encode(weights.data_ptr(), dt, n, work.data_ptr(),
                                          out.data_ptr(), out.numel())
            if self._enc_pin is None or self._enc_pin.numel() < 3 + body:
                self._enc_pin = torch.empty(3 + body + (3 + body) // 8, dtype=torch.uint8,
                                            pin_memory=True)
            pin = self._enc_pin[: 3 + body]
            pin.copy_(out[: 3 + body])  # device to pinned host: synchronous
        return pin.numpy()[3:]

    # ---------------- model body -> weights (K7d) ----------------

    _MODEL_DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64)
    # how decode_model gets a host body across: "pinned" (host copies into two
    # cached pinned chunks, overlapped with their DMAs), "pageable" (the runtime's staged
    # copy) or "register" (_hip.host_register on the caller's buffer for the
    # copy). scripts/model_decode_bench.py times all three; the fastest stays.
    _DEC_STAGING = "pinned"

    def decode_model(self, body, dtype: int, tile_blocks: int = 0):
        """The weights of an Option<Model> bincode body, decoded on the GPU
        (K7d), as a device tensor of mask::DataType code `dtype` (0=f32 1=f64
        2=i32 3=i64): bit for bit what _core.sdk.decode_model gives for a body
        that encode_model wrote. `body` is any C-contiguous 1-D buffer
        (ValueError otherwise, before any launch). Returns None for every
        other body: a wrong head or count, trailing bytes, an element that is
        not the canonical form of a value of the dtype, more than 2^32
        elements, or a body no device buffer takes. The tensor is a view of a
        cached buffer, valid until the next call on this engine. tile_blocks
        is a test hook (_hip._model_decode_plan)."""
        if dtype not in (0, 1, 2, 3):
            raise ValueError("dtype must be 0..3")
        try:
            mv = memoryview(body)
        except TypeError as e:
            raise ValueError("decode_model takes a C-contiguous 1-D buffer") from e
        if mv.ndim != 1 or not mv.c_contiguous:
            raise ValueError("decode_model takes a C-contiguous 1-D buffer")
        src = np.frombuffer(mv, dtype=np.uint8)
        nbytes = src.size
        if nbytes < 9 or src[0] != 1 or (nbytes - 9) % 4:
            return None
        n = int.from_bytes(src[1:9].tobytes(), "little")
        words = (nbytes - 9) // 4
        if n > 2**32 or not 7 * n <= words <= 42 * n:
            return None
        tdt = self._MODEL_DTYPES[dtype]
        if n == 0:
            return torch.empty(0, dtype=tdt, device=self.acc.device)
        with torch.cuda.device(self.acc.device):
            try:
                plan = _hip._model_decode_plan(words, tile_blocks)
                work = self._enc_buffer("_dec_work", plan["work_bytes"])
                dev = self._enc_buffer("_dec_dev", 3 + nbytes)
                out = self._enc_buffer("_dec_out", n * 8)
            except torch.OutOfMemoryError:
                return None
            self._upload_body(src, dev)
            rejected = _hip._model_decode(dev.data_ptr() + 3, nbytes, dtype, n, work.data_ptr(),
                                          out.data_ptr(), tile_blocks)
        if rejected:
            return None
        return out[: n * tdt.itemsize].view(tdt)

    def _upload_body(self, src: np.ndarray, dev: torch.Tensor, how: str | None = None):
        """Host bytes -> dev[3:3 + len]: at byte 3 the body's words are aligned."""
        how = how or self._DEC_STAGING
        nbytes = src.size
        if how == "pinned":
            self._upload_pinned(src, dev)
            return
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)  # a bytes body is read-only: only read
            host = torch.from_numpy(src)
        if how == "pageable":
            dev[3 : 3 + nbytes].copy_(host)
        elif how == "register":
            _hip.host_register(src.ctypes.data, nbytes)
            try:
                dev[3 : 3 + nbytes].copy_(host)
            finally:
                _hip.host_unregister(src.ctypes.data)
        else:
            raise ValueError(f"unknown staging {how!r}")

    # _upload_pinned: chunk size, and the host threads that fill one chunk
    _DEC_CHUNK = 32 << 20
    _DEC_COPY_THREADS = 4

    def _upload_pinned(self, src: np.ndarray, dev: torch.Tensor):
        """src -> dev[3:] through two cached pinned chunks: the host copy of
        one chunk (a few threads; numpy copies without the GIL) runs while the
        DMA of the chunk before it is in flight. Chunks are cut from the
        device buffer's offsets, so both sides of every DMA are aligned alike."""
        ch, end = self._DEC_CHUNK, 3 + src.size
        if self._dec_pin is None:
            self._dec_pin = (torch.empty((2, ch), dtype=torch.uint8, pin_memory=True),
                             [torch.cuda.Event(), torch.cuda.Event()],
                             ThreadPoolExecutor(self._DEC_COPY_THREADS))
        pin, events, pool = self._dec_pin
        for i, off in enumerate(range(0, end, ch)):
            lo, hi = max(off, 3), min(off + ch, end)
            slot, host = pin[i % 2], pin[i % 2].numpy()
            events[i % 2].synchronize()  # the DMA that last read this chunk is done
            if hi - lo < 1 << 20:  # not worth a hand-over to the threads
                np.copyto(host[lo - off : hi - off], src[lo - 3 : hi - 3])
            else:
                step = -(-(hi - lo) // self._DEC_COPY_THREADS)
                parts = [(a, min(a + step, hi)) for a in range(lo, hi, step)]
                list(pool.map(lambda ab: np.copyto(host[ab[0] - off : ab[1] - off],
                                                   src[ab[0] - 3 : ab[1] - 3]), parts))
            dev[lo:hi].copy_(slot[lo - off : hi - off], non_blocking=True)
            events[i % 2].record()
        events[0].synchronize()
        events[1].synchronize()

    def _enc_buffer(self, name: str, nbytes: int) -> torch.Tensor:
        """A cached device byte buffer of at least nbytes (contents not kept)."""
        buf = getattr(self, name)
        if buf is None or buf.numel() < nbytes:
            setattr(self, name, None)  # free before growing
            buf = torch.empty(nbytes + nbytes // 8, dtype=torch.uint8, device=self.device)
            setattr(self, name, buf)
        return buf
