"""What the GPU engine and its CPU analog share: the config-derived fields,
the update-pool layout, the exact CPU-side unit (scalar) arithmetic and the
shape of canonical value tensors."""
from fractions import Fraction

import torch

from xaynet_amd import _core


MAX_BYTES_PER_NUMBER = 40  # group orders below 2^320: up to five u64 limbs

# Updates one accumulator takes before its modular reduction: a plane entry is
# a sum of 32-bit digits, and 2^31 * (2^32 - 1) still fits the int64 planes
# (and the int64 collectives that sum them). Below the 10^12 models of the M12
# cap, so aggregate_pool enforces it.
MAX_UPDATES_PER_ACCUMULATOR = 2**31

# Bmax shifts per mask::DataType (csrc/mask/config.cpp, compute_exp_exponent
# and compute_add_shift): the clamp bound is the data type's own extreme.
_BMAX_SHIFTS = {
    0: (10**45, (2**24 - 1) << 104),  # F32: f32::MAX
    2: (10**10, 2**31),               # I32: -i32::MIN
    3: (10**10, 2**63),               # I64: -i64::MIN
}


def _cfg_scalars(cfg):
    """exp/add shifts as python scalars: floats (and the integer exp_shift)
    for the B0..B6 bounds, exact ints for Bmax, whose add_shift * exp_shift
    no double holds."""
    if cfg.bound == 255:
        if cfg.dtype not in _BMAX_SHIFTS:
            raise ValueError("F64 Bmax configs (2112..2143-bit orders) are not on the GPU "
                             "path; use the CPU oracle for this config")
        exp, add = _BMAX_SHIFTS[cfg.dtype]
        return {"exp_shift": exp, "exp_shift_u64": exp, "add_shift": add}
    exp_exp = {0: 10, 1: 20, 2: 10, 3: 10}[cfg.dtype]
    add = {0: 1.0, 2: 100.0, 4: 10_000.0, 6: 1_000_000.0}[cfg.bound]
    return {
        "exp_shift": float(10**exp_exp),
        "exp_shift_u64": 10**exp_exp,
        "add_shift": add,
    }


# Workspace budget of the batched sum2 path (value rows + candidate planes of
# one batch), from the sweep in profiles/r07_sum2_batch.md.
DEFAULT_SUM2_BUDGET_BYTES = 1 << 30
MAX_SUM2_ROWS = 65535  # rows one row-sum launch takes


class MaskedAggregatorBase:
    """Digit-plane aggregation state of one model: int64 [n_digits, length]
    accumulator planes plus the exact masked scalar sum."""

    _TORCH_DTYPES = {0: torch.float32, 1: torch.float64, 2: torch.int32, 3: torch.int64}

    def __init__(self, vect_cfg, unit_cfg, length: int, device,
                 sum2_budget_bytes: int = DEFAULT_SUM2_BUDGET_BYTES):
        if vect_cfg.bytes_per_number > MAX_BYTES_PER_NUMBER:
            raise ValueError(
                f"{type(self).__name__} covers group orders up to 2^320 (got "
                f"{vect_cfg.bytes_per_number} bytes/element); use the CPU oracle for this config"
            )
        self.vect_cfg = vect_cfg
        self.unit_cfg = unit_cfg
        self.length = length
        self.device = torch.device(device)
        self.bpn = vect_cfg.bytes_per_number
        # wide (order >= 2^64) configs: canonical values are rows of u64
        # limbs, [n_limbs, n] (lo/hi for orders up to 2^128); u64 orders: [n]
        self.wide = not vect_cfg.order_fits_u64
        self.n_limbs = (int(vect_cfg.order).bit_length() + 63) // 64
        self.bmax = vect_cfg.bound == 255
        self.n_digits = (self.bpn + 3) // 4
        self.order = vect_cfg.order  # decimal string
        self.order_int = int(vect_cfg.order)
        self.prng_nbytes = vect_cfg.prng_nbytes
        self.acc = torch.zeros(self.n_digits, length, dtype=torch.int64, device=self.device)
        self.nb_models = 0
        self.unit_acc = 0  # masked scalar sum (CPU, exact)
        # sum2 task (ops/sum2.py): planes and value rows of its own, made on
        # first use; self.acc belongs to update aggregation
        self.sum2_budget_bytes = int(sum2_budget_bytes)
        self._sum2_planes = None
        self._sum2_rows = None

    def reset(self):
        self.acc.zero_()
        self.nb_models = 0
        self.unit_acc = 0

    def _check_headroom(self, n_updates: int):
        """Before aggregate_pool touches the planes: the accumulator holds at
        most MAX_UPDATES_PER_ACCUMULATOR updates."""
        if n_updates < 0:
            raise ValueError("n_updates is negative")
        if self.nb_models + n_updates > MAX_UPDATES_PER_ACCUMULATOR:
            raise OverflowError(
                f"{self.nb_models} + {n_updates} updates exceed the 2^31 an accumulator's "
                "digit planes hold; reduce (canonical / unmask) and reset first")

    def plane_window_ok(self, k: int, digit_bits: int) -> bool:
        """Whether [k, n] planes of digit_bits-wide digit sums can be read back
        into one integer: with entries up to 2^64 the total is below
        2^((k-1)*digit_bits + 64), and the reduction mod order runs in a
        window of n_limbs + 1 words whose top bit stays clear."""
        return (k - 1) * digit_bits + 64 <= 64 * (self.n_limbs + 1) - 1

    def _check_window(self, k: int, digit_bits: int):
        if k < 1 or not self.plane_window_ok(k, digit_bits):
            raise ValueError(
                f"[{k}, n] planes of {digit_bits}-bit digits can spell 2^"
                f"{(k - 1) * digit_bits + 64}, outside the {64 * (self.n_limbs + 1) - 1}-bit "
                "window their reduction mod order takes")

    def new_values(self, n: int | None = None, zero: bool = False) -> torch.Tensor:
        """A canonical value tensor for n (default: length) elements: int64
        [n], or [n_limbs, n] limb rows (lo/hi for orders up to 2^128) when the
        order is wide."""
        n = self.length if n is None else n
        shape = (self.n_limbs, n) if self.wide else (n,)
        make = torch.zeros if zero else torch.empty
        return make(*shape, dtype=torch.int64, device=self.device)

    def new_rows(self, s: int) -> torch.Tensor:
        """s canonical value tensors in one: int64 [s, n], or [s, n_limbs, n]
        when the order is wide (what derive_mask_values_batch fills)."""
        shape = (s, self.n_limbs, self.length) if self.wide else (s, self.length)
        return torch.empty(*shape, dtype=torch.int64, device=self.device)

    # ---------------- sum2 workspace ----------------

    @property
    def sum2_group(self) -> int:
        """Masks summed by one add_rows_to_planes pass of the sum2 task: the
        value rows get half the workspace budget (the other half is for the
        candidate planes of a batch, which are at least as large)."""
        row_bytes = 8 * self.n_limbs * max(self.length, 1)
        return max(1, min(MAX_SUM2_ROWS, self.sum2_budget_bytes // (2 * row_bytes)))

    def sum2_workspace(self, n_seeds: int):
        """(zeroed planes, value rows) of the sum2 task: [n_digits, length]
        and min(n_seeds, sum2_group) rows, kept between calls."""
        if self._sum2_planes is None:
            self._sum2_planes = torch.empty_like(self.acc)
        rows = min(n_seeds, self.sum2_group)
        if self._sum2_rows is None or self._sum2_rows.shape[0] < rows:
            self._sum2_rows = None  # free before growing
            self._sum2_rows = self.new_rows(rows)
        self._sum2_planes.zero_()
        return self._sum2_planes, self._sum2_rows

    # ---------------- update staging ----------------

    def row_stride(self) -> int:
        # pad so the K3 tail reads stay in-row, and align rows to 16B
        raw = self.length * self.bpn + 16 * self.bpn  # EPT<=16 guard
        return (raw + 15) // 16 * 16

    def alloc_update_pool(self, n: int) -> torch.Tensor:
        """uint8 [n, stride] rows of packed updates (stride padded/aligned)."""
        return torch.empty(n, self.row_stride(), dtype=torch.uint8, device=self.device)

    def upload_update(self, pool: torch.Tensor, row: int, wire_limbs: bytes):
        t = torch.frombuffer(bytearray(wire_limbs), dtype=torch.uint8)
        # the source is pageable TEMPORARY memory: the copy must be
        # synchronous, or HIP may still be reading the bytearray after Python
        # frees it (observed as heap corruption in the staged-plane soak)
        pool[row, : t.numel()].copy_(t, non_blocking=False)

    # ---------------- unit (scalar) part: CPU, exact ----------------

    def unit_draw(self, seed: bytes) -> int:
        v, _ = _core.mask.unit_draw(seed, self.unit_cfg)
        return int(v)

    def clamped_scalar(self, scalar_num: int, scalar_den: int):
        """The scalar as the masker applies it: clamped to the unit config's
        add_shift, exactly, and reduced to lowest terms (p, q)."""
        if scalar_num < 0 or scalar_den <= 0:
            raise ValueError("a scalar is a non-negative fraction")
        s = min(Fraction(scalar_num, scalar_den),
                Fraction(int(_cfg_scalars(self.unit_cfg)["add_shift"])))
        return s.numerator, s.denominator

    def masked_unit_for(self, seed: bytes, scalar_num: int, scalar_den: int) -> int:
        """Masked scalar for a synthetic update."""
        info = _cfg_scalars(self.unit_cfg)
        exp = int(info["exp_shift_u64"])
        add = int(info["add_shift"])
        # trunc((clamp(scalar)+add)*exp) in exact integers (Bmax shifts
        # included): scalar = num/den <= add by protocol
        shifted = ((scalar_num + add * scalar_den) * exp) // scalar_den
        return (shifted + self.unit_draw(seed)) % int(self.unit_cfg.order)

    def _unmask_scalars(self, mask_unit: int, nb: int, dtype: int | None = None):
        """What every unmask needs besides the tensors: scalar_sum =
        n1/exp_1 - nb*add_1, the vect config's shifts, and the output
        mask::DataType (default: the vect config's). A Bmax unit config has
        nb*add_1 beyond the doubles that n1/exp_1 cancels against, so its
        scalar_sum = (n1 - nb*add_1*exp_1)/exp_1 is formed exactly and rounded
        once. The shifts carry the exact integer "offset" = nb * add_shift *
        exp_shift that the unmask can subtract in the integer domain, and the
        "divisor": with d the offset-free integer, a weight is
        d / (exp_shift * scalar_sum) = d / divisor, divisor = exp_shift *
        (n1 - nb*add_1*exp_1) / exp_1. Integer outputs truncate that
        quotient, which doubles cannot decide - beyond ~2^40 for Bmax, and at
        any size where the quotient is itself an integer (3 participants of
        scalar 1/3 and weight 2 give 1.9999999999963 in doubles) - so the
        divisor is handed on as an exact integer where it is one and fits a
        u64 (the same config for both parts and scalars summing to less than
        2^64 / exp_shift); None otherwise. Bmax configs always unmask through
        the offset; the other bounds do for integer outputs that have a
        divisor (`exact_integers`)."""
        info = _cfg_scalars(self.unit_cfg)
        n1 = (self.unit_acc + int(self.unit_cfg.order) - mask_unit) % int(self.unit_cfg.order)
        exp1 = info["exp_shift_u64"]
        if self.unit_cfg.bound == 255:
            scalar_sum = float(Fraction(n1 - nb * info["add_shift"] * exp1, exp1))
        else:
            scalar_sum = n1 / info["exp_shift"] - nb * info["add_shift"]
        if scalar_sum == 0:
            raise ZeroDivisionError("scalar_sum is zero")
        dt = self.vect_cfg.dtype if dtype is None else dtype
        vinfo = _cfg_scalars(self.vect_cfg)
        # add_shift is an integer for every bound (a float 1.0 .. 1e6 for B0..B6)
        vinfo["offset"] = nb * int(vinfo["add_shift"]) * vinfo["exp_shift_u64"]
        vinfo["divisor"] = None
        div = Fraction(vinfo["exp_shift_u64"] * (n1 - nb * int(info["add_shift"]) * exp1), exp1)
        if div.denominator == 1 and 0 < div < 2**64:
            vinfo["divisor"] = int(div)
        # the same integer at any size the config's limbs hold: what the
        # exact float unmask divides by (exact_divisor)
        vinfo["exact_divisor"] = None
        if div.denominator == 1 and 0 < div < 2**(64 * self.n_limbs):
            vinfo["exact_divisor"] = int(div)
        return scalar_sum, vinfo, dt

    def exact_integers(self, vinfo, dt: int) -> bool:
        """Whether a B0..B6 unmask takes the exact-offset path: integer
        outputs with an exact divisor (and the one-word exp_shift that integer
        vect configs have). Float outputs keep the double steps."""
        return (not self.bmax and dt in (2, 3) and vinfo["divisor"] is not None
                and vinfo["exp_shift_u64"] < 2**64)

    def exact_divisor(self, vinfo, dt: int) -> int | None:
        """What unmask(..., exact=True) needs, or ValueError where exact mode
        does not apply. Float outputs: Q = exp_shift * scalar_sum, a positive
        integer that fits the config's limbs; the weight is then (t - offset)
        / Q rounded once. Integer outputs: None - the default path is already
        the exact truncated quotient, but only with an exact one-word divisor
        (Bmax, or `exact_integers`); with the double steps alone exact mode is
        refused."""
        if dt in (0, 1):
            if vinfo["exact_divisor"] is None:
                raise ValueError(
                    "exact unmask needs exp_shift * scalar_sum to be a positive integer below "
                    f"2^{64 * self.n_limbs} (the same exp_shift for the vector and the unit "
                    "config, and a positive scalar sum)")
            return vinfo["exact_divisor"]
        if vinfo["divisor"] is None or not (self.bmax or self.exact_integers(vinfo, dt)):
            raise ValueError("exact unmask of an integer model needs exp_shift * scalar_sum to "
                             "be an integer below 2^64; only the double steps apply here")
        return None
