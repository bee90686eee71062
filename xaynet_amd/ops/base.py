"""What the GPU engine and its CPU analog share: the config-derived fields,
the update-pool layout, the exact CPU-side unit (scalar) arithmetic and the
shape of canonical value tensors."""
import torch

from xaynet_amd import _core


def _cfg_scalars(cfg):
    """exp/add shifts as python scalars (non-Bmax configs)."""
    exp_exp = {0: 10, 1: 20, 2: 10, 3: 10}[cfg.dtype]  # non-Bmax
    if cfg.bound == 255:
        raise ValueError("Bmax configs are not on the u64 GPU path")
    add = {0: 1.0, 2: 100.0, 4: 10_000.0, 6: 1_000_000.0}[cfg.bound]
    return {
        "exp_shift": float(10**exp_exp),
        "exp_shift_u64": 10**exp_exp,
        "add_shift": add,
    }


class MaskedAggregatorBase:
    """Digit-plane aggregation state of one model: int64 [n_digits, length]
    accumulator planes plus the exact masked scalar sum."""

    _TORCH_DTYPES = {0: torch.float32, 1: torch.float64, 2: torch.int32, 3: torch.int64}

    def __init__(self, vect_cfg, unit_cfg, length: int, device):
        if vect_cfg.bytes_per_number > 16:
            raise ValueError(
                f"{type(self).__name__} covers group orders up to 2^128 (got "
                f"{vect_cfg.bytes_per_number} bytes/element); use the CPU oracle for this config"
            )
        self.vect_cfg = vect_cfg
        self.unit_cfg = unit_cfg
        self.length = length
        self.device = torch.device(device)
        self.bpn = vect_cfg.bytes_per_number
        # wide (order >= 2^64) configs: canonical values are split lo/hi u64
        # rows, [2, n]; u64 orders: [n]
        self.wide = not vect_cfg.order_fits_u64
        self.n_digits = (self.bpn + 3) // 4
        self.order = vect_cfg.order  # decimal string
        self.order_int = int(vect_cfg.order)
        self.prng_nbytes = vect_cfg.prng_nbytes
        self.acc = torch.zeros(self.n_digits, length, dtype=torch.int64, device=self.device)
        self.nb_models = 0
        self.unit_acc = 0  # masked scalar sum (CPU, exact)

    def reset(self):
        self.acc.zero_()
        self.nb_models = 0
        self.unit_acc = 0

    def new_values(self, n: int | None = None, zero: bool = False) -> torch.Tensor:
        """A canonical value tensor for n (default: length) elements: int64
        [n], or [2, n] lo/hi rows when the order is wide."""
        n = self.length if n is None else n
        shape = (2, n) if self.wide else (n,)
        make = torch.zeros if zero else torch.empty
        return make(*shape, dtype=torch.int64, device=self.device)

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

    def masked_unit_for(self, seed: bytes, scalar_num: int, scalar_den: int) -> int:
        """Masked scalar for a synthetic update."""
        info = _cfg_scalars(self.unit_cfg)
        exp = int(info["exp_shift"])
        add = int(info["add_shift"])
        # trunc((clamp(scalar)+add)*exp): scalar = num/den <= add by protocol
        shifted = ((scalar_num + add * scalar_den) * exp) // scalar_den
        return (shifted + self.unit_draw(seed)) % int(self.unit_cfg.order)

    def _unmask_scalars(self, mask_unit: int, nb: int, dtype: int | None = None):
        """What every unmask needs besides the tensors: scalar_sum =
        n1/exp_1 - nb*add_1, the vect config's shifts, and the output
        mask::DataType (default: the vect config's)."""
        info = _cfg_scalars(self.unit_cfg)
        n1 = (self.unit_acc + int(self.unit_cfg.order) - mask_unit) % int(self.unit_cfg.order)
        scalar_sum = n1 / info["exp_shift"] - nb * info["add_shift"]
        if scalar_sum == 0:
            raise ZeroDivisionError("scalar_sum is zero")
        dt = self.vect_cfg.dtype if dtype is None else dtype
        return scalar_sum, _cfg_scalars(self.vect_cfg), dt
