// pybind11 module `xaynet_amd._hip` — host orchestration for the MI355X
// kernels in kernels.hip. Compiled with hipcc (gfx950); no torch headers —
// callers pass raw device pointers (torch `tensor.data_ptr()`), and all
// launches go to the null stream, which serializes with PyTorch's default
// stream on the device.
#include <pybind11/pybind11.h>

#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>

#include "kernels.h"

namespace py = pybind11;

// Orders and exp_shifts cross the Python boundary as decimal strings and the
// launcher ABI as lo/hi halves.
struct U128 {
    uint64_t lo, hi;
};

static U128 parse_u128(const std::string& dec) {
    if (dec.empty()) throw std::runtime_error("bad decimal");
    unsigned __int128 v = 0;
    for (char c : dec) {
        if (c < '0' || c > '9') throw std::runtime_error("bad decimal");
        v = v * 10 + unsigned(c - '0');
    }
    return {uint64_t(v), uint64_t(v >> 64)};
}

// The one width rule: an order is wide iff it is >= 2^64, and canonical
// values are a (lo, hi) pointer pair whose hi is null exactly for u64 orders.
// Checked before any HIP call; the launchers rely on it.
static U128 parse_order(const std::string& dec, uintptr_t hi_ptr) {
    U128 o = parse_u128(dec);
    if ((hi_ptr != 0) != (o.hi != 0))
        throw py::value_error(o.hi ? "order >= 2^64 takes split lo/hi values (hi pointer is null)"
                                   : "order < 2^64 takes plain u64 values (hi pointer is set)");
    return o;
}

// u64-order digit planes are 32 bits wide (the u64 kernels know no other).
static void check_digit_bits(const U128& order, int digit_bits) {
    if (order.hi == 0 && digit_bits != 32)
        throw py::value_error("u64-order digit planes are 32 bits wide");
}

static uint64_t* u64p(uintptr_t p) { return reinterpret_cast<uint64_t*>(p); }
static uint8_t* u8p(uintptr_t p) { return reinterpret_cast<uint8_t*>(p); }

static void check(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    }
}

// Move-only owner of one device allocation. reserve(n) grows it to at least n
// elements (contents are not kept); if the allocation fails the buffer is
// left empty, so nothing dangles and nothing is freed twice.
template <typename T>
class DeviceBuffer {
  public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : ptr_(o.ptr_), cap_(o.cap_) {
        o.ptr_ = nullptr;
        o.cap_ = 0;
    }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        std::swap(ptr_, o.ptr_);
        std::swap(cap_, o.cap_);
        return *this;
    }
    ~DeviceBuffer() {
        if (ptr_) (void)hipFree(ptr_);
    }

    void reserve(uint64_t n, const char* what) {
        if (n <= cap_) return;
        if (ptr_) (void)hipFree(ptr_);
        ptr_ = nullptr;
        cap_ = 0;
        check(hipMalloc(&ptr_, n * sizeof(T)), what);
        cap_ = n;
    }
    T* get() const { return ptr_; }

  private:
    T* ptr_ = nullptr;
    uint64_t cap_ = 0;
};

// ------------------------------------------------------------- MaskExpander
//
// Owns the rejection-sampling workspace. expand() reproduces the reference
// ChaCha20 draw stream exactly (see kernels.hip header comment): the caller
// provides start_word = keystream words consumed by the preceding unit draw
// (computed on CPU via _core.mask.unit_draw).
class MaskExpander {
  public:
    // Size a launch for the elements still missing at the acceptance
    // probability, run candidates -> scan -> scatter, read back the accepted
    // count, repeat until `len` are filled. Returns the number of draw
    // ATTEMPTS launched. That is NOT the stream position of the len-th
    // acceptance (the last launch overshoots); a caller needing that position
    // should account on the CPU. Masks are always derived from a fresh seed,
    // so the protocol never uses the tail position.
    uint64_t expand(const std::string& seed, uintptr_t out_lo_ptr, uintptr_t out_hi_ptr,
                    uint64_t len, const std::string& order_dec, int prng_nbytes,
                    uint64_t start_word) {
        const U128 order = parse_order(order_dec, out_hi_ptr);
        const bool wide = order.hi != 0;
        if (seed.size() != 32) throw py::value_error("seed must be 32 bytes");
        if (prng_nbytes < (wide ? 9 : 1) || prng_nbytes > (wide ? 16 : 8))
            throw py::value_error("prng_nbytes must be 1..8 for u64 orders, 9..16 for wide");
        const int wpd = (prng_nbytes + 3) / 4;  // keystream words per attempt: 1..4
        const int apt = 16 / wpd;  // attempts per candidates thread (workgroups cover 256 * apt)
        const double p = (double(order.hi) * 18446744073709551616.0 + double(order.lo)) *
                         std::pow(2.0, -8.0 * prng_nbytes);  // acceptance
        uint64_t* out_lo = u64p(out_lo_ptr);
        uint64_t* out_hi = u64p(out_hi_ptr);

        key_.reserve(8, "alloc key");
        total_.reserve(1, "alloc total");
        check(hipMemcpy(key_.get(), seed.data(), 32, hipMemcpyHostToDevice), "seed H2D");

        uint64_t filled = 0, attempt = 0;
        while (filled < len) {
            uint64_t remaining = len - filled;
            double exp_att = double(remaining) / p;
            uint64_t n_att = uint64_t(exp_att + 6.0 * std::sqrt(exp_att / p) + 1024.0);
            // accepted draws compact into per-workgroup segments of `cand`,
            // the last one cut at n_att; counts: one per workgroup
            uint64_t max_wgs = (n_att + 256 * apt - 1) / (256 * apt) + 2;
            cand_lo_.reserve(n_att, "alloc cand");
            if (wide) cand_hi_.reserve(n_att, "alloc cand_hi");
            counts_.reserve(max_wgs, "alloc counts");
            scan_tmp_.reserve(max_wgs / 1024 + 2, "alloc scan tmp");

            uint32_t n_wgs = 0;
            check(xhip_k1_candidates(key_.get(), start_word, attempt, n_att, wpd, prng_nbytes,
                                     order.lo, order.hi, cand_lo_.get(), cand_hi_.get(),
                                     counts_.get(), apt, &n_wgs),
                  "k1_candidates");
            check(xhip_k1_scan_hier(counts_.get(), n_wgs, scan_tmp_.get(), total_.get()),
                  "k1_scan");
            check(xhip_k1_scatter_compact(cand_lo_.get(), cand_hi_.get(), counts_.get(),
                                          total_.get(), n_wgs, apt, filled, out_lo, out_hi, len),
                  "k1_scatter_compact");
            uint64_t round_accepted = 0;
            check(hipMemcpy(&round_accepted, total_.get(), 8, hipMemcpyDeviceToHost),
                  "total D2H");
            filled += round_accepted;  // may overshoot len; clamped below
            if (filled > len) filled = len;
            attempt += n_att;
            if (round_accepted == 0 && n_att > 0 && p <= 0.0)
                throw std::runtime_error("expand: zero acceptance");
        }
        return attempt;
    }

  private:
    DeviceBuffer<uint64_t> cand_lo_;  // the only candidate plane of u64 orders
    DeviceBuffer<uint64_t> cand_hi_;  // wide orders only
    DeviceBuffer<uint32_t> counts_;   // accepted per candidates workgroup
    DeviceBuffer<uint32_t> scan_tmp_;
    DeviceBuffer<uint64_t> total_;
    DeviceBuffer<uint32_t> key_;
};

PYBIND11_MODULE(_hip, m) {
    m.doc() = "xaynet_amd MI355X (gfx950) kernels: mask expand, aggregate, unmask";
    const auto nogil = py::call_guard<py::gil_scoped_release>();

    m.def("device_count", []() {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        return e == hipSuccess ? n : 0;
    });
    m.def("synchronize", []() { check(hipDeviceSynchronize(), "sync"); });

    // Pin an existing host range (e.g. a POSIX shared-memory mapping) so
    // H2D copies from it can be asynchronous DMA — the serve plane's ingest
    // ring is a shm region shared with the coordinator process.
    m.def("host_register", [](uintptr_t ptr, size_t size) {
        check(hipHostRegister(reinterpret_cast<void*>(ptr), size, hipHostRegisterDefault),
              "hipHostRegister");
    });
    m.def("host_unregister", [](uintptr_t ptr) {
        check(hipHostUnregister(reinterpret_cast<void*>(ptr)), "hipHostUnregister");
    });

    // Every function below that takes canonical values takes them as
    // (lo, hi) device pointers plus the order as a decimal string; see
    // parse_order. exp_shift is a decimal string too (10^20 for f64 configs).
    py::class_<MaskExpander>(m, "MaskExpander")
        .def(py::init<>())
        .def("expand", &MaskExpander::expand, py::arg("seed"), py::arg("out_lo"),
             py::arg("out_hi"), py::arg("len"), py::arg("order"), py::arg("prng_nbytes"),
             py::arg("start_word"), nogil);

    m.def(
        "aggregate_batch",
        [](uintptr_t acc, uintptr_t updates, uint64_t stride, uint32_t n_updates, uint64_t len,
           int bpn, int ept) {
            check(xhip_k3_aggregate(u64p(acc), u8p(updates), stride, n_updates, len, bpn, ept),
                  "k3_aggregate");
        },
        py::arg("acc"), py::arg("updates"), py::arg("stride"), py::arg("n_updates"),
        py::arg("len"), py::arg("bpn"), py::arg("ept") = 0, nogil);

    // [n_planes][len] digit planes minus the mask -> model weights.
    // dtype follows mask::DataType: 0=F32 1=F64 2=I32 3=I64
    m.def(
        "unmask",
        [](uintptr_t planes, uintptr_t mask_lo, uintptr_t mask_hi, uintptr_t out, uint64_t len,
           int n_planes, const std::string& order, const std::string& exp_shift,
           double n_add_shift, double scalar_sum, int dtype, int digit_bits) {
            U128 o = parse_order(order, mask_hi), e = parse_u128(exp_shift);
            check_digit_bits(o, digit_bits);
            check(xhip_k4_unmask(u64p(planes), u64p(mask_lo), u64p(mask_hi), dtype,
                                 reinterpret_cast<void*>(out), len, n_planes, digit_bits, o.lo,
                                 o.hi, e.lo, e.hi, n_add_shift, scalar_sum),
                  "k4_unmask");
        },
        py::arg("planes"), py::arg("mask_lo"), py::arg("mask_hi"), py::arg("out"),
        py::arg("len"), py::arg("n_planes"), py::arg("order"), py::arg("exp_shift"),
        py::arg("n_add_shift"), py::arg("scalar_sum"), py::arg("dtype") = 0,
        py::arg("digit_bits") = 32, nogil);

    // u64 orders only: `vals` are plain u64 (cross-rank sums of) canonical values
    m.def(
        "unmask_values",
        [](uintptr_t vals, uintptr_t mask_lo, uintptr_t mask_hi, uintptr_t out, uint64_t len,
           const std::string& order, const std::string& exp_shift, double n_add_shift,
           double scalar_sum, int dtype) {
            U128 o = parse_order(order, mask_hi), e = parse_u128(exp_shift);
            if (o.hi || e.hi) throw py::value_error("unmask_values covers u64 orders");
            check(xhip_k4_unmask_values(u64p(vals), u64p(mask_lo), dtype,
                                        reinterpret_cast<void*>(out), len, o.lo, e.lo,
                                        n_add_shift, scalar_sum),
                  "k4_unmask_values");
        },
        py::arg("vals"), py::arg("mask_lo"), py::arg("mask_hi"), py::arg("out"), py::arg("len"),
        py::arg("order"), py::arg("exp_shift"), py::arg("n_add_shift"), py::arg("scalar_sum"),
        py::arg("dtype") = 0, nogil);

    // [n_planes][len] digit planes -> canonical values mod order
    m.def(
        "canonicalize",
        [](uintptr_t planes, uintptr_t out_lo, uintptr_t out_hi, uint64_t len, int n_planes,
           const std::string& order, int digit_bits) {
            U128 o = parse_order(order, out_hi);
            check_digit_bits(o, digit_bits);
            check(xhip_k2_canonicalize(u64p(planes), u64p(out_lo), u64p(out_hi), len, n_planes,
                                       digit_bits, o.lo, o.hi),
                  "k2_canonicalize");
        },
        py::arg("planes"), py::arg("out_lo"), py::arg("out_hi"), py::arg("len"),
        py::arg("n_planes"), py::arg("order"), py::arg("digit_bits") = 32, nogil);

    // canonical values -> add into [n_planes][len] planes of digit_bits-wide digits
    m.def(
        "add_to_planes",
        [](uintptr_t planes, uintptr_t lo, uintptr_t hi, uint64_t len, int n_planes,
           const std::string& order, int digit_bits) {
            check_digit_bits(parse_order(order, hi), digit_bits);
            check(xhip_add_to_planes(u64p(planes), u64p(lo), u64p(hi), len, n_planes,
                                     digit_bits),
                  "add_to_planes");
        },
        py::arg("planes"), py::arg("lo"), py::arg("hi"), py::arg("len"), py::arg("n_planes"),
        py::arg("order"), py::arg("digit_bits") = 32, nogil);

    // wide orders only: 32-bit accumulator planes -> k compact planes of the
    // value mod order
    m.def(
        "recode_planes",
        [](uintptr_t acc, uintptr_t out, uint64_t len, int n_digits, const std::string& order,
           int k, int digit_bits) {
            U128 o = parse_u128(order);
            if (!o.hi) throw py::value_error("recode_planes covers wide (u128) orders");
            check(xhip_k2_recode_planes(u64p(acc), u64p(out), len, n_digits, o.lo, o.hi, k,
                                        digit_bits),
                  "k2_recode_planes");
        },
        py::arg("acc"), py::arg("out"), py::arg("len"), py::arg("n_digits"), py::arg("order"),
        py::arg("k"), py::arg("digit_bits"), nogil);

    // a = (a + b) mod order
    m.def(
        "mod_add",
        [](uintptr_t a_lo, uintptr_t a_hi, uintptr_t b_lo, uintptr_t b_hi, uint64_t len,
           const std::string& order) {
            U128 o = parse_order(order, a_hi);
            parse_order(order, b_hi);
            check(xhip_k2_mod_add(u64p(a_lo), u64p(a_hi), u64p(b_lo), u64p(b_hi), len, o.lo,
                                  o.hi),
                  "k2_mod_add");
        },
        py::arg("a_lo"), py::arg("a_hi"), py::arg("b_lo"), py::arg("b_hi"), py::arg("len"),
        py::arg("order"), nogil);

    // synthetic update row: hash weights, quantize, add the mask, pack
    m.def(
        "mask_pack",
        [](uintptr_t mask_lo, uintptr_t mask_hi, uintptr_t out, uint64_t len, int bpn,
           const std::string& order, uint64_t participant, double scalar, double add_shift,
           const std::string& exp_shift) {
            U128 o = parse_order(order, mask_hi), e = parse_u128(exp_shift);
            check(xhip_k5_mask_pack(u64p(mask_lo), u64p(mask_hi), u8p(out), len, bpn, o.lo, o.hi,
                                    participant, scalar, add_shift, e.lo, e.hi),
                  "k5_mask_pack");
        },
        py::arg("mask_lo"), py::arg("mask_hi"), py::arg("out"), py::arg("len"), py::arg("bpn"),
        py::arg("order"), py::arg("participant"), py::arg("scalar"), py::arg("add_shift"),
        py::arg("exp_shift"), nogil);

    // real weights (dtype as for unmask): quantize, add the mask, pack
    m.def(
        "mask_weights",
        [](uintptr_t w, int dtype, uintptr_t mask_lo, uintptr_t mask_hi, uintptr_t out,
           uint64_t len, int bpn, const std::string& order, double scalar, double add_shift,
           const std::string& exp_shift) {
            U128 o = parse_order(order, mask_hi), e = parse_u128(exp_shift);
            check(xhip_k5_mask_weights(reinterpret_cast<const void*>(w), dtype, u64p(mask_lo),
                                       u64p(mask_hi), u8p(out), len, bpn, o.lo, o.hi, scalar,
                                       add_shift, e.lo, e.hi),
                  "k5_mask_weights");
        },
        py::arg("w"), py::arg("dtype"), py::arg("mask_lo"), py::arg("mask_hi"), py::arg("out"),
        py::arg("len"), py::arg("bpn"), py::arg("order"), py::arg("scalar"),
        py::arg("add_shift"), py::arg("exp_shift"), nogil);

    // canonical values <-> packed wire limbs of bpn bytes
    m.def(
        "pack",
        [](uintptr_t in_lo, uintptr_t in_hi, uintptr_t out, uint64_t len, int bpn,
           const std::string& order) {
            parse_order(order, in_hi);
            check(xhip_k6_pack(u64p(in_lo), u64p(in_hi), u8p(out), len, bpn), "k6_pack");
        },
        py::arg("in_lo"), py::arg("in_hi"), py::arg("out"), py::arg("len"), py::arg("bpn"),
        py::arg("order"), nogil);
    m.def(
        "unpack",
        [](uintptr_t in, uintptr_t out_lo, uintptr_t out_hi, uint64_t len, int bpn,
           const std::string& order) {
            parse_order(order, out_hi);
            check(xhip_k6_unpack(u8p(in), u64p(out_lo), u64p(out_hi), len, bpn), "k6_unpack");
        },
        py::arg("packed"), py::arg("out_lo"), py::arg("out_hi"), py::arg("len"), py::arg("bpn"),
        py::arg("order"), nogil);
}
