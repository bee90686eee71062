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

// decimal string -> u128 (orders/exp_shifts wider than u64)
static unsigned __int128 parse_u128(const std::string& dec) {
    unsigned __int128 v = 0;
    for (char c : dec) {
        if (c < '0' || c > '9') throw std::runtime_error("bad decimal");
        v = v * 10 + unsigned(c - '0');
    }
    return v;
}

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
    // Orders < 2^64. Returns the number of draw ATTEMPTS launched. That is
    // NOT the stream position of the len-th acceptance (the last launch
    // overshoots); a caller needing that position should account on the CPU.
    // Masks are always derived from a fresh seed, so the protocol never uses
    // the tail position.
    uint64_t expand(const std::string& s, uintptr_t out_ptr, uint64_t len,
                    const std::string& order_dec, int prng_nbytes, uint64_t start_word) {
        if (prng_nbytes > 8) throw std::runtime_error("expand: order > 2^64 takes expand_u128");
        uint64_t order = std::stoull(order_dec);
        int wpd = (prng_nbytes + 3) / 4;  // 1 or 2 words per attempt
        int dpt = 16 / wpd;               // draws per thread (16 or 8)
        double p = double(order) * std::pow(2.0, -8.0 * prng_nbytes);  // acceptance
        uint64_t* out = reinterpret_cast<uint64_t*>(out_ptr);
        return run(
            s, len, p, dpt, /*wide=*/false,
            [&](uint64_t attempt, uint64_t n_att, uint32_t* n_wgs) {
                return xhip_k1_candidates(key_.get(), start_word, attempt, n_att, wpd,
                                          prng_nbytes, order, cand_lo_.get(), counts_.get(), dpt,
                                          n_wgs);
            },
            [&](uint32_t n_wgs, uint64_t filled) {
                return xhip_k1_scatter_compact(cand_lo_.get(), counts_.get(), total_.get(),
                                               n_wgs, dpt, filled, out, len);
            });
    }

    // Wide orders (2^64 < order <= 2^128): split lo/hi u64 candidate planes,
    // same pipeline and return value as expand().
    uint64_t expand_u128(const std::string& s, uintptr_t out_lo_ptr, uintptr_t out_hi_ptr,
                         uint64_t len, const std::string& order_dec, int prng_nbytes,
                         uint64_t start_word) {
        if (prng_nbytes <= 8 || prng_nbytes > 16)
            throw std::runtime_error("expand_u128: nbytes must be 9..16");
        unsigned __int128 order = parse_u128(order_dec);
        uint64_t order_lo = uint64_t(order);
        uint64_t order_hi = uint64_t(order >> 64);
        int wpd = (prng_nbytes + 3) / 4;  // 3 or 4
        int apt = 16 / wpd;               // attempts per thread: 5 or 4
        double p = (double(order_hi) * 18446744073709551616.0 + double(order_lo)) *
                   std::pow(2.0, -8.0 * prng_nbytes);
        uint64_t* out_lo = reinterpret_cast<uint64_t*>(out_lo_ptr);
        uint64_t* out_hi = reinterpret_cast<uint64_t*>(out_hi_ptr);
        return run(
            s, len, p, apt, /*wide=*/true,
            [&](uint64_t attempt, uint64_t n_att, uint32_t* n_wgs) {
                return xhip_k1_candidates_u128(key_.get(), start_word, attempt, n_att, wpd,
                                               prng_nbytes, order_lo, order_hi, cand_lo_.get(),
                                               cand_hi_.get(), counts_.get(), apt, n_wgs);
            },
            [&](uint32_t n_wgs, uint64_t filled) {
                return xhip_k1_scatter_compact_u128(cand_lo_.get(), cand_hi_.get(),
                                                    counts_.get(), total_.get(), n_wgs, apt,
                                                    filled, out_lo, out_hi, len);
            });
    }

  private:
    // The expansion loop: size a launch for the elements still missing at
    // acceptance probability p, run candidates -> scan -> scatter, read back
    // the accepted count, repeat until `len` are filled. `apt` is the
    // attempts each candidates thread owns (its workgroups cover 256 * apt).
    template <typename Candidates, typename Scatter>
    uint64_t run(const std::string& seed, uint64_t len, double p, int apt, bool wide,
                 Candidates candidates, Scatter scatter) {
        if (seed.size() != 32) throw std::runtime_error("seed must be 32 bytes");
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
            check(candidates(attempt, n_att, &n_wgs), "k1_candidates");
            check(xhip_k1_scan_hier(counts_.get(), n_wgs, scan_tmp_.get(), total_.get()),
                  "k1_scan");
            check(scatter(n_wgs, filled), "k1_scatter_compact");
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

    DeviceBuffer<uint64_t> cand_lo_;  // the only candidate plane of u64 orders
    DeviceBuffer<uint64_t> cand_hi_;  // wide orders only
    DeviceBuffer<uint32_t> counts_;   // accepted per candidates workgroup
    DeviceBuffer<uint32_t> scan_tmp_;
    DeviceBuffer<uint64_t> total_;
    DeviceBuffer<uint32_t> key_;
};

PYBIND11_MODULE(_hip, m) {
    m.doc() = "xaynet_amd MI355X (gfx950) kernels: mask expand, aggregate, unmask";

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

    py::class_<MaskExpander>(m, "MaskExpander")
        .def(py::init<>())
        .def("expand", &MaskExpander::expand, py::arg("seed"), py::arg("out_ptr"), py::arg("len"),
             py::arg("order"), py::arg("prng_nbytes"), py::arg("start_word"),
             py::call_guard<py::gil_scoped_release>())
        .def("expand_u128", &MaskExpander::expand_u128, py::arg("seed"), py::arg("out_lo_ptr"),
             py::arg("out_hi_ptr"), py::arg("len"), py::arg("order"), py::arg("prng_nbytes"),
             py::arg("start_word"), py::call_guard<py::gil_scoped_release>());

    m.def(
        "aggregate_batch",
        [](uintptr_t acc, uintptr_t updates, uint64_t stride, uint32_t n_updates, uint64_t len,
           int bpn, int ept) {
            check(xhip_k3_aggregate(reinterpret_cast<uint64_t*>(acc),
                                    reinterpret_cast<const uint8_t*>(updates), stride, n_updates,
                                    len, bpn, ept),
                  "k3_aggregate");
        },
        py::arg("acc"), py::arg("updates"), py::arg("stride"), py::arg("n_updates"),
        py::arg("len"), py::arg("bpn"), py::arg("ept") = 0,
        py::call_guard<py::gil_scoped_release>());

    // dtype follows mask::DataType: 0=F32 1=F64 2=I32 3=I64
    m.def(
        "unmask",
        [](uintptr_t acc, uintptr_t mask, uintptr_t out, uint64_t len, int n_digits,
           const std::string& order_dec, uint64_t exp_shift, double n_add_shift,
           double scalar_sum, int dtype) {
            check(xhip_k4_unmask(reinterpret_cast<const uint64_t*>(acc),
                                 reinterpret_cast<const uint64_t*>(mask), dtype,
                                 reinterpret_cast<void*>(out), len, n_digits,
                                 std::stoull(order_dec), exp_shift, n_add_shift, scalar_sum),
                  "k4_unmask");
        },
        py::arg("acc"), py::arg("mask"), py::arg("out"), py::arg("len"), py::arg("n_digits"),
        py::arg("order"), py::arg("exp_shift"), py::arg("n_add_shift"),
        py::arg("scalar_sum"), py::arg("dtype") = 0,
        py::call_guard<py::gil_scoped_release>());

    m.def(
        "unmask_values",
        [](uintptr_t vals, uintptr_t mask, uintptr_t out, uint64_t len,
           const std::string& order_dec, uint64_t exp_shift, double n_add_shift,
           double scalar_sum, int dtype) {
            check(xhip_k4_unmask_values(reinterpret_cast<const uint64_t*>(vals),
                                        reinterpret_cast<const uint64_t*>(mask), dtype,
                                        reinterpret_cast<void*>(out), len, std::stoull(order_dec),
                                        exp_shift, n_add_shift, scalar_sum),
                  "k4_unmask_values");
        },
        py::call_guard<py::gil_scoped_release>());

    // ---- u128-order variants (bpn 9..16: F64 families, narrow Bmax) ----
    m.def(
        "canonicalize_u128",
        [](uintptr_t acc, uintptr_t out_lo, uintptr_t out_hi, uint64_t len, int n_digits,
           const std::string& order_dec, int digit_bits) {
            auto o = parse_u128(order_dec);
            check(xhip_k2_canonicalize_u128(reinterpret_cast<const uint64_t*>(acc),
                                            reinterpret_cast<uint64_t*>(out_lo),
                                            reinterpret_cast<uint64_t*>(out_hi), len, n_digits,
                                            digit_bits, uint64_t(o), uint64_t(o >> 64)),
                  "k2_canonicalize_u128");
        },
        py::arg("acc"), py::arg("out_lo"), py::arg("out_hi"), py::arg("len"),
        py::arg("n_digits"), py::arg("order"), py::arg("digit_bits") = 32,
        py::call_guard<py::gil_scoped_release>());
    // canonical lo/hi values -> add into k planes of digit_bits-wide digits
    m.def(
        "add_u128_to_planes",
        [](uintptr_t planes, uintptr_t lo, uintptr_t hi, uint64_t len, int k, int digit_bits) {
            check(xhip_add_u128_to_planes(reinterpret_cast<uint64_t*>(planes),
                                          reinterpret_cast<const uint64_t*>(lo),
                                          reinterpret_cast<const uint64_t*>(hi), len, k,
                                          digit_bits),
                  "add_u128_to_planes");
        },
        py::arg("planes"), py::arg("lo"), py::arg("hi"), py::arg("len"), py::arg("k"),
        py::arg("digit_bits") = 32, py::call_guard<py::gil_scoped_release>());
    // 32-bit accumulator planes -> k compact planes of the value mod order
    m.def(
        "recode_planes_u128",
        [](uintptr_t acc, uintptr_t out, uint64_t len, int n_digits,
           const std::string& order_dec, int k, int digit_bits) {
            auto o = parse_u128(order_dec);
            check(xhip_k2_recode_planes_u128(reinterpret_cast<const uint64_t*>(acc),
                                             reinterpret_cast<uint64_t*>(out), len, n_digits,
                                             uint64_t(o), uint64_t(o >> 64), k, digit_bits),
                  "k2_recode_planes_u128");
        },
        py::arg("acc"), py::arg("out"), py::arg("len"), py::arg("n_digits"), py::arg("order"),
        py::arg("k"), py::arg("digit_bits"), py::call_guard<py::gil_scoped_release>());
    m.def(
        "mod_add_u128",
        [](uintptr_t a_lo, uintptr_t a_hi, uintptr_t b_lo, uintptr_t b_hi, uint64_t len,
           const std::string& order_dec) {
            auto o = parse_u128(order_dec);
            check(xhip_k2_mod_add_u128(reinterpret_cast<uint64_t*>(a_lo),
                                       reinterpret_cast<uint64_t*>(a_hi),
                                       reinterpret_cast<const uint64_t*>(b_lo),
                                       reinterpret_cast<const uint64_t*>(b_hi), len, uint64_t(o),
                                       uint64_t(o >> 64)),
                  "k2_mod_add_u128");
        },
        py::call_guard<py::gil_scoped_release>());
    m.def(
        "unpack_u128",
        [](uintptr_t in, uintptr_t out_lo, uintptr_t out_hi, uint64_t len, int bpn) {
            check(xhip_k6_unpack_u128(reinterpret_cast<const uint8_t*>(in),
                                      reinterpret_cast<uint64_t*>(out_lo),
                                      reinterpret_cast<uint64_t*>(out_hi), len, bpn),
                  "k6_unpack_u128");
        },
        py::call_guard<py::gil_scoped_release>());
    m.def(
        "unmask_u128",
        [](uintptr_t acc, uintptr_t mask_lo, uintptr_t mask_hi, uintptr_t out, uint64_t len,
           int n_digits, const std::string& order_dec, const std::string& exp_dec,
           double n_add_shift, double scalar_sum, int dtype, int digit_bits) {
            if (dtype < 0 || dtype > 3) throw std::runtime_error("bad dtype");
            auto o = parse_u128(order_dec);
            auto e = parse_u128(exp_dec);
            check(xhip_k4_unmask_u128(reinterpret_cast<const uint64_t*>(acc),
                                      reinterpret_cast<const uint64_t*>(mask_lo),
                                      reinterpret_cast<const uint64_t*>(mask_hi),
                                      reinterpret_cast<void*>(out), len, n_digits, digit_bits,
                                      uint64_t(o), uint64_t(o >> 64), uint64_t(e),
                                      uint64_t(e >> 64), n_add_shift, scalar_sum, dtype),
                  "k4_unmask_u128");
        },
        py::arg("acc"), py::arg("mask_lo"), py::arg("mask_hi"), py::arg("out"), py::arg("len"),
        py::arg("n_digits"), py::arg("order"), py::arg("exp_shift"), py::arg("n_add_shift"),
        py::arg("scalar_sum"), py::arg("dtype"), py::arg("digit_bits") = 32,
        py::call_guard<py::gil_scoped_release>());

    m.def(
        "canonicalize",
        [](uintptr_t acc, uintptr_t out, uint64_t len, int n_digits, const std::string& order) {
            check(xhip_k2_canonicalize(reinterpret_cast<const uint64_t*>(acc),
                                       reinterpret_cast<uint64_t*>(out), len, n_digits,
                                       std::stoull(order)),
                  "k2_canonicalize");
        },
        py::call_guard<py::gil_scoped_release>());

    m.def(
        "mod_add_u64",
        [](uintptr_t a, uintptr_t b, uint64_t len, const std::string& order) {
            check(xhip_k2_mod_add_u64(reinterpret_cast<uint64_t*>(a),
                                      reinterpret_cast<const uint64_t*>(b), len,
                                      std::stoull(order)),
                  "k2_mod_add");
        },
        py::call_guard<py::gil_scoped_release>());

    m.def(
        "mask_pack",
        [](uintptr_t mask, uintptr_t out, uint64_t len, int bpn, const std::string& order,
           uint64_t participant, double scalar, double add_shift, double exp_shift_d,
           uint64_t exp_shift) {
            check(xhip_k5_mask_pack(reinterpret_cast<const uint64_t*>(mask),
                                    reinterpret_cast<uint8_t*>(out), len, bpn,
                                    std::stoull(order), participant, scalar, add_shift,
                                    exp_shift_d, exp_shift),
                  "k5_mask_pack");
        },
        py::call_guard<py::gil_scoped_release>());

    m.def(
        "mask_pack_u128",
        [](uintptr_t mask_lo, uintptr_t mask_hi, uintptr_t out, uint64_t len, int bpn,
           const std::string& order, uint64_t participant, double scalar, double add_shift,
           double exp_shift_d) {
            unsigned __int128 o = parse_u128(order);
            check(xhip_k5_mask_pack_u128(reinterpret_cast<const uint64_t*>(mask_lo),
                                         reinterpret_cast<const uint64_t*>(mask_hi),
                                         reinterpret_cast<uint8_t*>(out), len, bpn, uint64_t(o),
                                         uint64_t(o >> 64), participant, scalar, add_shift,
                                         exp_shift_d),
                  "k5_mask_pack_u128");
        },
        py::call_guard<py::gil_scoped_release>());

    m.def(
        "mask_weights",
        [](uintptr_t w, int dtype, uintptr_t mask_lo, uintptr_t mask_hi, uintptr_t out,
           uint64_t len, int bpn, const std::string& order, double scalar, double add_shift,
           const std::string& exp_shift, bool wide) {
            unsigned __int128 o = parse_u128(order);
            unsigned __int128 e = parse_u128(exp_shift);
            check(xhip_k5_mask_weights(reinterpret_cast<const void*>(w), dtype,
                                       reinterpret_cast<const uint64_t*>(mask_lo),
                                       reinterpret_cast<const uint64_t*>(mask_hi),
                                       reinterpret_cast<uint8_t*>(out), len, bpn, uint64_t(o),
                                       uint64_t(o >> 64), scalar, add_shift, uint64_t(e),
                                       uint64_t(e >> 64), wide ? 1 : 0),
                  "k5_mask_weights");
        },
        py::call_guard<py::gil_scoped_release>());

    m.def(
        "pack_u128",
        [](uintptr_t in_lo, uintptr_t in_hi, uintptr_t out, uint64_t len, int bpn) {
            check(xhip_k6_pack_u128(reinterpret_cast<const uint64_t*>(in_lo),
                                    reinterpret_cast<const uint64_t*>(in_hi),
                                    reinterpret_cast<uint8_t*>(out), len, bpn),
                  "k6_pack_u128");
        },
        py::call_guard<py::gil_scoped_release>());

    m.def(
        "unpack_u64",
        [](uintptr_t in, uintptr_t out, uint64_t len, int bpn) {
            check(xhip_k6_unpack_u64(reinterpret_cast<const uint8_t*>(in),
                                     reinterpret_cast<uint64_t*>(out), len, bpn),
                  "k6_unpack");
        },
        py::call_guard<py::gil_scoped_release>());

    m.def(
        "pack_u64",
        [](uintptr_t in, uintptr_t out, uint64_t len, int bpn) {
            check(xhip_k6_pack_u64(reinterpret_cast<const uint64_t*>(in),
                                   reinterpret_cast<uint8_t*>(out), len, bpn),
                  "k6_pack");
        },
        py::call_guard<py::gil_scoped_release>());

    m.def(
        "add_u64_to_planes",
        [](uintptr_t acc, uintptr_t vals, uint64_t len, int n_digits) {
            check(xhip_add_u64_to_planes(reinterpret_cast<uint64_t*>(acc),
                                         reinterpret_cast<const uint64_t*>(vals), len, n_digits),
                  "add_u64_to_planes");
        },
        py::call_guard<py::gil_scoped_release>());
}
