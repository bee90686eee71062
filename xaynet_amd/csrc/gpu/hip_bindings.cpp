// pybind11 module `xaynet_amd._hip` — host orchestration for the MI355X
// kernels in kernels.hip. Compiled with hipcc (gfx950); no torch headers —
// callers pass raw device pointers (torch `tensor.data_ptr()`), and all
// launches go to the null stream, which serializes with PyTorch's default
// stream on the device.
#include <pybind11/pybind11.h>

#include <pybind11/stl.h>

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "kernels.h"

namespace py = pybind11;

// Orders, exp_shifts and offsets cross the Python boundary as decimal strings
// and the launcher ABI as five u64 limbs (xhip_limbs): values below 2^320.
struct Limbs {
    xhip_limbs v;
    int n;  // limb count, ceil(bits / 64), at least 1

    bool is_zero() const { return n == 1 && v.w[0] == 0; }
};

static Limbs parse_limbs(const std::string& dec) {
    if (dec.empty()) throw std::runtime_error("bad decimal");
    Limbs r{{{0, 0, 0, 0, 0}}, 1};
    for (char c : dec) {
        if (c < '0' || c > '9') throw std::runtime_error("bad decimal");
        uint64_t carry = unsigned(c - '0');
        for (int j = 0; j < ML_MAX_LIMBS; ++j) {
            unsigned __int128 t = (unsigned __int128)r.v.w[j] * 10 + carry;
            r.v.w[j] = uint64_t(t);
            carry = uint64_t(t >> 64);
        }
        if (carry) throw py::value_error("orders and shifts must be below 2^320");
    }
    for (int j = 1; j < ML_MAX_LIMBS; ++j)
        if (r.v.w[j]) r.n = j + 1;
    return r;
}

// an optional constant: the empty string is 0
static Limbs parse_optional(const std::string& dec) {
    if (dec.empty()) return Limbs{{{0, 0, 0, 0, 0}}, 1};
    return parse_limbs(dec);
}

// A double that is an integer in [1, 2^320) as limbs, exactly; false for any
// other double.
static bool integral_limbs(double x, Limbs& out) {
    if (!(x >= 1.0) || !std::isfinite(x) || x != std::floor(x)) return false;
    int e;
    const double m = std::frexp(x, &e);  // x = m * 2^e, m in [0.5, 1), e >= 1
    if (e > 64 * ML_MAX_LIMBS) return false;
    limbs<ML_MAX_LIMBS> v = ml_zero<ML_MAX_LIMBS>();
    v.w[0] = uint64_t(std::ldexp(m, 53));  // the 53-bit mantissa
    if (e >= 53) {
        ml_shl(v, e - 53);
    } else {
        v.w[0] >>= 53 - e;  // x is an integer: only zeros leave
    }
    out = Limbs{{{v.w[0], v.w[1], v.w[2], v.w[3], v.w[4]}}, 1};
    for (int j = 1; j < ML_MAX_LIMBS; ++j)
        if (out.v.w[j]) out.n = j + 1;
    return true;
}

// The one width rule: an order is wide iff it is >= 2^64, and canonical
// values are a (lo, hi) pointer pair whose hi is null exactly for u64 orders.
// For wide orders lo and hi are limb rows 0 and 1, and row j of the order's
// ceil(bits/64) rows lives at lo + j*(hi - lo). Checked before any HIP call;
// the launchers rely on it.
static Limbs parse_order(const std::string& dec, uintptr_t hi_ptr) {
    Limbs o = parse_limbs(dec);
    const bool wide = o.n > 1;
    if ((hi_ptr != 0) != wide)
        throw py::value_error(wide ? "order >= 2^64 takes split lo/hi values (hi pointer is null)"
                                   : "order < 2^64 takes plain u64 values (hi pointer is set)");
    return o;
}

// u64-order digit planes are 32 bits wide (the u64 kernels know no other).
static void check_digit_bits(const Limbs& order, int digit_bits) {
    if (order.n == 1 && digit_bits != 32)
        throw py::value_error("u64-order digit planes are 32 bits wide");
}

// a constant as a long double (x86: 64-bit mantissa)
static long double limbs_to_ld(const Limbs& a) {
    long double r = 0;
    for (int j = a.n - 1; j >= 0; --j) r = r * 18446744073709551616.0L + (long double)a.v.w[j];
    return r;
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
    // The sizes of one seed's first launch, and with them the batch rule.
    struct Plan {
        int wpd;          // keystream words per attempt: 1..10
        int apt;          // attempts per candidates thread (workgroups cover 256 * apt)
        double p;         // acceptance probability
        uint64_t n_att;   // attempts of the first launch
        uint64_t wgs;     // its candidate workgroups
        bool batchable;   // seeds may share a launch
    };

    // attempts == 0: size the launch for `remaining` elements at the
    // acceptance probability (+6 sigma). Seeds are expanded together only for
    // u64 and u128 orders and only while one seed's launch stays within the
    // single-workgroup scan (XHIP_K1_SCAN_ONE_WG candidate workgroups); this
    // is the one place that decides it.
    static Plan plan(const Limbs& order, int prng_nbytes, uint64_t remaining, uint64_t attempts) {
        Plan pl;
        const int L = order.n;
        pl.wpd = (prng_nbytes + 3) / 4;
        pl.apt = 16 / pl.wpd;
        const double order_d =
            L <= 2 ? double(order.v.w[1]) * 18446744073709551616.0 + double(order.v.w[0])
                   : double(limbs_to_ld(order));
        pl.p = order_d * std::pow(2.0, -8.0 * prng_nbytes);
        const double exp_att = double(remaining) / pl.p;
        pl.n_att = attempts ? attempts
                            : uint64_t(exp_att + 6.0 * std::sqrt(exp_att / pl.p) + 1024.0);
        // multi-limb orders accept as few as 1 draw in 200: cap the launch
        // so the workspace does not grow with 1/p, and loop
        if (L > 2 && pl.n_att > kMaxAttemptsPerLaunch) pl.n_att = kMaxAttemptsPerLaunch;
        pl.wgs = (pl.n_att + 256 * pl.apt - 1) / (256 * pl.apt);
        pl.batchable = L <= 2 && pl.wgs <= XHIP_K1_SCAN_ONE_WG;
        return pl;
    }

    static void check_nbytes(const Limbs& order, int prng_nbytes) {
        const int L = order.n;
        const int lo_bytes = L == 1 ? 1 : L == 2 ? 9 : 17, hi_bytes = L <= 2 ? 8 * L : 40;
        if (prng_nbytes < lo_bytes || prng_nbytes > hi_bytes || prng_nbytes > 8 * L)
            throw py::value_error(
                "prng_nbytes must be 1..8 for u64 orders, 9..16 for u128, 17..40 beyond");
    }

    // How many seeds one expand() call should carry for masks of `len`
    // elements: as many as keep the value rows and the candidate planes of a
    // batch within budget_bytes, at most XHIP_K1_MAX_BATCH, and 1 where the
    // batch rule (plan) says so.
    static uint64_t batch_size(uint64_t len, const std::string& order_dec, int prng_nbytes,
                               uint64_t budget_bytes) {
        const Limbs order = parse_limbs(order_dec);
        check_nbytes(order, prng_nbytes);
        if (len == 0) return 1;
        const Plan pl = plan(order, prng_nbytes, len, 0);
        if (!pl.batchable) return 1;
        const uint64_t per_seed = 8 * uint64_t(order.n) * (len + pl.wgs * 256 * pl.apt);
        uint64_t b = budget_bytes / per_seed;
        if (b > XHIP_K1_MAX_BATCH) b = XHIP_K1_MAX_BATCH;
        return b < 1 ? 1 : b;
    }

    // Expand S = seeds.size()/32 seeds; seed s fills out_lo/out_hi +
    // s*seed_stride with `len` mask values. Each seed's launch is sized for
    // the missing elements at the acceptance probability (or `attempts`, the
    // first time), runs candidates -> scan -> scatter, reads back the
    // accepted count, and repeats until `len` are filled. Seeds that may
    // share a launch (plan) take their first launch together: one copy of
    // keys and start words in, one copy of S accepted counts out; a seed that
    // falls short is finished by the single-seed loop from where the batch
    // left it. Returns the number of draw ATTEMPTS launched. That is NOT the
    // stream position of the len-th acceptance (the last launch overshoots);
    // a caller needing that position should account on the CPU. Masks are
    // always derived from a fresh seed, so the protocol never uses the tail
    // position.
    uint64_t expand(const std::string& seeds, uintptr_t out_lo_ptr, uintptr_t out_hi_ptr,
                    uint64_t len, const std::string& order_dec, int prng_nbytes,
                    const std::vector<uint64_t>& start_words, uint64_t seed_stride,
                    uint64_t attempts) {
        const Limbs order = parse_order(order_dec, out_hi_ptr);
        const uint64_t S = seeds.size() / 32;
        if (seeds.empty() || seeds.size() % 32) throw py::value_error("seed must be 32*S bytes");
        if (S > XHIP_K1_MAX_BATCH) throw py::value_error("at most 65535 seeds per call");
        if (start_words.size() != S) throw py::value_error("one start_word per seed");
        if (S > 1 && (seed_stride == 0 || seed_stride < len))
            throw py::value_error("several seeds need seed_stride, the u64 elements between "
                                  "their outputs (at least len)");
        check_nbytes(order, prng_nbytes);
        if (len == 0) return 0;
        uint64_t* out_lo = u64p(out_lo_ptr);
        uint64_t* out_hi = u64p(out_hi_ptr);

        // keys, then the start words, in one buffer and one copy
        std::vector<uint32_t> staging(10 * S);
        std::memcpy(staging.data(), seeds.data(), 32 * S);
        std::memcpy(staging.data() + 8 * S, start_words.data(), 8 * S);
        key_.reserve(10 * S, "alloc keys");
        check(hipMemcpy(key_.get(), staging.data(), 40 * S, hipMemcpyHostToDevice), "seed H2D");

        const Plan pl = plan(order, prng_nbytes, len, attempts);
        if (S == 1 || !pl.batchable) {
            uint64_t launched = 0;
            for (uint64_t s = 0; s < S; ++s)
                launched += finish(key_.get() + 8 * s, start_words[s], out_lo + s * seed_stride,
                                   out_hi ? out_hi + s * seed_stride : nullptr, len, order,
                                   prng_nbytes, 0, 0, attempts);
            return launched;
        }

        const uint64_t cand_stride = pl.wgs * 256 * pl.apt;
        const uint32_t counts_stride = uint32_t(pl.wgs);
        cand_lo_.reserve(S * cand_stride, "alloc cand");
        if (order.n == 2) cand_hi_.reserve(S * cand_stride, "alloc cand_hi");
        counts_.reserve(S * counts_stride, "alloc counts");
        total_.reserve(S, "alloc totals");
        check(xhip_k1_expand_batch(
                  key_.get(), reinterpret_cast<const uint64_t*>(key_.get() + 8 * S), uint32_t(S),
                  pl.n_att, pl.wpd, prng_nbytes, order.v.w[0], order.v.w[1], cand_lo_.get(),
                  order.n == 2 ? cand_hi_.get() : nullptr, cand_stride, counts_.get(),
                  counts_stride, total_.get(), pl.apt, out_lo, out_hi, seed_stride, len),
              "k1_expand_batch");
        std::vector<uint64_t> totals(S);
        check(hipMemcpy(totals.data(), total_.get(), 8 * S, hipMemcpyDeviceToHost),
              "totals D2H");
        uint64_t launched = S * pl.n_att;
        for (uint64_t s = 0; s < S; ++s) {
            if (totals[s] >= len) continue;
            launched += finish(key_.get() + 8 * s, start_words[s], out_lo + s * seed_stride,
                               out_hi ? out_hi + s * seed_stride : nullptr, len, order,
                               prng_nbytes, totals[s], pl.n_att, 0) -
                        pl.n_att;
        }
        return launched;
    }

  private:
    // The single-seed loop, from `filled` elements in place after `attempt`
    // attempts of the stream (0, 0 for a fresh seed): launch, read back the
    // accepted count, repeat until `len` are filled. first_attempts != 0
    // sizes the first launch. Returns the attempts launched, `attempt`
    // included.
    uint64_t finish(const uint32_t* key_dev, uint64_t start_word, uint64_t* out_lo,
                    uint64_t* out_hi, uint64_t len, const Limbs& order, int prng_nbytes,
                    uint64_t filled, uint64_t attempt, uint64_t first_attempts) {
        const int L = order.n;
        total_.reserve(1, "alloc total");
        while (filled < len) {
            const Plan pl = plan(order, prng_nbytes, len - filled, first_attempts);
            first_attempts = 0;
            const uint64_t n_att = pl.n_att;
            // accepted draws compact into per-workgroup segments of `cand`,
            // the last one cut at n_att; counts: one per workgroup
            uint64_t max_wgs = pl.wgs + 2;
            // candidate limb planes: one buffer each for lo and hi, or for
            // multi-limb orders L planes of n_att in the first
            cand_lo_.reserve(L > 2 ? L * n_att : n_att, "alloc cand");
            if (L == 2) cand_hi_.reserve(n_att, "alloc cand_hi");
            uint64_t* cand_hi = L > 2 ? cand_lo_.get() + n_att : cand_hi_.get();
            counts_.reserve(max_wgs, "alloc counts");
            scan_tmp_.reserve(max_wgs / 1024 + 2, "alloc scan tmp");

            uint32_t n_wgs = 0;
            check(xhip_k1_candidates_limbs(key_dev, start_word, attempt, n_att, pl.wpd,
                                           prng_nbytes, order.v, cand_lo_.get(), cand_hi,
                                           counts_.get(), pl.apt, &n_wgs),
                  "k1_candidates");
            check(xhip_k1_scan_hier(counts_.get(), n_wgs, scan_tmp_.get(), total_.get()),
                  "k1_scan");
            check(xhip_k1_scatter_compact_limbs(cand_lo_.get(), cand_hi, counts_.get(),
                                                total_.get(), n_wgs, pl.apt, filled, out_lo,
                                                out_hi, len, order.v),
                  "k1_scatter_compact");
            uint64_t round_accepted = 0;
            check(hipMemcpy(&round_accepted, total_.get(), 8, hipMemcpyDeviceToHost),
                  "total D2H");
            filled += round_accepted;  // may overshoot len; clamped below
            if (filled > len) filled = len;
            attempt += n_att;
            if (round_accepted == 0 && n_att > 0 && pl.p <= 0.0)
                throw std::runtime_error("expand: zero acceptance");
        }
        return attempt;
    }

    // 2^22 attempts: 160 MiB of candidate planes at five limbs
    static constexpr uint64_t kMaxAttemptsPerLaunch = uint64_t(1) << 22;

    DeviceBuffer<uint64_t> cand_lo_;  // u64 orders' only plane; every plane of multi-limb ones
    DeviceBuffer<uint64_t> cand_hi_;  // u128 orders only
    DeviceBuffer<uint32_t> counts_;   // accepted per candidates workgroup
    DeviceBuffer<uint32_t> scan_tmp_;
    DeviceBuffer<uint64_t> total_;    // accepted per seed of the launch
    DeviceBuffer<uint32_t> key_;      // S keys (8 words each), then S u64 start words
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
    // parse_order. exp_shift is a decimal string too (10^20 for f64 configs,
    // 10^45 for f32 Bmax).
    py::class_<MaskExpander>(m, "MaskExpander")
        .def(py::init<>())
        // seed: 32*S bytes; start_word: an int, or S of them
        .def(
            "expand",
            [](MaskExpander& self, const std::string& seed, uintptr_t out_lo, uintptr_t out_hi,
               uint64_t len, const std::string& order, int prng_nbytes, py::object start_word,
               uint64_t seed_stride, uint64_t attempts) {
                std::vector<uint64_t> words;
                if (py::isinstance<py::int_>(start_word))
                    words.push_back(start_word.cast<uint64_t>());
                else
                    words = start_word.cast<std::vector<uint64_t>>();
                py::gil_scoped_release release;
                return self.expand(seed, out_lo, out_hi, len, order, prng_nbytes, words,
                                   seed_stride, attempts);
            },
            py::arg("seed"), py::arg("out_lo"), py::arg("out_hi"), py::arg("len"),
            py::arg("order"), py::arg("prng_nbytes"), py::arg("start_word"), py::kw_only(),
            py::arg("seed_stride") = 0, py::arg("attempts") = 0)
        // private: the engine's batch size (the batch rule lives in plan())
        .def_static("_batch_size", &MaskExpander::batch_size, py::arg("len"), py::arg("order"),
                    py::arg("prng_nbytes"), py::arg("budget_bytes"));

    m.def(
        "aggregate_batch",
        [](uintptr_t acc, uintptr_t updates, uint64_t stride, uint32_t n_updates, uint64_t len,
           int bpn, int ept) {
            check(xhip_k3_aggregate(u64p(acc), u8p(updates), stride, n_updates, len, bpn, ept),
                  "k3_aggregate");
        },
        py::arg("acc"), py::arg("updates"), py::arg("stride"), py::arg("n_updates"),
        py::arg("len"), py::arg("bpn"), py::arg("ept") = 0, nogil);

    // private (tests, scripts/k3_sweep.py): the tile-streaming K3 plan (ept
    // 401 / 402) for a row of `len` elements, and a read-bandwidth probe
    m.def(
        "_k3_tile_plan",
        [](uint64_t len, int bpn, uint64_t stride) {
            XhipK3TilePlan p;
            xhip_k3_tile_plan(len, bpn, stride, &p);
            py::dict d;
            d["tile_elems"] = p.tile_elems;
            d["depth"] = p.depth;
            d["waves"] = p.waves;
            d["n_tiles"] = p.n_tiles;
            d["rem_start"] = p.rem_start;
            d["max_byte"] = p.max_byte;
            return d;
        },
        py::arg("len"), py::arg("bpn"), py::arg("stride"));

    // private (tests): what the loader-wave K3 kernel (ept 411 / 412) launches
    m.def(
        "_k3_loader_plan",
        [](uint64_t len, int bpn, uint64_t stride) {
            XhipK3LoaderPlan p;
            xhip_k3_loader_plan(len, bpn, stride, &p);
            py::dict d;
            d["consumers"] = p.consumers;
            d["depth"] = p.depth;
            d["tile_blocks"] = p.tile_blocks;
            d["has_remainder"] = bool(p.has_remainder);
            d["n_tiles"] = p.n_tiles;
            d["rem_start"] = p.rem_start;
            d["max_byte"] = p.max_byte;
            return d;
        },
        py::arg("len"), py::arg("bpn"), py::arg("stride"));

    m.def(
        "_read_ceiling",
        [](uintptr_t src, uint64_t bytes, bool nontemporal, uintptr_t sink) {
            check(xhip_read_ceiling(u8p(src), bytes, nontemporal,
                                    reinterpret_cast<uint32_t*>(sink)),
                  "read_ceiling");
        },
        py::arg("src"), py::arg("bytes"), py::arg("nontemporal"), py::arg("sink"), nogil);

    // private (ops/engine.py encode_model, tests): K7, the weights at `src`
    // (dtype 0=F32 1=F64 2=I32 3=I64) as their Option<Model> bincode body.
    // Returns the body's length in bytes. The body is written at out + 3 (its
    // words are then aligned) if out_bytes >= 3 + that length; a smaller
    // buffer is left untouched, and the caller calls again with a larger one.
    // The length is data-dependent (28..168 bytes per element), so it is read
    // back from the device, 8 bytes, between the count and the emit: sizing
    // `out` for the worst case instead would take 1.5x (F32) to 4x (F64) the
    // memory of a typical body. `work` holds _model_plan(len)["work_bytes"]
    // bytes. len == 0 launches nothing: the body is then the 9-byte head alone,
    // which the caller has without a device.
    m.def(
        "_model_encode",
        [](uintptr_t src, int dtype, uint64_t len, uintptr_t work, uintptr_t out,
           uint64_t out_bytes) -> uint64_t {
            if (dtype < 0 || dtype > 3) throw py::value_error("dtype must be 0..3");
            if (len > (uint64_t(1) << 32))
                throw py::value_error("a model has at most 2^32 weights");
            if (len == 0) return 9;
            py::gil_scoped_release release;
            void* w = reinterpret_cast<void*>(src);
            void* ws = reinterpret_cast<void*>(work);
            check(xhip_k7_model_count(w, dtype, len, ws), "k7_model_count");
            uint64_t words = 0;
            check(hipMemcpy(&words, ws, sizeof words, hipMemcpyDeviceToHost), "k7 total");
            const uint64_t body = 9 + 4 * words;
            if (out_bytes >= 3 + body)
                check(xhip_k7_model_emit(w, dtype, len, ws, u8p(out), out_bytes),
                      "k7_model_emit");
            return body;
        },
        py::arg("src"), py::arg("dtype"), py::arg("len"), py::arg("work"), py::arg("out"),
        py::arg("out_bytes"));

    // private: how _model_encode splits `len` weights (XhipK7Plan, kernels.h)
    m.def(
        "_model_plan",
        [](uint64_t len) {
            XhipK7Plan p;
            xhip_k7_plan(len, &p);
            py::dict d;
            d["block_elems"] = p.block_elems;
            d["blocks"] = p.blocks;
            d["scan_levels"] = p.scan_levels;
            d["tile_blocks"] = p.tile_blocks;
            d["tiles"] = p.tiles;
            d["work_bytes"] = p.work_bytes;
            return d;
        },
        py::arg("len"));

    // private (ops/engine.py decode_model, tests): K7d, the Option<Model>
    // body of `nbytes` bytes at device address `body` (3 bytes past a 4-byte
    // boundary of its buffer, where _model_encode leaves one) into `len`
    // weights of dtype 0..3 at `out`. Returns 0 for "decoded" and non-zero for
    // "rejected": the body is not head 01, u64 len, len canonical elements of
    // the dtype and nothing after; `out` is then unspecified. `work` holds
    // _model_decode_plan((nbytes - 9) / 4, tile_blocks)["work_bytes"] bytes.
    // One status word is read back after the last kernel.
    m.def(
        "_model_decode",
        [](uintptr_t body, uint64_t nbytes, int dtype, uint64_t len, uintptr_t work,
           uintptr_t out, uint32_t tile_blocks) -> uint32_t {
            if (dtype < 0 || dtype > 3) throw py::value_error("dtype must be 0..3");
            if (tile_blocks > XHIP_K7D_TILE_BLOCKS)
                throw py::value_error("tile_blocks is at most " +
                                      std::to_string(XHIP_K7D_TILE_BLOCKS));
            py::gil_scoped_release release;
            uint32_t rejected = 1;
            check(xhip_k7d_decode(reinterpret_cast<const void*>(body), nbytes, dtype, len,
                                  reinterpret_cast<void*>(work), reinterpret_cast<void*>(out),
                                  tile_blocks, &rejected),
                  "k7d_decode");
            return rejected;
        },
        py::arg("body"), py::arg("nbytes"), py::arg("dtype"), py::arg("len"), py::arg("work"),
        py::arg("out"), py::arg("tile_blocks") = 0);

    // private: how _model_decode splits `words` element words (XhipK7dPlan)
    m.def(
        "_model_decode_plan",
        [](uint64_t words, uint32_t tile_blocks) {
            XhipK7dPlan p;
            xhip_k7d_plan(words, tile_blocks, &p);
            py::dict d;
            d["block_words"] = p.block_words;
            d["blocks"] = p.blocks;
            d["tile_blocks"] = p.tile_blocks;
            d["tiles"] = p.tiles;
            d["levels"] = p.levels;
            d["work_bytes"] = p.work_bytes;
            return d;
        },
        py::arg("words"), py::arg("tile_blocks") = 0);

    // [n_planes][len] digit planes minus the mask -> model weights.
    // dtype follows mask::DataType: 0=F32 1=F64 2=I32 3=I64
    // Bmax configs, and integer outputs of the other bounds, pass `offset` =
    // nb * add_shift * exp_shift as a decimal string: the shift is then
    // subtracted in integers (n_add_shift is unused), and `divisor`, where
    // exp_shift * scalar_sum is an exact integer below 2^64, makes integer
    // outputs the exact truncated quotient. A float dtype given offset and
    // divisor (any size that fits the order's limbs) runs in exact mode: the
    // rational (t - offset) / divisor rounded once to the output type.
    m.def(
        "unmask",
        [](uintptr_t planes, uintptr_t mask_lo, uintptr_t mask_hi, uintptr_t out, uint64_t len,
           int n_planes, const std::string& order, const std::string& exp_shift,
           double n_add_shift, double scalar_sum, int dtype, int digit_bits,
           const std::string& offset, const std::string& divisor) {
            Limbs o = parse_order(order, mask_hi), e = parse_limbs(exp_shift);
            Limbs off = parse_optional(offset), div = parse_optional(divisor);
            check_digit_bits(o, digit_bits);
            if (off.is_zero()) {
                if (o.n > 2)
                    throw py::value_error("orders >= 2^128 are Bmax configs: unmask needs "
                                          "their exact offset");
                if (e.n > 2) throw py::value_error("exp_shift >= 2^128 needs the exact offset");
                if (!div.is_zero()) throw py::value_error("divisor goes with an offset");
            } else if (off.n > o.n) {
                throw py::value_error("the exact offset must be below the order");
            }
            const bool is_float = dtype == 0 || dtype == 1;
            if (is_float ? div.n > o.n : div.n > 1)
                throw py::value_error(is_float ? "the exact divisor must fit the order's limbs"
                                               : "divisor must be below 2^64");
            // 1 / (exp_shift * scalar_sum), rounded to a double once
            const double scale = double(1.0L / (limbs_to_ld(e) * (long double)scalar_sum));
            check(xhip_k4_unmask_limbs(u64p(planes), u64p(mask_lo), u64p(mask_hi), dtype,
                                       reinterpret_cast<void*>(out), len, n_planes, digit_bits,
                                       o.v, e.v, n_add_shift, scalar_sum, off.v, div.v, scale),
                  "k4_unmask");
        },
        py::arg("planes"), py::arg("mask_lo"), py::arg("mask_hi"), py::arg("out"),
        py::arg("len"), py::arg("n_planes"), py::arg("order"), py::arg("exp_shift"),
        py::arg("n_add_shift"), py::arg("scalar_sum"), py::arg("dtype") = 0,
        py::arg("digit_bits") = 32, py::arg("offset") = "", py::arg("divisor") = "", nogil);

    // u64 orders only: `vals` are plain u64 (cross-rank sums of) canonical
    // values. `offset` and `divisor` as for unmask: integer outputs, and float
    // outputs in exact mode (both given).
    m.def(
        "unmask_values",
        [](uintptr_t vals, uintptr_t mask_lo, uintptr_t mask_hi, uintptr_t out, uint64_t len,
           const std::string& order, const std::string& exp_shift, double n_add_shift,
           double scalar_sum, int dtype, const std::string& offset,
           const std::string& divisor) {
            Limbs o = parse_order(order, mask_hi), e = parse_limbs(exp_shift);
            Limbs off = parse_optional(offset), div = parse_optional(divisor);
            if (o.n > 1 || e.n > 1) throw py::value_error("unmask_values covers u64 orders");
            if (off.n > 1 || div.n > 1)
                throw py::value_error("offset and divisor must be below 2^64");
            if (off.is_zero() && !div.is_zero())
                throw py::value_error("divisor goes with an offset");
            check(xhip_k4_unmask_values(u64p(vals), u64p(mask_lo), dtype,
                                        reinterpret_cast<void*>(out), len, o.v.w[0], e.v.w[0],
                                        n_add_shift, scalar_sum, off.v.w[0], div.v.w[0]),
                  "k4_unmask_values");
        },
        py::arg("vals"), py::arg("mask_lo"), py::arg("mask_hi"), py::arg("out"), py::arg("len"),
        py::arg("order"), py::arg("exp_shift"), py::arg("n_add_shift"), py::arg("scalar_sum"),
        py::arg("dtype") = 0, py::arg("offset") = "", py::arg("divisor") = "", nogil);

    // [n_planes][len] digit planes -> canonical values mod order
    m.def(
        "canonicalize",
        [](uintptr_t planes, uintptr_t out_lo, uintptr_t out_hi, uint64_t len, int n_planes,
           const std::string& order, int digit_bits) {
            Limbs o = parse_order(order, out_hi);
            check_digit_bits(o, digit_bits);
            check(xhip_k2_canonicalize_limbs(u64p(planes), u64p(out_lo), u64p(out_hi), len,
                                             n_planes, digit_bits, o.v),
                  "k2_canonicalize");
        },
        py::arg("planes"), py::arg("out_lo"), py::arg("out_hi"), py::arg("len"),
        py::arg("n_planes"), py::arg("order"), py::arg("digit_bits") = 32, nogil);

    // canonical values -> add into [n_planes][len] planes of digit_bits-wide
    // digits; `rows` value vectors, row_stride u64 elements apart, in one call
    m.def(
        "add_to_planes",
        [](uintptr_t planes, uintptr_t lo, uintptr_t hi, uint64_t len, int n_planes,
           const std::string& order, int digit_bits, uint32_t rows, uint64_t row_stride) {
            Limbs o = parse_order(order, hi);
            check_digit_bits(o, digit_bits);
            if (rows < 1 || rows > XHIP_K1_MAX_BATCH)
                throw py::value_error("rows must be in 1..65535");
            if (rows > 1 && (row_stride == 0 || row_stride < len))
                throw py::value_error("several rows need row_stride, the u64 elements between "
                                      "them (at least len)");
            check(xhip_add_rows_to_planes_limbs(u64p(planes), u64p(lo), u64p(hi), len, n_planes,
                                                digit_bits, o.v, rows, row_stride),
                  "add_to_planes");
        },
        py::arg("planes"), py::arg("lo"), py::arg("hi"), py::arg("len"), py::arg("n_planes"),
        py::arg("order"), py::arg("digit_bits") = 32, py::kw_only(), py::arg("rows") = 1,
        py::arg("row_stride") = 0, nogil);

    // wide orders only: 32-bit accumulator planes -> k compact planes of the
    // value mod order
    m.def(
        "recode_planes",
        [](uintptr_t acc, uintptr_t out, uint64_t len, int n_digits, const std::string& order,
           int k, int digit_bits) {
            Limbs o = parse_limbs(order);
            if (o.n == 1) throw py::value_error("recode_planes covers wide (>= 2^64) orders");
            check(xhip_k2_recode_planes_limbs(u64p(acc), u64p(out), len, n_digits, o.v, k,
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
            Limbs o = parse_order(order, a_hi);
            parse_order(order, b_hi);
            check(xhip_k2_mod_add_limbs(u64p(a_lo), u64p(a_hi), u64p(b_lo), u64p(b_hi), len,
                                        o.v),
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
            Limbs o = parse_order(order, mask_hi), e = parse_limbs(exp_shift);
            if (o.n > 2 || e.n > 2)
                throw py::value_error("synthetic update rows cover orders up to 2^128");
            check(xhip_k5_mask_pack(u64p(mask_lo), u64p(mask_hi), u8p(out), len, bpn, o.v.w[0],
                                    o.v.w[1], participant, scalar, add_shift, e.v.w[0],
                                    e.v.w[1]),
                  "k5_mask_pack");
        },
        py::arg("mask_lo"), py::arg("mask_hi"), py::arg("out"), py::arg("len"), py::arg("bpn"),
        py::arg("order"), py::arg("participant"), py::arg("scalar"), py::arg("add_shift"),
        py::arg("exp_shift"), nogil);

    // real weights (dtype as for unmask): quantize, add the mask, pack. Bmax
    // configs pass `offset` = add_shift * exp_shift as a decimal string, which
    // is then added in integers.
    // scalar_den != 0 selects the exact kernel for every width: the scalar is
    // the fraction scalar_num / scalar_den (both below 2^63), add_shift must
    // be an integer, and `scalar` and `offset` are not used.
    m.def(
        "mask_weights",
        [](uintptr_t w, int dtype, uintptr_t mask_lo, uintptr_t mask_hi, uintptr_t out,
           uint64_t len, int bpn, const std::string& order, double scalar, double add_shift,
           const std::string& exp_shift, const std::string& offset, const py::int_& scalar_num,
           const py::int_& scalar_den) {
            const py::int_ zero(0), top = py::int_(1).attr("__lshift__")(63);
            for (const py::int_& x : {scalar_num, scalar_den})
                if (x < zero || x >= top)
                    throw py::value_error("mask_weights: scalar_num and scalar_den must be "
                                          "in [0, 2^63)");
            const uint64_t p = scalar_num.cast<uint64_t>(), q = scalar_den.cast<uint64_t>();
            if (p != 0 && q == 0)
                throw py::value_error("mask_weights: scalar_num goes with scalar_den");
            Limbs a{{{0, 0, 0, 0, 0}}, 1};
            if (q != 0 && !integral_limbs(add_shift, a))
                throw py::value_error("mask_weights: the exact kernel needs an integral "
                                      "add_shift in [1, 2^320)");
            py::gil_scoped_release release;
            Limbs o = parse_order(order, mask_hi), e = parse_limbs(exp_shift);
            if (q != 0) {
                check(xhip_k5_mask_weights_exact_limbs(reinterpret_cast<const void*>(w), dtype,
                                                       u64p(mask_lo), u64p(mask_hi), u8p(out),
                                                       len, bpn, o.v, a.v, e.v, p, q),
                      "k5_mask_weights_exact");
                return;
            }
            Limbs off = parse_optional(offset);
            if (off.is_zero() ? (o.n > 2 || e.n > 2) : (o.n < 2 || off.n > o.n || e.n > o.n))
                throw py::value_error(
                    "mask_weights: orders >= 2^128 (Bmax) need offset = add_shift * exp_shift, "
                    "below the order");
            check(xhip_k5_mask_weights_limbs(reinterpret_cast<const void*>(w), dtype,
                                             u64p(mask_lo), u64p(mask_hi), u8p(out), len, bpn,
                                             o.v, scalar, add_shift, e.v, off.v),
                  "k5_mask_weights");
        },
        py::arg("w"), py::arg("dtype"), py::arg("mask_lo"), py::arg("mask_hi"), py::arg("out"),
        py::arg("len"), py::arg("bpn"), py::arg("order"), py::arg("scalar"),
        py::arg("add_shift"), py::arg("exp_shift"), py::arg("offset") = "",
        py::arg("scalar_num") = py::int_(0), py::arg("scalar_den") = py::int_(0));

    // canonical values <-> packed wire limbs of bpn bytes
    m.def(
        "pack",
        [](uintptr_t in_lo, uintptr_t in_hi, uintptr_t out, uint64_t len, int bpn,
           const std::string& order) {
            Limbs o = parse_order(order, in_hi);
            check(xhip_k6_pack_limbs(u64p(in_lo), u64p(in_hi), u8p(out), len, bpn, o.v),
                  "k6_pack");
        },
        py::arg("in_lo"), py::arg("in_hi"), py::arg("out"), py::arg("len"), py::arg("bpn"),
        py::arg("order"), nogil);
    m.def(
        "unpack",
        [](uintptr_t in, uintptr_t out_lo, uintptr_t out_hi, uint64_t len, int bpn,
           const std::string& order) {
            Limbs o = parse_order(order, out_hi);
            check(xhip_k6_unpack_limbs(u8p(in), u64p(out_lo), u64p(out_hi), len, bpn, o.v),
                  "k6_unpack");
        },
        py::arg("packed"), py::arg("out_lo"), py::arg("out_hi"), py::arg("len"), py::arg("bpn"),
        py::arg("order"), nogil);
}
