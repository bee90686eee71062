// Bindings for mask config / masking / aggregation (CPU oracle path).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "gpu/mask_quant.h"
#include "gpu/u192.h"
#include "gpu/unmask_round.h"
#include "mask/masking.h"

namespace py = pybind11;
using namespace xaynet;
using namespace xaynet::mask;

static MaskConfig cfg_from_ints(int g, int d, int b, int m) {
    uint8_t raw[4] = {uint8_t(g), uint8_t(d), uint8_t(b), uint8_t(m)};
    auto c = MaskConfig::from_bytes(raw);
    if (!c) throw std::runtime_error("invalid mask config");
    return *c;
}

// ---- quantize_exact: the GPU's exact quantiser (gpu/mask_quant.h) on the host

static bool to_limbs(const BigUint& v, xhip_limbs& out) {
    if (v.bits() > 64 * ML_MAX_LIMBS) return false;
    uint8_t raw[8 * ML_MAX_LIMBS];
    v.to_bytes_le_fixed(raw, sizeof raw);
    for (int j = 0; j < ML_MAX_LIMBS; ++j) {
        out.w[j] = 0;
        for (int b = 7; b >= 0; --b) out.w[j] = (out.w[j] << 8) | raw[8 * j + b];
    }
    return true;
}

template <typename T, int L>
static py::list quantize_exact_as(const T* w, size_t n, const mq_params& params) {
    py::list out;
    for (size_t i = 0; i < n; ++i) {
        const limbs<L> v = mq_quantize<L>(mq_decompose(w[i]), params);
        out.append(BigUint::from_bytes_le(reinterpret_cast<const uint8_t*>(v.w), 8 * L).to_dec());
    }
    return out;
}

template <typename T>
static py::list quantize_exact_typed(const py::array& weights, int L, const mq_params& params) {
    auto a = py::array_t<T, py::array::c_style>::ensure(weights);
    if (!a || a.ndim() != 1) throw py::value_error("weights must be a 1-D array");
    const size_t n = size_t(a.shape(0));
    switch (L) {
        case 1: return quantize_exact_as<T, 1>(a.data(), n, params);
        case 2: return quantize_exact_as<T, 2>(a.data(), n, params);
        case 3: return quantize_exact_as<T, 3>(a.data(), n, params);
        case 4: return quantize_exact_as<T, 4>(a.data(), n, params);
        default: return quantize_exact_as<T, 5>(a.data(), n, params);
    }
}

// trunc((clamp(num/den * w) + add_shift) * exp_shift) per element of `weights`
// (taken as typed: f32, f64, i32 or i64), as decimal strings. num/den is the
// scalar already clamped to the unit config's bound.
static py::list quantize_exact(const py::array& weights, const MaskConfig& cfg,
                               const py::int_& num, const py::int_& den) {
    const py::int_ zero(0), top = py::int_(1).attr("__lshift__")(63);
    if (num < zero || num >= top || den <= zero || den >= top)
        throw py::value_error("quantize_exact: num in [0, 2^63) and den in [1, 2^63)");
    const CfgInfo& ci = cfg.info();
    const BigInt a_t = ci.add_shift.trunc();
    xhip_limbs order, a, e;
    mq_params params;
    const int L = int((ci.order.bits() + 63) / 64);
    if (a_t.neg || Rational::cmp(ci.add_shift, Rational::from_integer(a_t)) != 0 ||
        !to_limbs(ci.order, order) || !to_limbs(a_t.mag, a) || !to_limbs(ci.exp_shift, e) ||
        !mq_prepare(order, L, a, e, num.cast<uint64_t>(), den.cast<uint64_t>(), params))
        throw py::value_error("quantize_exact: config outside the exact quantiser (integral "
                              "add_shift, order below 2^320)");
    const int tn = weights.dtype().num();  // by type number, not identity
    if (tn == py::dtype::of<float>().num()) return quantize_exact_typed<float>(weights, L, params);
    if (tn == py::dtype::of<double>().num())
        return quantize_exact_typed<double>(weights, L, params);
    if (tn == py::dtype::of<int32_t>().num())
        return quantize_exact_typed<int32_t>(weights, L, params);
    if (tn == py::dtype::of<int64_t>().num())
        return quantize_exact_typed<int64_t>(weights, L, params);
    throw py::value_error("quantize_exact: weights dtype must be f32/f64/i32/i64");
}

// ---- planes_mod: the finalize kernels' plane recombination and reduction
// (gpu/limbs.h, gpu/u192.h) on the host

static py::object int_from_limbs(const uint64_t* w, int n) {
    const py::object from_bytes = py::module_::import("builtins").attr("int").attr("from_bytes");
    uint8_t raw[8 * ML_MAX_LIMBS];
    for (int j = 0; j < n; ++j)
        for (int b = 0; b < 8; ++b) raw[8 * j + b] = uint8_t(w[j] >> (8 * b));
    return from_bytes(py::bytes(reinterpret_cast<const char*>(raw), size_t(8 * n)), "little");
}

template <int L>
static py::list planes_mod_ml(const uint64_t* planes, uint64_t n, int k, int digit_bits,
                              const xhip_limbs& order) {
    py::list out;
    for (uint64_t i = 0; i < n; ++i) {
        const limbs<L> r =
            ml_mod<L>(ml_from_planes<L + 1>(planes, n, i, k, digit_bits), ml_from<L>(order));
        out.append(int_from_limbs(r.w, L));
    }
    return out;
}

template <int DB>
static py::list planes_mod_u192(const uint64_t* planes, uint64_t n, int k, int digit_bits,
                                const xhip_limbs& order) {
    const unsigned __int128 o = ((unsigned __int128)order.w[1] << 64) | order.w[0];
    py::list out;
    for (uint64_t i = 0; i < n; ++i) {
        const unsigned __int128 r =
            u192_mod_u128(u192_from_planes<DB>(planes, n, i, k, digit_bits), o);
        const uint64_t w[2] = {uint64_t(r), uint64_t(r >> 64)};
        out.append(int_from_limbs(w, 2));
    }
    return out;
}

// sum_d planes[d][i] << (digit_bits * d) mod order for every column i of a
// uint64 [k, n] array. path "ml": ml_mod<L>(ml_from_planes<L + 1>) at the
// order's limb count L = 1..5, the arithmetic of the *_ml kernels and of
// k4_unmask_offset; path "u192": u192_mod_u128(u192_from_planes<32 or 0>),
// the *_u128 kernels (L = 2 only; digit_bits 32 takes the compile-time
// shift). `runtime_shift` forces <0> at 32 bits too. The plane shape must lie
// inside the window the launchers check: (k - 1) * digit_bits + 64 <=
// 64 * (L + 1) - 1.
static py::list planes_mod(const py::array& planes, const py::int_& order, int digit_bits,
                           const std::string& path, bool runtime_shift) {
    auto a = py::array_t<uint64_t, py::array::c_style>::ensure(planes);
    if (!a || a.ndim() != 2 || !planes.dtype().is(py::dtype::of<uint64_t>()))
        throw py::value_error("planes_mod: planes must be a uint64 [k, n] array");
    const int k = int(a.shape(0));
    const uint64_t n = uint64_t(a.shape(1));
    const int bits = order.attr("bit_length")().cast<int>();
    if (order < py::int_(1) || bits > 64 * ML_MAX_LIMBS)
        throw py::value_error("planes_mod: order in [1, 2^320)");
    const int L = (bits + 63) / 64;
    if (k < 1 || digit_bits < 1 || digit_bits > 63 ||
        int64_t(k - 1) * digit_bits + 64 > 64 * (L + 1) - 1)
        throw py::value_error("planes_mod: plane shape outside the reduction window");
    xhip_limbs o;
    const std::string raw = order.attr("to_bytes")(8 * ML_MAX_LIMBS, "little").cast<std::string>();
    for (int j = 0; j < ML_MAX_LIMBS; ++j) {
        o.w[j] = 0;
        for (int b = 7; b >= 0; --b) o.w[j] = (o.w[j] << 8) | uint8_t(raw[8 * j + b]);
    }
    if (path == "u192") {
        if (L != 2) throw py::value_error("planes_mod: the u192 path covers two-limb orders");
        return digit_bits == 32 && !runtime_shift
                   ? planes_mod_u192<32>(a.data(), n, k, digit_bits, o)
                   : planes_mod_u192<0>(a.data(), n, k, digit_bits, o);
    }
    if (path != "ml") throw py::value_error("planes_mod: path is \"ml\" or \"u192\"");
    switch (L) {
        case 1: return planes_mod_ml<1>(a.data(), n, k, digit_bits, o);
        case 2: return planes_mod_ml<2>(a.data(), n, k, digit_bits, o);
        case 3: return planes_mod_ml<3>(a.data(), n, k, digit_bits, o);
        case 4: return planes_mod_ml<4>(a.data(), n, k, digit_bits, o);
        default: return planes_mod_ml<5>(a.data(), n, k, digit_bits, o);
    }
}

// ---- unmask_round: the exact float unmask's element function
// (gpu/unmask_round.h) on the host

static bool int_to_limbs(const py::int_& v, xhip_limbs& out) {
    if (v < py::int_(0) || v.attr("bit_length")().cast<int>() > 64 * ML_MAX_LIMBS) return false;
    const std::string raw = v.attr("to_bytes")(8 * ML_MAX_LIMBS, "little").cast<std::string>();
    for (int j = 0; j < ML_MAX_LIMBS; ++j) {
        out.w[j] = 0;
        for (int b = 7; b >= 0; --b) out.w[j] = (out.w[j] << 8) | uint8_t(raw[8 * j + b]);
    }
    return true;
}

template <typename F, int L>
static py::array unmask_round_as(const std::vector<xhip_limbs>& mags,
                                 const std::vector<bool>& negs, const xhip_limbs& q) {
    py::array_t<F> out(py::ssize_t(mags.size()));
    F* o = out.mutable_data();
    for (size_t i = 0; i < mags.size(); ++i)
        o[i] = ur_round<F, L>(negs[i], ml_from<L>(mags[i]), ml_from<L>(q));
    return out;
}

template <typename F>
static py::array unmask_round_typed(int L, const std::vector<xhip_limbs>& mags,
                                    const std::vector<bool>& negs, const xhip_limbs& q) {
    switch (L) {
        case 1: return unmask_round_as<F, 1>(mags, negs, q);
        case 2: return unmask_round_as<F, 2>(mags, negs, q);
        case 3: return unmask_round_as<F, 3>(mags, negs, q);
        case 4: return unmask_round_as<F, 4>(mags, negs, q);
        default: return unmask_round_as<F, 5>(mags, negs, q);
    }
}

// The float (dtype 0: f32, 1: f64) nearest to mags[i] / q, ties to even,
// negative where negs[i], as a numpy array: ur_round<F, L> at `limbs` = L
// limbs, by default the fewest that hold q and every magnitude.
static py::array unmask_round(const py::sequence& mags, const py::sequence& negs,
                              const py::int_& q, int dtype, int n_limbs) {
    if (dtype != 0 && dtype != 1) throw py::value_error("unmask_round: dtype is 0 (f32) or 1 (f64)");
    if (py::len(mags) != py::len(negs))
        throw py::value_error("unmask_round: one sign per magnitude");
    xhip_limbs qv;
    if (q <= py::int_(0) || !int_to_limbs(q, qv))
        throw py::value_error("unmask_round: q in [1, 2^320)");
    std::vector<xhip_limbs> mv(py::len(mags));
    std::vector<bool> nv(mv.size());
    int need = 1;
    for (int j = 1; j < ML_MAX_LIMBS; ++j)
        if (qv.w[j]) need = j + 1;
    for (size_t i = 0; i < mv.size(); ++i) {
        if (!int_to_limbs(py::int_(mags[i]), mv[i]))
            throw py::value_error("unmask_round: magnitudes in [0, 2^320)");
        for (int j = need; j < ML_MAX_LIMBS; ++j)
            if (mv[i].w[j]) need = j + 1;
        nv[i] = py::cast<bool>(negs[i]);
    }
    if (n_limbs == 0) n_limbs = need;
    if (n_limbs < need || n_limbs > ML_MAX_LIMBS)
        throw py::value_error("unmask_round: limbs must hold q and every magnitude (at most 5)");
    return dtype == 0 ? unmask_round_typed<float>(n_limbs, mv, nv, qv)
                      : unmask_round_typed<double>(n_limbs, mv, nv, qv);
}

void bind_mask(py::module_& m) {
    auto mm = m.def_submodule("mask");
    mm.def("unmask_round", &unmask_round, py::arg("mags"), py::arg("negs"), py::arg("q"),
           py::arg("dtype"), py::arg("limbs") = 0);
    mm.def("planes_mod", &planes_mod, py::arg("planes"), py::arg("order"), py::arg("digit_bits"),
           py::arg("path") = "ml", py::arg("runtime_shift") = false);
    mm.def("quantize_exact", &quantize_exact, py::arg("weights"), py::arg("cfg"), py::arg("num"),
           py::arg("den"));

    py::class_<MaskConfig>(mm, "MaskConfig")
        .def(py::init([](int g, int d, int b, int mo) { return cfg_from_ints(g, d, b, mo); }),
             py::arg("group"), py::arg("dtype"), py::arg("bound"), py::arg("model"))
        .def_property_readonly("group", [](const MaskConfig& c) { return int(c.group); })
        .def_property_readonly("dtype", [](const MaskConfig& c) { return int(c.dtype); })
        .def_property_readonly("bound", [](const MaskConfig& c) { return int(c.bound); })
        .def_property_readonly("model", [](const MaskConfig& c) { return int(c.model); })
        .def_property_readonly("bytes_per_number",
                               [](const MaskConfig& c) { return c.info().bpn; })
        .def_property_readonly("prng_nbytes", [](const MaskConfig& c) { return c.info().prng_nbytes; })
        .def_property_readonly("order", [](const MaskConfig& c) { return c.info().order.to_dec(); })
        .def_property_readonly("order_fits_u64",
                               [](const MaskConfig& c) { return c.info().order_fits_u64; })
        .def_property_readonly("max_nb_models",
                               [](const MaskConfig& c) { return c.info().max_nb_models; })
        .def("__eq__", [](const MaskConfig& a, const MaskConfig& b) { return a == b; })
        .def("to_bytes", [](const MaskConfig& c) {
            uint8_t raw[4];
            c.write_bytes(raw);
            return py::bytes(reinterpret_cast<char*>(raw), 4);
        })
        .def_static("from_bytes", [](py::bytes b) {
            std::string s = b;
            if (s.size() != 4) throw std::runtime_error("config must be 4 bytes");
            auto c = MaskConfig::from_bytes(reinterpret_cast<const uint8_t*>(s.data()));
            if (!c) throw std::runtime_error("invalid mask config bytes");
            return *c;
        });

    py::class_<MaskConfigPair>(mm, "MaskConfigPair")
        .def(py::init([](const MaskConfig& v, const MaskConfig& u) {
                 return MaskConfigPair{v, u};
             }),
             py::arg("vect"), py::arg("unit"))
        .def_readonly("vect", &MaskConfigPair::vect)
        .def_readonly("unit", &MaskConfigPair::unit)
        .def("__eq__", [](const MaskConfigPair& a, const MaskConfigPair& b) { return a == b; });

    py::class_<MaskObject>(mm, "MaskObject")
        .def_property_readonly("count", [](const MaskObject& o) { return o.vect.count; })
        .def_property_readonly("config", [](const MaskObject& o) { return o.config(); })
        .def("is_valid", &MaskObject::is_valid)
        .def("serialize", [](const MaskObject& o) {
            Bytes b = o.serialize();
            return py::bytes(reinterpret_cast<char*>(b.data()), b.size());
        })
        .def_static("deserialize", [](py::bytes data) {
            std::string s = data;
            auto o = MaskObject::deserialize(reinterpret_cast<const uint8_t*>(s.data()), s.size(),
                                             nullptr);
            if (!o) throw std::runtime_error("invalid mask object bytes");
            return *o;
        })
        .def("element", [](const MaskObject& o, size_t i) { return o.vect.element(i).to_dec(); })
        .def_property_readonly("unit_value", [](const MaskObject& o) { return o.unit.value().to_dec(); })
        .def_property_readonly("vect_bytes", [](const MaskObject& o) {
            return py::bytes(reinterpret_cast<const char*>(o.vect.data.data()),
                             o.vect.data.size());
        });

    py::class_<Scalar>(mm, "Scalar")
        .def(py::init<uint64_t, uint64_t>(), py::arg("numer"), py::arg("denom"))
        .def_static("unit", []() { return Scalar(); });

    // The unit (scalar) draw that precedes the vector draws in the mask
    // stream: returns (value_dec, keystream_words_consumed). The GPU K1
    // expander starts its vector draws at that word offset.
    mm.def("unit_draw", [](py::bytes seed, const MaskConfig& cfg) {
        std::string s = seed;
        if (s.size() != 32) throw std::runtime_error("seed must be 32 bytes");
        MaskPrng prng(reinterpret_cast<const uint8_t*>(s.data()));
        BigUint v = prng.generate_integer(cfg.info());
        return py::make_tuple(v.to_dec(), prng.words_consumed());
    });

    mm.def("derive_mask", [](py::bytes seed, size_t len, const MaskConfigPair& cfg) {
        std::string s = seed;
        if (s.size() != 32) throw std::runtime_error("seed must be 32 bytes");
        return derive_mask(reinterpret_cast<const uint8_t*>(s.data()), len, cfg);
    });

    // exact-rational oracle path (bypasses the fast typed masker; used by
    // tests to assert bit-equality of the fast path)
    mm.def("mask_model_oracle", [](py::bytes seed, const Scalar& scalar, py::array weights,
                                   const MaskConfigPair& cfg) {
        std::string s = seed;
        if (s.size() != 32) throw std::runtime_error("seed must be 32 bytes");
        const uint8_t* sp = reinterpret_cast<const uint8_t*>(s.data());
        auto buf = weights.request();
        if (buf.ndim != 1) throw std::runtime_error("weights must be 1-D");
        size_t n = size_t(buf.shape[0]);
        RationalModel m;
        switch (cfg.vect.dtype) {
            case DataType::F32:
                m = model_from_f32(weights.cast<py::array_t<float>>().data(), n);
                break;
            case DataType::F64:
                m = model_from_f64(weights.cast<py::array_t<double>>().data(), n);
                break;
            case DataType::I32:
                m = model_from_i32(weights.cast<py::array_t<int32_t>>().data(), n);
                break;
            case DataType::I64:
                m = model_from_i64(weights.cast<py::array_t<int64_t>>().data(), n);
                break;
        }
        return mask_model(sp, scalar, m, cfg);
    });

    mm.def("mask_model", [](py::bytes seed, const Scalar& scalar, py::array weights,
                            const MaskConfigPair& cfg) {
        std::string s = seed;
        if (s.size() != 32) throw std::runtime_error("seed must be 32 bytes");
        const uint8_t* sp = reinterpret_cast<const uint8_t*>(s.data());
        auto buf = weights.request();
        if (buf.ndim != 1) throw std::runtime_error("weights must be 1-D");
        size_t n = size_t(buf.shape[0]);
        switch (cfg.vect.dtype) {
            case DataType::F32: {
                auto a = weights.cast<py::array_t<float>>();
                return mask_f32(sp, scalar, a.data(), n, cfg);
            }
            case DataType::F64: {
                auto a = weights.cast<py::array_t<double>>();
                return mask_f64(sp, scalar, a.data(), n, cfg);
            }
            case DataType::I32: {
                auto a = weights.cast<py::array_t<int32_t>>();
                return mask_i32(sp, scalar, a.data(), n, cfg);
            }
            case DataType::I64: {
                auto a = weights.cast<py::array_t<int64_t>>();
                return mask_i64(sp, scalar, a.data(), n, cfg);
            }
        }
        throw std::runtime_error("unreachable");
    });

    py::class_<Aggregation>(mm, "Aggregation")
        .def(py::init<const MaskConfigPair&, size_t>(), py::arg("config"), py::arg("object_size"))
        .def_property_readonly("nb_models", &Aggregation::nb_models)
        .def_property_readonly("object", &Aggregation::object)
        .def("validate_aggregation",
             [](const Aggregation& a, const MaskObject& o) {
                 return int(a.validate_aggregation(o));
             })
        .def("aggregate", &Aggregation::aggregate)
        .def("validate_unmasking",
             [](const Aggregation& a, const MaskObject& o) { return int(a.validate_unmasking(o)); })
        .def("set", &Aggregation::set, py::arg("object"), py::arg("nb_models"))
        // tests: the unmasked model as the exact rationals themselves, one
        // (numerator, denominator) pair of decimal strings per weight
        .def("unmask_rationals", [](const Aggregation& a, const MaskObject& mask_obj) {
            py::list out;
            for (const Rational& r : a.unmask(mask_obj))
                out.append(py::make_tuple(r.numer.to_dec(), r.denom.to_dec()));
            return out;
        })
        .def("unmask", [](const Aggregation& a, const MaskObject& mask_obj) -> py::object {
            RationalModel rm = a.unmask(mask_obj);
            switch (a.config().vect.dtype) {
                case DataType::F32: {
                    auto v = model_to_f32(rm);
                    return py::array_t<float>(py::ssize_t(v.size()), v.data());
                }
                case DataType::F64: {
                    auto v = model_to_f64(rm);
                    return py::array_t<double>(py::ssize_t(v.size()), v.data());
                }
                case DataType::I32: {
                    auto v = model_to_i32(rm);
                    return py::array_t<int32_t>(py::ssize_t(v.size()), v.data());
                }
                case DataType::I64: {
                    auto v = model_to_i64(rm);
                    return py::array_t<int64_t>(py::ssize_t(v.size()), v.data());
                }
            }
            throw std::runtime_error("unreachable");
        });
}
