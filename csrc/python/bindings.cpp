// Python bindings (pybind11): the native core exposed to the Python package.
// (The reference has no Python API; this is the torch-facing front end of the
// same engine the C++ CLI drives)
//
// Device buffers cross the boundary as integer pointers (torch tensor
// data_ptr()) plus a stream handle (torch.cuda.current_stream().cuda_stream),
// so the Python side never copies pixel data; host images cross as numpy arrays.
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <thread>
#include <pybind11/stl.h>

#include <memory>

#include "../hip/launch_policy.h"
#include "stripe/chain.h"
#include "stripe/comm.h"
#include "stripe/engine.h"
#include "stripe/trace.h"
#include "stripe/golden.h"
#include "stripe/cpu_exec.h"
#include "stripe/image.h"
#include "stripe/orient.h"
#include "stripe/partition.h"
#include "stripe/rank_net.h"

namespace py = pybind11;
using namespace stripe;

namespace {

using U8Array = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>;

Image image_from_numpy(const U8Array& a) {
  Image img;
  if (a.ndim() == 2) {
    img = Image((int)a.shape(1), (int)a.shape(0), 1, NoInit{});
  } else if (a.ndim() == 3) {
    img = Image((int)a.shape(1), (int)a.shape(0), (int)a.shape(2), NoInit{});
  } else {
    fail("image array must be HxW or HxWxC");
  }
  STRIPE_CHECK(img.C == 1 || img.C == 3, "image must have 1 or 3 channels");
  std::memcpy(img.data.data(), a.data(), img.bytes());
  return img;
}

U8Array image_to_numpy(const Image& img) {
  std::vector<py::ssize_t> shape = {img.H, img.W};
  if (img.C != 1) shape.push_back(img.C);
  U8Array a(shape);
  std::memcpy(a.mutable_data(), img.data.data(), img.bytes());
  return a;
}

hipStream_t as_stream(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

// Histograms cross as int64 arrays of shape (C, 256) (a (256,) array is one channel).
using I64Array = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;

py::array_t<int64_t> hist_to_numpy(const Histogram& h) {
  py::array_t<int64_t> a(std::vector<py::ssize_t>{h.C, 256});
  int64_t* d = a.mutable_data();
  for (size_t i = 0; i < h.bins.size(); ++i) d[i] = (int64_t)h.bins[i];
  return a;
}

Histogram hist_from_numpy(const I64Array& a) {
  STRIPE_CHECK((a.ndim() == 1 && a.shape(0) == 256) || (a.ndim() == 2 && a.shape(1) == 256 &&
                                                         (a.shape(0) == 1 || a.shape(0) == 3)),
               "histogram must have shape (256,), (1, 256) or (3, 256)");
  Histogram h(a.ndim() == 1 ? 1 : (int)a.shape(0));
  const int64_t* s = a.data();
  for (size_t i = 0; i < h.bins.size(); ++i) {
    STRIPE_CHECK(s[i] >= 0, "histogram counts must not be negative");
    h.bins[i] = (uint64_t)s[i];
  }
  return h;
}

// A crop window crosses as None or (x0, y0, w, h).
CropRect crop_from_py(const py::object& o) {
  if (o.is_none()) return {};
  const auto t = o.cast<std::tuple<int, int, int, int>>();
  CropRect c{std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t)};
  STRIPE_CHECK(c.w >= 1 && c.h >= 1, "crop (" << c.x0 << ", " << c.y0 << ", " << c.w << ", " << c.h << "): empty window");
  return c;
}

Op stat_op(const std::string& token) {
  auto ops = parse_chain(token);
  STRIPE_CHECK(ops.size() == 1 && ops[0].kind == OpKind::Stat,
               "'" << token << "' is not one statistic op (equalize, autocontrast[:P], threshold:otsu)");
  return ops[0];
}

// Comm wrapper owning its hub reference (Python-visible handle).
struct PyComm {
  std::unique_ptr<Comm> comm;
};

}  // namespace

PYBIND11_MODULE(_C, m) {
  m.doc() = "stripe: MI355X-native distributed image filtering core (HIP/RCCL)";

  py::register_exception<Error>(m, "StripeError", PyExc_RuntimeError);

  py::enum_<Border>(m, "Border")
      .value("reflect101", Border::Reflect101)
      .value("replicate", Border::Replicate)
      .value("constant", Border::Constant)
      .value("skip", Border::Skip);
  m.def("parse_border", &parse_border);
  m.def("border_index", &border_index);

  py::enum_<BackendKind>(m, "Backend").value("device", BackendKind::Device).value("host", BackendKind::Host);

  // ---- image I/O ----
  m.def("read_pnm", [](const std::string& p) { return image_to_numpy(read_pnm(p)); });
  m.def("write_pnm", [](const std::string& p, const U8Array& a) { write_pnm(p, image_from_numpy(a)); });
  m.def("decode_pnm", [](py::bytes b) { return image_to_numpy(decode_pnm(std::string(b))); });
  m.def("encode_pnm", [](const U8Array& a) { return py::bytes(encode_pnm(image_from_numpy(a))); });
  m.def("decode_jpeg", [](py::bytes b) { return image_to_numpy(decode_jpeg(std::string(b))); });
  m.def(
      "encode_jpeg",
      [](const U8Array& a, int quality, bool subsample, int restart) {
        return py::bytes(encode_jpeg(image_from_numpy(a), quality, subsample, restart));
      },
      py::arg("img"), py::arg("quality") = 95, py::arg("subsample") = true, py::arg("restart_interval") = -1);
  // JPEG split at the entropy stage: Huffman on the host, pixels on the GPU
  py::class_<JpegCoefs>(m, "JpegCoefs")
      .def_readonly("W", &JpegCoefs::W)
      .def_readonly("H", &JpegCoefs::H)
      .def_property_readonly("C", [](const JpegCoefs& j) { return (int)j.comps.size(); })
      .def(
          "to_device",
          [](const JpegCoefs& j, uintptr_t dst, int64_t pitch, uintptr_t stream) {
            py::gil_scoped_release nogil;
            jpeg_pixels_device(j, reinterpret_cast<uint8_t*>(dst), pitch, as_stream(stream));
          },
          py::arg("dst"), py::arg("pitch"), py::arg("stream") = 0)
      .def("to_host", [](const JpegCoefs& j) {
        JpegCoefs c = j;
        return image_to_numpy(jpeg_pixels(std::move(c)));
      });
  m.def("jpeg_entropy_decode", [](py::bytes b) {
    const std::string s(b);
    py::gil_scoped_release nogil;
    return jpeg_entropy_decode(s);
  });
  m.def(
      "jpeg_encode_device",
      [](uintptr_t src, int64_t pitch, int W, int H, int C, int quality, bool subsample, int restart, uintptr_t stream) {
        std::string out;
        {
          py::gil_scoped_release nogil;
          out = jpeg_entropy_encode(
              jpeg_quantise_device(reinterpret_cast<const uint8_t*>(src), pitch, W, H, C, quality, subsample,
                                   as_stream(stream)),
              restart);
        }
        return py::bytes(out);
      },
      py::arg("src"), py::arg("pitch"), py::arg("W"), py::arg("H"), py::arg("C"), py::arg("quality") = 95,
      py::arg("subsample") = true, py::arg("restart_interval") = -1, py::arg("stream") = 0);
  m.def("read_image", [](const std::string& p) { return image_to_numpy(read_image(p)); });
  m.def(
      "write_image", [](const std::string& p, const U8Array& a, int q) { write_image(p, image_from_numpy(a), q); },
      py::arg("path"), py::arg("img"), py::arg("quality") = 95);
  m.def("synth_image", [](uint64_t seed, int W, int H, int C) { return image_to_numpy(synth_image(seed, W, H, C)); });
  m.def("synth_rows", [](uint64_t seed, int W, int C, int row0, int rows) {
    Image img(W, rows, C, NoInit{});
    synth_rows(seed, W, C, row0, rows, img.data.data());
    return image_to_numpy(img);
  });
  m.def("synth_byte", [](uint64_t seed, int64_t y, int64_t b) { return synth_byte(seed, y, b); });
  m.def("pattern_word", [](uint32_t tag, uint64_t j) { return pattern_word(tag, j); });

  // ---- filter spec ----
  m.def("parse_chain", [](const std::string& s) { return chain_to_string(parse_chain(s)); },
        "canonical spelling of a chain");
  m.def("gray_pixel", [](const std::string& mode, int r, int g, int b) {
    return (int)gray_pixel(mode == "ref" ? GrayMode::Ref : GrayMode::BT601, (uint8_t)r, (uint8_t)g, (uint8_t)b);
  });
  m.def("pointwise_lut", [](const std::string& op) {
    auto ops = parse_chain(op);
    STRIPE_CHECK(ops.size() == 1 && ops[0].pointwise() && ops[0].kind != OpKind::Gray &&
                     ops[0].kind != OpKind::Expand && ops[0].kind != OpKind::ColorMatrix,
                 "pointwise_lut needs one per-channel op");
    std::vector<int> lut(256);
    for (int v = 0; v < 256; ++v) lut[v] = apply_pointwise_u8(ops[0], (uint8_t)v);
    return lut;
  });
  m.def("filter_catalogue", &filter_catalogue, "(syntax, description) rows of the parser's token table, in its order");
  m.def("stencil_names", [] {
    std::vector<std::string> names;
    for (int i = 0; i < (int)StencilId::kCount; ++i) names.push_back(stencil_info((StencilId)i).name);
    return names;
  }, "canonical names of the integer stencils, in id order");
  m.def("stencil_weights", [](const std::string& name) {
    StencilId sid;
    STRIPE_CHECK(stencil_from_name(name, &sid), "unknown stencil " << name);
    const StencilInfo& s = stencil_info(sid);
    py::dict d;
    d["K"] = s.K;
    d["w"] = s.w;
    d["div"] = s.div;
    d["separable"] = s.separable;
    d["sobel"] = s.sobel;
    d["rank"] = rank_name(s.rank);  // "none" | "min" | "max" | "median" (rank filters: w empty)
    d["bilateral"] = s.bilateral;   // w: the spatial weights; the range table: bilateral_table
    return d;
  });
  m.def("color_matrix", [](const std::string& token) {
    // the quantised matrix of one colour token (colormatrix:..., sepia, ...), for the tests
    auto ops = parse_chain(token);
    STRIPE_CHECK(ops.size() == 1 && ops[0].kind == OpKind::ColorMatrix, "color_matrix needs one colour matrix token");
    py::dict d;
    py::list q;
    for (int c = 0; c < 3; ++c) q.append(std::vector<int>(ops[0].cm + 3 * c, ops[0].cm + 3 * c + 3));
    d["q"] = q;
    d["b"] = std::vector<int>(ops[0].cm + 9, ops[0].cm + 12);
    d["shift"] = kColorShift;
    return d;
  }, "Q12 coefficients of a colour matrix token: out_c = sat((sum_k q[c][k] p_k + b[c] + 2048) >> 12)");
  m.def("bilateral_table", [](const std::string& token) {
    // the range table of one bilateral token, for the tests
    auto ops = parse_chain(token);
    STRIPE_CHECK(ops.size() == 1 && ops[0].kind == OpKind::Stencil && stencil_info(ops[0].sid).bilateral,
                 "bilateral_table needs one bilateral token");
    return std::vector<int>(ops[0].range.begin(), ops[0].range.end());
  }, "r[d] = rint(255 exp(-d^2 / (2 S^2))), d = 0..255, of a bilateral token (filters.h)");
  m.def("rank_network", [](int K) {
    // the median networks of rank_net.h as (i, j, mode) steps, for the tests
    STRIPE_CHECK(K == 3 || K == 5, "rank networks exist for K = 3 and 5");
    py::dict d;
    py::list cs, sel;
    auto fill = [](py::list& l, auto net) {
      for (int k = 0; k < decltype(net)::N; ++k) l.append(py::make_tuple(net.at(k).i, net.at(k).j, net.at(k).mode));
    };
    if (K == 3) {
      fill(cs, ranknet::ColSort<3>{});
      fill(sel, ranknet::Select<3>{});
      d["out"] = ranknet::Select<3>::kOut;
    } else {
      fill(cs, ranknet::ColSort<5>{});
      fill(sel, ranknet::Select<5>{});
      d["out"] = ranknet::Select<5>::kOut;
    }
    d["colsort"] = cs;
    d["select"] = sel;
    return d;
  }, "compare-exchange networks of the KxK median (mode 0: both, 1: min -> i, 2: max -> j)");
  m.def("gaussian_1d", &gaussian_1d, py::arg("K"), py::arg("sigma") = 0.0);
  m.def("describe_chain", [](const std::string& chain, int cin, const std::string& border, bool fuse) {
    return compile_chain(parse_chain(chain), cin, parse_border(border), fuse).describe();
  }, py::arg("chain"), py::arg("cin") = 3, py::arg("border") = "reflect101", py::arg("fuse") = true);
  m.def("combine_u8", [](const std::string& token, const U8Array& x, const U8Array& h) {
    // one combine token (add, sub, ..., lincomb:a:b[:c], blend:t, above[:d]) on two equal-shaped arrays
    auto ops = parse_chain(token);
    STRIPE_CHECK(ops.size() == 1 && ops[0].kind == OpKind::Combine, "'" << token << "' is not one combine op");
    STRIPE_CHECK(x.size() == h.size(), "combine_u8: the arrays differ in size");
    U8Array out(std::vector<py::ssize_t>(x.shape(), x.shape() + x.ndim()));
    const uint8_t* px = x.data();
    const uint8_t* ph = h.data();
    uint8_t* po = out.mutable_data();
    for (py::ssize_t i = 0; i < x.size(); ++i) po[i] = combine_u8(ops[0], px[i], ph[i]);
    return out;
  }, py::arg("token"), py::arg("x"), py::arg("h"),
        "combine_u8 (filters.h) per byte: x the current image's bytes, h the held image's");
  m.def("plan_info", [](const std::string& chain, int cin, const std::string& border, bool fuse, int held_channels) {
    Plan p = compile_chain(parse_chain(chain), cin, parse_border(border), fuse, held_channels);
    py::dict d;
    d["cin"] = p.cin;
    d["cout"] = p.cout;
    d["max_radius"] = p.max_radius;
    d["in_margin_px"] = p.in_margin_px;
    py::list passes;
    for (const auto& ps : p.passes) {
      py::dict q;
      q["kind"] = (int)ps.kind;
      q["desc"] = ps.desc;
      q["R"] = ps.R;
      q["cin"] = ps.cin;
      q["cout"] = ps.cout;
      q["cmid"] = ps.cmid;
      q["epi_lut"] = ps.has_epi;
      q["epi_expand"] = ps.epi_expand;
      q["out_margin_px"] = ps.out_margin_px;
      q["cmat"] = ps.pro.cmat;
      q["stat"] = ps.pro.has_stat ? ps.pro.stat.text : std::string();  // statistic op leading the program
      // two-image plans: the slot actions in front of the pass, a combine pass's op and folded table
      py::list slots;
      for (char a : ps.slots) slots.append(a == 'h' ? "hold" : "swap");
      q["slots"] = slots;
      q["combine"] = ps.kind == PassKind::Combine ? std::string(combine_name(ps.comb)) : std::string();
      q["post_lut"] = ps.kind == PassKind::Combine && ps.pro.has_post;
      q["fill_in"] = ps.fill_in;
      q["bilateral"] = ps.bilateral;
      q["sigma"] = ps.bilateral ? ps.sigma : 0.0;  // the range sigma S
      passes.append(q);
    }
    d["passes"] = passes;
    d["data_dependent"] = p.data_dependent();
    d["branched"] = p.branched();
    d["static_chain"] = p.static_chain();
    return d;
  }, py::arg("chain"), py::arg("cin") = 3, py::arg("border") = "reflect101", py::arg("fuse") = true,
     py::arg("held_channels") = 0);

  // ---- launch policy (csrc/hip/launch_policy.h: pure host functions, no GPU) ----
  m.def("launch_policy", [](const std::string& family, int cin, int cout, int cmid, int W, int rows, int nt, int wgs,
                            bool gray_prologue, bool lut_stage, int W2, int rows2, int64_t mesh_bytes) {
    static const std::pair<const char*, policy::Family> names[] = {
        {"sep", policy::Family::Sep},           {"sobel_rp", policy::Family::SobelRp},
        {"direct", policy::Family::Direct},     {"rank", policy::Family::Rank},
        {"bilateral", policy::Family::Bilateral},
        {"conv_small", policy::Family::ConvSmall}, {"pointwise", policy::Family::PointwiseChan},
        {"pointwise_flat", policy::Family::PointwiseFlat}, {"colormix", policy::Family::ColorMix},
        {"blur", policy::Family::Blur},         {"combine", policy::Family::Combine},
        {"resize", policy::Family::Resize},     {"orient", policy::Family::Orient},
        {"warp", policy::Family::Warp},         {"remap", policy::Family::Remap}};
    const policy::Family* f = nullptr;
    for (const auto& n : names)
      if (family == n.first) f = &n.second;
    STRIPE_CHECK(f != nullptr, "unknown kernel family '" << family << "'");
    policy::PolicyIn in{*f};
    in.cin = cin;
    in.cout = cout;
    in.cmid = cmid;
    in.W = W;
    in.rows = rows;
    in.nt = nt;
    in.wgs = wgs;
    in.gray_prologue = gray_prologue;
    in.lut_stage = lut_stage;
    in.W2 = W2;
    in.rows2 = rows2;
    in.mesh_bytes = mesh_bytes;
    const policy::StreamPolicy r = policy::stream_policy(in);
    py::dict d;
    d["nt_stores"] = r.nt_stores;
    d["streaming"] = r.streaming;
    d["nxcd"] = r.nxcd;
    d["cap"] = r.cap;
    d["cap_applied"] = r.cap_applied;
    return d;
  }, py::arg("family"), py::arg("cin") = 3, py::arg("cout") = 3, py::arg("cmid") = 3, py::arg("W") = 0,
     py::arg("rows") = 0, py::arg("nt") = -1, py::arg("wgs") = -1, py::arg("gray_prologue") = false,
     py::arg("lut_stage") = false, py::arg("W2") = 0, py::arg("rows2") = 0, py::arg("mesh_bytes") = 0,
     "the launch decision of a kernel family: sep | sobel_rp | direct | rank | bilateral | conv_small | pointwise | "
     "pointwise_flat | colormix | blur | combine | resize (W2, rows2: the destination of a resize) | orient (W, rows: "
     "the source window) | warp (W, rows: the source; W2, rows2: the destination) | remap (as warp; mesh_bytes: the "
     "bytes of the mesh)");
  m.def("lds_reserve_bytes", &policy::lds_reserve_bytes, py::arg("lds_per_cu"), py::arg("static_lds"),
        py::arg("target"));

  // ---- golden ----
  // held: a second image of the same shape, the external held image of the chain (None: none)
  m.def("golden_apply", [](const U8Array& a, const std::string& chain, const std::string& border, bool fuse,
                           py::object held) {
    Image img = image_from_numpy(a);
    Image himg;
    if (!held.is_none()) himg = image_from_numpy(held.cast<U8Array>());
    const bool has_held = !held.is_none();
    Image out;
    {
      py::gil_scoped_release nogil;
      Plan p = compile_chain(parse_chain(chain), img.C, parse_border(border), fuse, has_held ? himg.C : 0);
      out = golden_apply_plan(img, p, has_held ? &himg : nullptr);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("chain"), py::arg("border") = "reflect101", py::arg("fuse") = true,
     py::arg("held") = py::none());
  m.def("cpu_apply", [](const U8Array& a, const std::string& chain, const std::string& border, bool fuse,
                        int threads, py::object held) {
    Image img = image_from_numpy(a);
    Image himg;
    if (!held.is_none()) himg = image_from_numpy(held.cast<U8Array>());
    const bool has_held = !held.is_none();
    Image out;
    {
      py::gil_scoped_release nogil;
      Plan p = compile_chain(parse_chain(chain), img.C, parse_border(border), fuse, has_held ? himg.C : 0);
      out = cpu_apply_plan(img, p, threads > 0 ? threads : cpu_threads(), has_held ? &himg : nullptr);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("chain"), py::arg("border") = "reflect101", py::arg("fuse") = true,
     py::arg("threads") = 0, py::arg("held") = py::none());
  m.def("golden_apply_unfused", [](const U8Array& a, const std::string& chain, const std::string& border,
                                   py::object held) {
    Image img = image_from_numpy(a);
    Image himg;
    if (!held.is_none()) himg = image_from_numpy(held.cast<U8Array>());
    const bool has_held = !held.is_none();
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_apply_ops(img, parse_chain(chain), parse_border(border), has_held ? &himg : nullptr);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("chain"), py::arg("border") = "reflect101", py::arg("held") = py::none());

  // ---- resize (stripe/resize.h): a stage in front of the chain, not a chain token ----
  m.def("parse_resize_spec", [](const std::string& token) {
    const ResizeSpec r = parse_resize_spec(token);
    return py::make_tuple(r.W, r.H, std::string(resize_mode_name(r.mode)));
  }, py::arg("spec"), "'WxH[:mode]' -> (W, H, mode)");
  m.def("resize_taps", [](int n_in, int n_out, const std::string& mode) {
    const ResizeTaps t = resize_taps(n_in, n_out, parse_resize_mode(mode));
    py::array_t<int32_t> first((py::ssize_t)t.first.size()), count((py::ssize_t)t.first.size());
    py::array_t<int32_t> w((py::ssize_t)t.w.size());
    for (size_t i = 0; i < t.first.size(); ++i) {
      first.mutable_data()[i] = t.first[i];
      count.mutable_data()[i] = t.count((int)i);
    }
    for (size_t i = 0; i < t.w.size(); ++i) w.mutable_data()[i] = t.w[i];
    return py::make_tuple(first, count, w);
  }, py::arg("n_in"), py::arg("n_out"), py::arg("mode") = "auto",
     "(first, count, weights): per output index the first input index and the tap count; the Q15 weights of all "
     "outputs, concatenated in order");
  m.def("golden_resize", [](const U8Array& a, int W2, int H2, const std::string& mode) {
    const Image img = image_from_numpy(a);
    const ResizeMode rm = parse_resize_mode(mode);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_resize(img, W2, H2, rm);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("W2"), py::arg("H2"), py::arg("mode") = "auto");
  m.def("cpu_resize", [](const U8Array& a, int W2, int H2, const std::string& mode, int threads) {
    const Image img = image_from_numpy(a);
    const ResizeMode rm = parse_resize_mode(mode);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = cpu_resize(img, W2, H2, rm, threads > 0 ? threads : cpu_threads());
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("W2"), py::arg("H2"), py::arg("mode") = "auto", py::arg("threads") = 0);
  m.def("resize_device", [](uintptr_t src, int64_t src_pitch, int W, int H, int C, uintptr_t dst, int64_t dst_pitch,
                            int W2, int H2, const std::string& mode, uintptr_t stream) {
    const ResizeMode rm = parse_resize_mode(mode);
    py::gil_scoped_release nogil;
    resize_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, C, reinterpret_cast<uint8_t*>(dst),
                  dst_pitch, W2, H2, rm, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("C"), py::arg("dst"),
     py::arg("dst_pitch"), py::arg("W2"), py::arg("H2"), py::arg("mode") = "auto", py::arg("stream") = 0,
     "k_resize on pitched device buffers (any alignment), queued on the stream");
  m.def("resize_tile", [] {
    py::dict d;
    d["tile"] = kResizeTile;
    d["band"] = kResizeBand;
    return d;
  }, "k_resize's tile constants: output bytes per workgroup tile, output rows per band");

  // ---- orientation and crop (stripe/orient.h): a stage in front of the chain, not a chain token ----
  m.def("orient_names", [] { return orient_names(); }, "the eight orientation names in Exif order (1..8)");
  m.def("parse_orient", [](const std::string& token) {
    const Orient o = parse_orient(token);
    return py::make_tuple(std::string(orient_name(o)), (int)o);
  }, py::arg("token"), "a name, cw / ccw or exif:N -> (name, bits = T << 2 | FX << 1 | FY)");
  m.def("orient_compose", [](const std::string& a, const std::string& b) {
    return std::string(orient_name(orient_compose(parse_orient(a), parse_orient(b))));
  }, py::arg("a"), py::arg("b"), "the one orientation equal to a, then b");
  m.def("orient_inverse", [](const std::string& a) { return std::string(orient_name(orient_inverse(parse_orient(a)))); },
        py::arg("a"));
  m.def("parse_crop_spec", [](const std::string& spec, int W, int H) {
    const CropRect c = parse_crop_spec(spec);
    if (W > 0 || H > 0) check_crop(c, W, H, spec);
    return py::make_tuple(c.x0, c.y0, c.w, c.h);
  }, py::arg("spec"), py::arg("W") = 0, py::arg("H") = 0,
     "'WxH+X+Y' -> (x0, y0, w, h); with W, H (the oriented frame) the window must lie inside it");
  m.def("orient_source_window", [](const std::string& op, int w, int h, const py::object& crop) {
    const CropRect c = orient_source_window(parse_orient(op), w, h, crop_from_py(crop));
    return py::make_tuple(c.x0, c.y0, c.w, c.h);
  }, py::arg("op"), py::arg("w"), py::arg("h"), py::arg("crop") = py::none(),
     "the window of the w x h source that the crop of the oriented frame comes from");
  m.def("golden_orient", [](const U8Array& a, const std::string& op, const py::object& crop) {
    const Image img = image_from_numpy(a);
    const Orient o = parse_orient(op);
    const CropRect c = crop_from_py(crop);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_orient(img, o, c);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("op"), py::arg("crop") = py::none());
  m.def("cpu_orient", [](const U8Array& a, const std::string& op, const py::object& crop, int threads) {
    const Image img = image_from_numpy(a);
    const Orient o = parse_orient(op);
    const CropRect c = crop_from_py(crop);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = cpu_orient(img, o, c, threads > 0 ? threads : cpu_threads());
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("op"), py::arg("crop") = py::none(), py::arg("threads") = 0);
  m.def("orient_device", [](uintptr_t src, int64_t src_pitch, int W, int H, int C, uintptr_t dst, int64_t dst_pitch,
                            const std::string& op, const py::object& crop, uintptr_t stream) {
    const Orient o = parse_orient(op);
    const CropRect c = crop_from_py(crop);
    py::gil_scoped_release nogil;
    orient_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, C, reinterpret_cast<uint8_t*>(dst),
                  dst_pitch, o, c, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("C"), py::arg("dst"),
     py::arg("dst_pitch"), py::arg("op"), py::arg("crop") = py::none(), py::arg("stream") = 0,
     "k_orient on pitched device buffers (any alignment), queued on the stream; crop: a window of the oriented frame");
  m.def("orient_tile", [] {
    py::dict d;
    for (int t = 0; t < 2; ++t) {
      py::dict e;
      e["rows"] = orient_tile_rows(t);
      e["seg_gray"] = orient_seg_px(1, t);
      e["seg_rgb"] = orient_seg_px(3, t);
      e["lds_gray"] = orient_lds_bytes(1, t);
      e["lds_rgb"] = orient_lds_bytes(3, t);
      d[t ? "transposing" : "fx"] = e;
    }
    d["copy_rows"] = kOrientCopyRows;
    d["cpu_tile"] = kCpuOrientTile;
    return d;
  }, "k_orient's tile constants, for the FX and the transposing instances: source rows of a tile, source pixels "
     "per tile row (gray / RGB), LDS bytes; rows per workgroup of the copying instances; cpu_orient's tile side");
  m.def("jpeg_orientation", [](py::bytes b) {
    const std::string s(b);
    return jpeg_orientation(reinterpret_cast<const uint8_t*>(s.data()), s.size());
  }, py::arg("data"), "Exif Orientation (1..8) of a JPEG stream; 1 when it carries no well-formed one");

  // ---- affine warp (stripe/warp.h): a stage in front of the chain, not a chain token ----
  // A quantised map travels as its six integers (A00, A01, B0, A10, A11, B1) and the destination size.
  static const auto warp_map_from_py = [](const std::vector<int64_t>& q, int W2, int H2, const std::string& mode,
                                          const std::string& border, int fill) {
    STRIPE_CHECK(q.size() == 6, "warp: a quantised map is six integers (A00, A01, B0, A10, A11, B1), got " << q.size());
    STRIPE_CHECK(fill >= 0 && fill <= 255, "warp: the fill value must be in 0..255, got " << fill);
    WarpMap m;
    const int64_t lim = int64_t(64) << kWarpQ;
    for (int i = 0; i < 2; ++i) {
      STRIPE_CHECK(q[3 * i] > -lim && q[3 * i] < lim && q[3 * i + 1] > -lim && q[3 * i + 1] < lim,
                   "warp: map coefficient outside (-64, 64)");
      STRIPE_CHECK(q[3 * i + 2] > -(int64_t(1) << (20 + kWarpQ)) && q[3 * i + 2] < (int64_t(1) << (20 + kWarpQ)),
                   "warp: map offset outside (-2^20, 2^20)");
      m.A[i][0] = (int32_t)q[3 * i], m.A[i][1] = (int32_t)q[3 * i + 1], m.B[i] = q[3 * i + 2];
    }
    m.W2 = W2, m.H2 = H2;
    m.mode = parse_warp_mode(mode);
    if (border == "constant") m.border = WarpBorder::Constant, m.fill = (uint8_t)fill;
    else if (border == "replicate") m.border = WarpBorder::Replicate;
    else fail("warp: unknown border '" + border + "' (constant | replicate)");
    return m;
  };
  m.def("warp_quantise", [](const std::vector<double>& M, bool inverse, int W, int H, int W2, int H2,
                            const std::string& token) {
    STRIPE_CHECK(M.size() == 6, "warp: a matrix is six numbers a, b, c, d, e, f (row-major 2 x 3), got " << M.size());
    const WarpMap q = warp_quantise(M.data(), inverse, W, H, W2 > 0 ? W2 : W, H2 > 0 ? H2 : H, WarpMode::Bilinear,
                                    WarpBorder::Constant, 0, token);
    return py::make_tuple((int64_t)q.A[0][0], (int64_t)q.A[0][1], q.B[0], (int64_t)q.A[1][0], (int64_t)q.A[1][1], q.B[1],
                          q.W2, q.H2);
  }, py::arg("M"), py::arg("inverse") = false, py::arg("W") = 1, py::arg("H") = 1, py::arg("W2") = 0,
     py::arg("H2") = 0, py::arg("token") = "matrix",
     "(A00, A01, B0, A10, A11, B1, W2, H2): the Q24 inverse map of the forward (or, inverse=True, the inverse) "
     "matrix; W2, H2 = 0: the source's size");
  m.def("rotate_matrix", [](double deg, bool fit, int W, int H) {
    const Rotation r = rotate_matrix(deg, fit, W, H);
    return py::make_tuple(std::vector<double>(r.minv, r.minv + 6), r.W2, r.H2);
  }, py::arg("deg"), py::arg("fit"), py::arg("W"), py::arg("H"),
     "(inverse matrix, W2, H2) of a counter-clockwise rotation about the source centre");
  m.def("parse_warp_spec", [](const std::string& spec) {
    const WarpSpec s = parse_warp_spec(spec);
    return py::make_tuple(std::vector<double>(s.M, s.M + 6), s.W2, s.H2);
  }, py::arg("spec"), "'a;b;c;d;e;f[:WxH]' -> (forward matrix, W2, H2); 0, 0 without a size");
  m.def("parse_rotate_spec", [](const std::string& spec) {
    const RotateSpec r = parse_rotate_spec(spec);
    return py::make_tuple(r.deg, r.fit, rotate_token(r));
  }, py::arg("spec"), "'DEG[:same|fit]' -> (deg, fit, canonical token)");
  m.def("warp_token", [](const std::vector<double>& M, int W2, int H2) {
    STRIPE_CHECK(M.size() == 6, "warp: a matrix is six numbers");
    WarpSpec s;
    for (int i = 0; i < 6; ++i) s.M[i] = M[(size_t)i];
    return warp_token(s, W2, H2);
  }, py::arg("M"), py::arg("W2"), py::arg("H2"), "the canonical token of a forward matrix and its destination size");
  m.def("parse_warp_border", [](const std::string& token) {
    WarpBorder b;
    uint8_t fill;
    parse_warp_border(token, &b, &fill);
    return py::make_tuple(std::string(warp_border_name(b)), (int)fill);
  }, py::arg("token"), "'constant[:V]' | 'replicate' -> (name, fill)");
  m.def("parse_warp_mode", [](const std::string& token) { return std::string(warp_mode_name(parse_warp_mode(token))); },
        py::arg("token"));
  m.def("golden_warp", [](const U8Array& a, const std::vector<int64_t>& q, int W2, int H2, const std::string& mode,
                          const std::string& border, int fill) {
    const Image img = image_from_numpy(a);
    const WarpMap wm = warp_map_from_py(q, W2, H2, mode, border, fill);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_warp(img, wm);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("map"), py::arg("W2"), py::arg("H2"), py::arg("mode") = "bilinear",
     py::arg("border") = "constant", py::arg("fill") = 0);
  m.def("cpu_warp", [](const U8Array& a, const std::vector<int64_t>& q, int W2, int H2, const std::string& mode,
                       const std::string& border, int fill, int threads) {
    const Image img = image_from_numpy(a);
    const WarpMap wm = warp_map_from_py(q, W2, H2, mode, border, fill);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = cpu_warp(img, wm, threads > 0 ? threads : cpu_threads());
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("map"), py::arg("W2"), py::arg("H2"), py::arg("mode") = "bilinear",
     py::arg("border") = "constant", py::arg("fill") = 0, py::arg("threads") = 0);
  m.def("warp_device", [](uintptr_t src, int64_t src_pitch, int W, int H, int C, uintptr_t dst, int64_t dst_pitch,
                          const std::vector<int64_t>& q, int W2, int H2, const std::string& mode,
                          const std::string& border, int fill, uintptr_t stream) {
    const WarpMap wm = warp_map_from_py(q, W2, H2, mode, border, fill);
    py::gil_scoped_release nogil;
    warp_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, C, reinterpret_cast<uint8_t*>(dst), dst_pitch,
                wm, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("C"), py::arg("dst"),
     py::arg("dst_pitch"), py::arg("map"), py::arg("W2"), py::arg("H2"), py::arg("mode") = "bilinear",
     py::arg("border") = "constant", py::arg("fill") = 0, py::arg("stream") = 0,
     "k_warp on pitched device buffers (any alignment), queued on the stream");
  m.def("warp_tile", [] {
    py::dict d;
    d["tile"] = kWarpTile;
    d["box"] = kWarpBox;
    d["row_bytes_gray"] = warp_row_bytes(1);
    d["row_bytes_rgb"] = warp_row_bytes(3);
    d["lds_gray"] = warp_lds_bytes(1);
    d["lds_rgb"] = warp_lds_bytes(3);
    return d;
  }, "k_warp's tile constants: destination pixels per tile side, source pixels per side of the staged box, "
     "bytes of a staged row and LDS bytes of the staged instances (gray / RGB); the direct instances hold none");
  m.def("warp_plan", [](const std::vector<int64_t>& q) {
    const WarpMap wm = warp_map_from_py(q, 1, 1, "bilinear", "constant", 0);
    return std::string(warp_plan_staged(wm) ? "staged" : "direct");
  }, py::arg("map"), "'staged' | 'direct': the k_warp instance a quantised map takes");

  // ---- mesh warp (stripe/remap.h): perspective, undistort, remap; in the affine warp's slot ----
  // A mesh travels as an int32 array of shape (gh, gw, 2) with its spacing.
  using MeshArray = py::array_t<int32_t, py::array::c_style>;
  static const auto mesh_to_numpy = [](const Mesh& me) {
    MeshArray out({(py::ssize_t)me.gh(), (py::ssize_t)me.gw(), (py::ssize_t)2});
    std::memcpy(out.mutable_data(), me.nodes.data(), me.nodes.size() * sizeof(int32_t));
    return py::make_tuple(out, me.spacing());
  };
  static const auto remap_view = [](const int32_t* nodes, int spacing, int W2, int H2, const std::string& mode,
                                    const std::string& border, int fill) {
    STRIPE_CHECK(fill >= 0 && fill <= 255, "remap: the fill value must be in 0..255, got " << fill);
    RemapMesh rm;
    rm.nodes = nodes;
    rm.shift = remap_shift(spacing);
    rm.W2 = W2, rm.H2 = H2;
    rm.mode = parse_warp_mode(mode);
    if (border == "constant") rm.border = WarpBorder::Constant, rm.fill = (uint8_t)fill;
    else if (border == "replicate") rm.border = WarpBorder::Replicate;
    else fail("warp: unknown border '" + border + "' (constant | replicate)");
    return rm;
  };
  static const auto mesh_from_numpy = [](const py::array& mesh, int spacing, int W2, int H2, const std::string& mode,
                                         const std::string& border, int fill, MeshArray* keep) {
    STRIPE_CHECK(py::isinstance<py::array_t<int32_t>>(mesh), "remap 'mesh': the mesh must be an int32 array");
    *keep = MeshArray::ensure(mesh);
    STRIPE_CHECK(*keep, "remap 'mesh': the mesh must be an int32 array");
    RemapMesh rm = remap_view(keep->data(), spacing, W2, H2, mode, border, fill);
    STRIPE_CHECK(W2 >= 1 && W2 <= kWarpMaxSize && H2 >= 1 && H2 <= kWarpMaxSize,
                 "remap 'mesh': destination size " << W2 << "x" << H2 << " outside 1.." << kWarpMaxSize);
    STRIPE_CHECK(keep->ndim() == 3 && keep->shape(0) == rm.gh() && keep->shape(1) == rm.gw() && keep->shape(2) == 2,
                 "remap 'mesh': a mesh of spacing " << spacing << " for " << W2 << "x" << H2 << " has shape " << rm.gh()
                                                    << "x" << rm.gw() << "x2");
    check_mesh(rm, (int64_t)keep->size(), true);
    return rm;
  };
  m.def("perspective_mesh", [](const std::vector<double>& Hm, bool inverse, int W, int H, int W2, int H2, int spacing,
                               const std::string& token) {
    STRIPE_CHECK(Hm.size() == 9, "remap '" << token << "': a matrix is nine numbers (row-major 3 x 3), got " << Hm.size());
    return mesh_to_numpy(perspective_mesh(Hm.data(), inverse, W, H, W2 > 0 ? W2 : W, H2 > 0 ? H2 : H, spacing, token));
  }, py::arg("H"), py::arg("inverse") = false, py::arg("W") = 1, py::arg("Hs") = 1, py::arg("W2") = 0,
     py::arg("H2") = 0, py::arg("spacing") = 0, py::arg("token") = "perspective",
     "(int32 mesh (gh, gw, 2), spacing) of the forward (or, inverse=True, the inverse) 3 x 3 matrix for a W x Hs "
     "source; W2, H2 = 0: the source's size; spacing 0: automatic");
  m.def("radial_mesh", [](double k1, double k2, py::object f, py::object centre, int W, int H, int spacing,
                          const std::string& token) {
    RadialSpec r;
    r.k1 = k1, r.k2 = k2;
    if (!f.is_none()) r.has_f = true, r.f = f.cast<double>();
    if (!centre.is_none()) {
      const auto c = centre.cast<std::vector<double>>();
      STRIPE_CHECK(c.size() == 2, "remap '" << token << "': the centre is (cx, cy)");
      r.has_centre = true, r.cx = c[0], r.cy = c[1];
    }
    return mesh_to_numpy(radial_mesh(r, W, H, spacing, token));
  }, py::arg("k1"), py::arg("k2") = 0.0, py::arg("f") = py::none(), py::arg("centre") = py::none(), py::arg("W") = 1,
     py::arg("H") = 1, py::arg("spacing") = 0, py::arg("token") = "undistort",
     "(int32 mesh, spacing) of the radial undistortion map of a W x H frame");
  m.def("perspective_from_points", [](const std::vector<double>& src, const std::vector<double>& dst) {
    STRIPE_CHECK(src.size() == 8 && dst.size() == 8, "remap 'points': four points x, y each for source and destination");
    std::vector<double> Hm(9);
    perspective_from_points(src.data(), dst.data(), Hm.data());
    return Hm;
  }, py::arg("src"), py::arg("dst"), "cv::getPerspectiveTransform: the forward matrix, row-major");
  m.def("parse_quad_spec", [](const std::string& spec) {
    const QuadSpec q = parse_quad_spec(spec);
    return py::make_tuple(std::vector<double>(q.pts, q.pts + 8), q.W2, q.H2);
  }, py::arg("spec"), "'x0,y0;x1,y1;x2,y2;x3,y3[:WxH]' -> (points TL TR BR BL, W2, H2), the default size resolved");
  m.def("quad_matrix", [](const std::vector<double>& pts, int W2, int H2) {
    STRIPE_CHECK(pts.size() == 8, "remap 'quad': four points x, y each");
    if (W2 <= 0 || H2 <= 0) quad_default_size(pts.data(), &W2, &H2);
    std::vector<double> Hm(9);
    quad_matrix(pts.data(), W2, H2, Hm.data());
    return py::make_tuple(Hm, W2, H2);
  }, py::arg("points"), py::arg("W2") = 0, py::arg("H2") = 0,
     "(forward matrix, W2, H2) that maps the quad TL TR BR BL to the destination's corners");
  m.def("parse_perspective_spec", [](const std::string& spec) {
    const PerspectiveSpec p = parse_perspective_spec(spec);
    return py::make_tuple(std::vector<double>(p.Hm, p.Hm + 9), p.W2, p.H2);
  }, py::arg("spec"), "'h00;...;h22[:WxH]' -> (forward matrix, W2, H2); 0, 0 without a size");
  m.def("parse_undistort_spec", [](const std::string& spec) {
    const RadialSpec r = parse_undistort_spec(spec);
    return py::make_tuple(r.k1, r.k2, r.has_f ? py::object(py::float_(r.f)) : py::object(py::none()),
                          r.has_centre ? py::object(py::make_tuple(r.cx, r.cy)) : py::object(py::none()));
  }, py::arg("spec"), "'k1[;k2[;f[;cx;cy]]]' -> (k1, k2, f | None, (cx, cy) | None)");
  m.def("perspective_token", [](const std::vector<double>& Hm, int W2, int H2) {
    STRIPE_CHECK(Hm.size() == 9, "remap: a matrix is nine numbers");
    return perspective_token(Hm.data(), W2, H2);
  }, py::arg("H"), py::arg("W2"), py::arg("H2"), "the canonical token of a forward matrix and its destination size");
  m.def("quad_token", [](const std::vector<double>& pts, int W2, int H2) {
    STRIPE_CHECK(pts.size() == 8, "remap: a quad is four points");
    return quad_token(pts.data(), W2, H2);
  }, py::arg("points"), py::arg("W2"), py::arg("H2"));
  m.def("undistort_token", [](const std::string& spec, int W, int H) {
    return undistort_token(radial_resolve(parse_undistort_spec(spec), W, H));
  }, py::arg("spec"), py::arg("W"), py::arg("H"), "the canonical token of an undistort spec for a W x H frame");
  m.def("golden_remap", [](const U8Array& a, const py::array& mesh, int spacing, int W2, int H2, const std::string& mode,
                           const std::string& border, int fill) {
    const Image img = image_from_numpy(a);
    MeshArray keep;
    const RemapMesh rm = mesh_from_numpy(mesh, spacing, W2, H2, mode, border, fill, &keep);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_remap(img, rm);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("mesh"), py::arg("spacing"), py::arg("W2"), py::arg("H2"), py::arg("mode") = "bilinear",
     py::arg("border") = "constant", py::arg("fill") = 0);
  m.def("cpu_remap", [](const U8Array& a, const py::array& mesh, int spacing, int W2, int H2, const std::string& mode,
                        const std::string& border, int fill, int threads) {
    const Image img = image_from_numpy(a);
    MeshArray keep;
    const RemapMesh rm = mesh_from_numpy(mesh, spacing, W2, H2, mode, border, fill, &keep);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = cpu_remap(img, rm, threads > 0 ? threads : cpu_threads());
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("mesh"), py::arg("spacing"), py::arg("W2"), py::arg("H2"), py::arg("mode") = "bilinear",
     py::arg("border") = "constant", py::arg("fill") = 0, py::arg("threads") = 0);
  m.def("remap_device", [](uintptr_t src, int64_t src_pitch, int W, int H, int C, uintptr_t dst, int64_t dst_pitch,
                           uintptr_t mesh, int64_t mesh_count, int spacing, int W2, int H2, const std::string& mode,
                           const std::string& border, int fill, uintptr_t stream) {
    STRIPE_CHECK(mesh != 0, "bad remap launch: null mesh");
    const RemapMesh rm = remap_view(reinterpret_cast<const int32_t*>(mesh), spacing, W2, H2, mode, border, fill);
    py::gil_scoped_release nogil;
    remap_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, C, reinterpret_cast<uint8_t*>(dst), dst_pitch,
                 rm, mesh_count, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("C"), py::arg("dst"),
     py::arg("dst_pitch"), py::arg("mesh"), py::arg("mesh_count"), py::arg("spacing"), py::arg("W2"), py::arg("H2"),
     py::arg("mode") = "bilinear", py::arg("border") = "constant", py::arg("fill") = 0, py::arg("stream") = 0,
     "k_remap on pitched device buffers (any alignment) with a device-resident int32 mesh of mesh_count values, "
     "queued on the stream");
  m.def("remap_tile", [] {
    py::dict d;
    d["tile"] = kWarpTile;
    d["box"] = kWarpBox;
    d["lds_spacing"] = kRemapLdsSpacing;
    d["nodes"] = kRemapNodes;
    d["node_bytes"] = remap_node_bytes();
    d["reduce_bytes"] = kRemapReduceBytes;
    d["lds_gray"] = remap_lds_bytes(1);
    d["lds_rgb"] = remap_lds_bytes(3);
    return d;
  }, "k_remap's tile constants: destination pixels per tile side, source pixels per side of the staged box, the "
     "smallest spacing whose nodes go to LDS, nodes per tile side, their bytes, and the LDS bytes of an instance");

  // ---- connected components (stripe/components.h): labels, stats, area filter; entry points of their own ----
  static const auto labels_to_numpy = [](const std::vector<int32_t>& l, int W, int H) {
    py::array_t<int32_t> a(std::vector<py::ssize_t>{H, W});
    std::memcpy(a.mutable_data(), l.data(), l.size() * sizeof(int32_t));
    return a;
  };
  static const auto stats_to_numpy = [](const std::vector<int64_t>& t) {
    py::array_t<int64_t> a(std::vector<py::ssize_t>{(py::ssize_t)(t.size() / kStatCols), kStatCols});
    std::memcpy(a.mutable_data(), t.data(), t.size() * sizeof(int64_t));
    return a;
  };
  m.def("parse_connectivity", &parse_connectivity, py::arg("token"));
  m.def("golden_components", [labels = labels_to_numpy](const U8Array& a, int conn) {
    const Image img = image_from_numpy(a);
    std::vector<int32_t> l;
    int n;
    {
      py::gil_scoped_release nogil;
      n = golden_components(img, conn, &l);
    }
    return py::make_tuple(labels(l, img.W, img.H), n);
  }, py::arg("image"), py::arg("connectivity") = 8, "(int32 labels HxW, N): the flood-fill oracle");
  m.def("cpu_components", [labels = labels_to_numpy](const U8Array& a, int conn, int threads) {
    const Image img = image_from_numpy(a);
    check_components(img.W, img.H, img.C, conn);
    std::vector<int32_t> l((size_t)img.W * img.H);
    int n;
    {
      py::gil_scoped_release nogil;
      n = cpu_components(img.data.data(), img.W, img.W, img.H, conn, l.data(), img.W,
                         threads > 0 ? threads : cpu_threads());
    }
    return py::make_tuple(labels(l, img.W, img.H), n);
  }, py::arg("image"), py::arg("connectivity") = 8, py::arg("threads") = 0,
     "(int32 labels HxW, N) on the host executor: min(threads, H) row blocks");
  using I32Array = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
  m.def("component_stats", [stats = stats_to_numpy](const I32Array& l, int n, int threads) {
    STRIPE_CHECK(l.ndim() == 2 && l.shape(0) >= 1 && l.shape(1) >= 1, "components: labels must be HxW");
    const int H = (int)l.shape(0), W = (int)l.shape(1);
    std::vector<int64_t> t;
    {
      py::gil_scoped_release nogil;
      t = threads == 1 ? component_stats(l.data(), W, W, H, n)
                       : cpu_component_stats(l.data(), W, W, H, n, threads > 0 ? threads : cpu_threads());
    }
    return stats(t);
  }, py::arg("labels"), py::arg("n"), py::arg("threads") = 1,
     "int64 (n + 1, 7): area, x0, y0, x1, y1, sum_x, sum_y per label (threads = 1: the plain loop)");
  m.def("golden_area_filter", [](const U8Array& a, int conn, int64_t amin, int64_t amax) {
    const Image img = image_from_numpy(a);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_area_filter(img, conn, amin, amax);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("connectivity") = 8, py::arg("min_area") = 1, py::arg("max_area") = kAreaNoLimit);
  m.def("cpu_area_filter", [](const U8Array& a, int conn, int64_t amin, int64_t amax, int threads) {
    const Image img = image_from_numpy(a);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = cpu_area_filter(img, conn, amin, amax, threads > 0 ? threads : cpu_threads());
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("connectivity") = 8, py::arg("min_area") = 1, py::arg("max_area") = kAreaNoLimit,
     py::arg("threads") = 0);
  m.def("components_device", [](uintptr_t src, int64_t src_pitch, int W, int H, int conn, uintptr_t labels,
                                int64_t labels_pitch, uintptr_t stream) {
    py::gil_scoped_release nogil;
    return components_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, conn,
                             reinterpret_cast<int32_t*>(labels), labels_pitch, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("connectivity"), py::arg("labels"),
     py::arg("labels_pitch"), py::arg("stream") = 0,
     "k_ccl_* on a pitched u8 device mask (any alignment) into an int32 device plane (pitch in elements); returns N "
     "after the call's one synchronisation of the stream");
  m.def("component_stats_device", [](uintptr_t labels, int64_t labels_pitch, int W, int H, int n, uintptr_t stats,
                                     uintptr_t stream) {
    py::gil_scoped_release nogil;
    component_stats_device(reinterpret_cast<const int32_t*>(labels), labels_pitch, W, H, n,
                           reinterpret_cast<int64_t*>(stats), as_stream(stream));
  }, py::arg("labels"), py::arg("labels_pitch"), py::arg("W"), py::arg("H"), py::arg("n"), py::arg("stats"),
     py::arg("stream") = 0, "k_ccl_stats into an int64 (n + 1, 7) device table; synchronises the stream");
  m.def("area_filter_device", [](uintptr_t src, int64_t src_pitch, int W, int H, uintptr_t labels, int64_t labels_pitch,
                                 uintptr_t stats, int n, int64_t amin, int64_t amax, uintptr_t dst, int64_t dst_pitch,
                                 uintptr_t stream) {
    py::gil_scoped_release nogil;
    area_filter_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, reinterpret_cast<const int32_t*>(labels),
                       labels_pitch, reinterpret_cast<const int64_t*>(stats), n, amin, amax,
                       reinterpret_cast<uint8_t*>(dst), dst_pitch, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("labels"), py::arg("labels_pitch"),
     py::arg("stats"), py::arg("n"), py::arg("min_area"), py::arg("max_area"), py::arg("dst"), py::arg("dst_pitch"),
     py::arg("stream") = 0, "k_ccl_select: the area filter from device labels and their device table, queued on the stream");
  m.def("components_tile", [] { return py::make_tuple(kCclTile, kCclTile); }, "k_ccl_tile's tile: (tw, th) pixels");
  m.def("components_lds", [] {
    py::dict d;
    d["k_ccl_tile"] = ccl_lds_bytes();
    d["k_ccl_number"] = ccl_number_lds_bytes();
    d["k_ccl_scan"] = ccl_scan_lds_bytes();
    return d;
  }, "LDS bytes of the k_ccl_* kernels that use any");
  m.attr("AREA_NO_LIMIT") = kAreaNoLimit;
  m.attr("STAT_COLUMNS") = std::vector<std::string>{"area", "x0", "y0", "x1", "y1", "sum_x", "sum_y"};

  // ---- distance transform and disc morphology (stripe/distance.h); entry points of their own ----
  static const auto plane_to_numpy = [](const std::vector<int32_t>& d, int W, int H) {
    py::array_t<int32_t> a(std::vector<py::ssize_t>{H, W});
    std::memcpy(a.mutable_data(), d.data(), d.size() * sizeof(int32_t));
    return a;
  };
  m.def("golden_distance", [plane = plane_to_numpy](const U8Array& a, bool to_foreground) {
    const Image img = image_from_numpy(a);
    std::vector<int32_t> d;
    {
      py::gil_scoped_release nogil;
      golden_distance(img, to_foreground, &d);
    }
    return plane(d, img.W, img.H);
  }, py::arg("image"), py::arg("to_foreground") = false,
     "int32 squared distances HxW: the column scans and the brute-force minimum over every column, O(W^2 H)");
  m.def("cpu_distance", [plane = plane_to_numpy](const U8Array& a, bool to_foreground, int threads) {
    const Image img = image_from_numpy(a);
    check_distance(img.W, img.H, img.C);
    std::vector<int32_t> d((size_t)img.W * img.H);
    {
      py::gil_scoped_release nogil;
      cpu_distance(img.data.data(), img.W, img.W, img.H, to_foreground, d.data(), img.W,
                   threads > 0 ? threads : cpu_threads());
    }
    return plane(d, img.W, img.H);
  }, py::arg("image"), py::arg("to_foreground") = false, py::arg("threads") = 0,
     "int32 squared distances HxW on the host executor (column blocks, then lower envelopes over row blocks)");
  m.def("golden_distance_u8", [](const U8Array& a, bool to_foreground) {
    const Image img = image_from_numpy(a);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_distance_u8(img, to_foreground);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("to_foreground") = false);
  m.def("golden_distance_mask", [](const U8Array& a, bool to_foreground, int64_t t, bool keep_above) {
    const Image img = image_from_numpy(a);
    check_distance_mode((int)DistanceMode::MaskAbove, t);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_distance_mask(img, to_foreground, (int32_t)t, keep_above);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("to_foreground"), py::arg("t"), py::arg("keep_above"));
  m.def("cpu_distance_u8", [](const U8Array& a, bool to_foreground, int threads) {
    const Image img = image_from_numpy(a);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = cpu_distance_u8(img, to_foreground, threads > 0 ? threads : cpu_threads());
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("to_foreground") = false, py::arg("threads") = 0);
  m.def("cpu_distance_mask", [](const U8Array& a, bool to_foreground, int64_t t, bool keep_above, int threads) {
    const Image img = image_from_numpy(a);
    check_distance_mode((int)DistanceMode::MaskAbove, t);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = cpu_distance_mask(img, to_foreground, (int32_t)t, keep_above, threads > 0 ? threads : cpu_threads());
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("to_foreground"), py::arg("t"), py::arg("keep_above"), py::arg("threads") = 0);
  m.def("golden_disk_morph", [](const U8Array& a, const std::string& op, double radius) {
    const Image img = image_from_numpy(a);
    const DiskOp o = parse_disk_op(op);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_disk_morph(img, o, radius);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("op"), py::arg("radius"), "erode / dilate / open / close by the disc {dx^2 + dy^2 <= floor(r^2)}");
  m.def("cpu_disk_morph", [](const U8Array& a, const std::string& op, double radius, int threads) {
    const Image img = image_from_numpy(a);
    const DiskOp o = parse_disk_op(op);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = cpu_disk_morph(img, o, radius, threads > 0 ? threads : cpu_threads());
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("op"), py::arg("radius"), py::arg("threads") = 0);
  m.def("check_radius", [](double r) { return (int64_t)check_radius(r); }, py::arg("radius"),
        "floor(r^2), the threshold of a disc of radius r; refuses a negative or non-finite radius");
  m.def("distance_device", [](uintptr_t src, int64_t src_pitch, int W, int H, bool to_foreground, int mode, int64_t t,
                              uintptr_t dst, int64_t dst_pitch, uintptr_t stream) {
    py::gil_scoped_release nogil;
    distance_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, to_foreground, mode, t,
                    reinterpret_cast<void*>(dst), dst_pitch, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("to_foreground"), py::arg("mode"),
     py::arg("t"), py::arg("dst"), py::arg("dst_pitch"), py::arg("stream") = 0,
     "k_edt_* on a pitched u8 device mask (any alignment); mode 0: int32 d^2 (pitch in elements), 1: u8 floor(sqrt), "
     "2 / 3: u8 mask d^2 > t / d^2 <= t; queued on the stream, no synchronisation");
  m.def("disk_morph_device", [](uintptr_t src, int64_t src_pitch, int W, int H, const std::string& op, int64_t t,
                                uintptr_t dst, int64_t dst_pitch, uintptr_t stream) {
    const int o = (int)parse_disk_op(op);
    py::gil_scoped_release nogil;
    disk_morph_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, o, t, reinterpret_cast<uint8_t*>(dst),
                      dst_pitch, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("op"), py::arg("t"), py::arg("dst"),
     py::arg("dst_pitch"), py::arg("stream") = 0,
     "erode / dilate (one column and one row pass) or open / close (two, through a cached u8 mask) with t = floor(r^2)");
  m.def("distance_release_scratch", [] {
    py::gil_scoped_release nogil;
    distance_release_scratch();
  }, "free the cached device scratch of the distance transform");
  m.def("distance_tile", [] { return py::make_tuple(kEdtBand, kEdtRowThreads, kEdtRowsPerGroup); },
        "(rows per band of the column pass, threads of a row-pass workgroup, rows per row-pass workgroup)");
  m.def("distance_widths", [] { return std::vector<int>(kEdtWidths, kEdtWidths + 3); },
        "the row pass's LDS classes: the largest W of each");
  m.def("distance_lds", [] {
    py::dict d;
    for (int w : kEdtWidths) d[py::int_(w)] = edt_row_lds_bytes(w);
    return d;
  }, "LDS bytes of k_edt_row per width class (the other k_edt_* kernels use none)");
  m.attr("DISTANCE_NONE") = (int64_t)kDistanceNone;
  m.attr("DISTANCE_MAX_SIDE") = kDistanceMaxSide;
  m.attr("DISTANCE_MODES") = std::vector<std::string>{"squared", "u8", "mask_above", "mask_within"};

  // ---- integral images and the window operations (stripe/integral.h); entry points of their own ----
  static const auto table_to_numpy = [](const std::vector<int32_t>& t, int W, int H) {
    py::array_t<int32_t> a(std::vector<py::ssize_t>{H + 1, W + 1});
    std::memcpy(a.mutable_data(), t.data(), t.size() * sizeof(int32_t));
    return a;
  };
  static const auto window_spec = [](const std::string& op, int K, int c, double k) {
    WindowSpec spec;
    spec.op = parse_window_op(op);
    spec.K = K, spec.C = c;
    spec.kq = window_kq(k);
    return spec;
  };
  m.def("golden_integral", [table = table_to_numpy](const U8Array& a, bool squared) {
    const Image img = image_from_numpy(a);
    std::vector<int32_t> t;
    {
      py::gil_scoped_release nogil;
      golden_integral(img, squared, &t);
    }
    return table(t, img.W, img.H);
  }, py::arg("image"), py::arg("squared") = false,
     "int32 (H + 1) x (W + 1): I[y][x] = the sum of p (p^2) over y' < y, x' < x modulo 2^32, cv::integral's layout");
  m.def("cpu_integral", [table = table_to_numpy](const U8Array& a, bool squared, int threads) {
    const Image img = image_from_numpy(a);
    check_integral(img.W, img.H, img.C);
    std::vector<int32_t> t(((size_t)img.W + 1) * ((size_t)img.H + 1));
    {
      py::gil_scoped_release nogil;
      cpu_integral(img.data.data(), img.W, img.W, img.H, squared, t.data(), img.W + 1,
                   threads > 0 ? threads : cpu_threads());
    }
    return table(t, img.W, img.H);
  }, py::arg("image"), py::arg("squared") = false, py::arg("threads") = 0,
     "the integral on the host executor (block-local scans over row blocks plus carries)");
  m.def("golden_window", [spec_of = window_spec](const U8Array& a, const std::string& op, int K, const std::string& border,
                                                 int c, double k) {
    const Image img = image_from_numpy(a);
    const WindowSpec spec = spec_of(op, K, c, k);
    const Border b = parse_border(border);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_window(img, spec, b);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("op"), py::arg("ksize"), py::arg("border") = "reflect101", py::arg("c") = 0,
     py::arg("k") = 0.0, "box / std / mean / niblack / sauvola over a K x K window: the plain loop over the extended frame");
  m.def("cpu_window", [spec_of = window_spec](const U8Array& a, const std::string& op, int K, const std::string& border,
                                              int c, double k, int threads) {
    const Image img = image_from_numpy(a);
    check_integral(img.W, img.H, img.C);
    const WindowSpec spec = spec_of(op, K, c, k);
    const Border b = parse_border(border);
    Image out(img.W, img.H, 1);
    {
      py::gil_scoped_release nogil;
      cpu_window(img.data.data(), img.W, img.W, img.H, spec, b, out.data.data(), img.W,
                 threads > 0 ? threads : cpu_threads());
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("op"), py::arg("ksize"), py::arg("border") = "reflect101", py::arg("c") = 0,
     py::arg("k") = 0.0, py::arg("threads") = 0,
     "the window operations on the host executor: the wrapping u32 tables, then four corners per table and pixel");
  m.def("window_kq", [](double k) { return window_kq(k); }, py::arg("k"),
        "nearbyint(4096 k), ties to even; refuses a non-finite k and |k| > 4");
  m.def("integral_device", [](uintptr_t src, int64_t src_pitch, int W, int H, bool squared, uintptr_t dst,
                              int64_t dst_pitch, uintptr_t stream) {
    py::gil_scoped_release nogil;
    integral_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, squared, reinterpret_cast<int32_t*>(dst),
                    dst_pitch, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("squared"), py::arg("dst"),
     py::arg("dst_pitch"), py::arg("stream") = 0,
     "k_sat_* on a pitched u8 device frame (any alignment) into an int32 plane of (H + 1) x (W + 1) (pitch in "
     "elements); queued on the stream, no synchronisation");
  m.def("window_device", [](uintptr_t src, int64_t src_pitch, int W, int H, int op, int K, const std::string& border,
                            int c, int64_t kq, uintptr_t dst, int64_t dst_pitch, uintptr_t stream) {
    const int b = (int)parse_border(border);
    py::gil_scoped_release nogil;
    window_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, op, K, b, c, kq,
                  reinterpret_cast<uint8_t*>(dst), dst_pitch, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("op"), py::arg("ksize"),
     py::arg("border"), py::arg("c"), py::arg("kq"), py::arg("dst"), py::arg("dst_pitch"), py::arg("stream") = 0,
     "the tables of the extended frame (k_sat_reduce / carry / scan), then k_sat_window<op> (op: the index in "
     "WINDOW_OPS, kq = window_kq(k)); queued on the stream, no synchronisation");
  m.def("integral_release_scratch", [] {
    py::gil_scoped_release nogil;
    integral_release_scratch();
  }, "free the cached device scratch of the integral images");
  m.def("integral_tile", [] { return py::make_tuple(kSatTile, kSatWaves, kSatWindowPixels); },
        "(rows and columns of a wave's tile, wave tiles side by side in a workgroup, pixels per lane of k_sat_window)");
  m.def("integral_lds", [] {
    py::dict d;
    for (const char* name : {"k_sat_reduce", "k_sat_carry", "k_sat_scan", "k_sat_window"}) d[name] = sat_lds_bytes();
    return d;
  }, "LDS bytes of each k_sat_* kernel");
  m.attr("INTEGRAL_MAX_SIDE") = kIntegralMaxSide;
  m.attr("WINDOW_MAX_K") = kWindowMaxK;
  m.attr("WINDOW_MAX_K_SQUARES") = kWindowMaxKSquares;
  m.attr("WINDOW_MAX_ABS_K") = kWindowMaxAbsK;
  m.attr("WINDOW_OPS") = std::vector<std::string>{"box", "std", "mean", "niblack", "sauvola"};

  // ---- canny and hysteresis thresholding (stripe/canny.h); entry points of their own ----
  // The host executor's calls take any uint8 array whose rows are packed (a strided view is read in place) and,
  // with `out`, write into such a view.
  struct U8View {
    uint8_t* p;
    int64_t pitch;
    int W, H, C;
  };
  static const auto u8_view = [](const py::array& a, bool writable) {
    STRIPE_CHECK(a.dtype().is(py::dtype::of<uint8_t>()), "canny: the image must be uint8");
    STRIPE_CHECK(a.ndim() == 2 || a.ndim() == 3, "canny: the image must be HxW or HxWx1");
    STRIPE_CHECK(!writable || a.writeable(), "canny: out is not writable");
    U8View v{};
    v.H = (int)a.shape(0), v.W = (int)a.shape(1), v.C = a.ndim() == 3 ? (int)a.shape(2) : 1;
    // (C != 1 is refused by the caller's check, with the message every layer shares)
    STRIPE_CHECK(v.C != 1 || ((v.W <= 1 || a.strides(1) == 1) && (v.H <= 1 || a.strides(0) >= v.W)),
                 "canny: a row's pixels must be packed and the rows must not overlap");
    v.p = static_cast<uint8_t*>(const_cast<void*>(a.data()));
    v.pitch = v.H > 1 ? (int64_t)a.strides(0) : v.W;
    return v;
  };
  static const auto u8_out = [](const py::object& out, int W, int H) {
    if (out.is_none()) return py::array(py::array_t<uint8_t>(std::vector<py::ssize_t>{H, W}));
    STRIPE_CHECK(py::isinstance<py::array>(out), "canny: out must be a numpy array");
    py::array o = py::reinterpret_borrow<py::array>(out);
    STRIPE_CHECK(o.ndim() == 2 && o.shape(0) == H && o.shape(1) == W, "canny: out must be " << H << "x" << W);
    return o;
  };
  m.def("golden_canny", [](const U8Array& a, int low, int high, const std::string& norm, const std::string& border) {
    const Image img = image_from_numpy(a);
    const CannyNorm n = parse_canny_norm(norm);
    const Border b = parse_border(border);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_canny(img, low, high, n, b);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("low"), py::arg("high"), py::arg("norm") = "l1", py::arg("border") = "reflect101",
     "the u8 edge map (255 / 0): golden_canny_classes, then the flood fill from every class 2 pixel, 8-connected");
  m.def("golden_canny_classes", [](const U8Array& a, int low, int high, const std::string& norm,
                                   const std::string& border) {
    const Image img = image_from_numpy(a);
    const CannyNorm n = parse_canny_norm(norm);
    const Border b = parse_border(border);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_canny_classes(img, low, high, n, b);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("low"), py::arg("high"), py::arg("norm") = "l1", py::arg("border") = "reflect101",
     "the class plane (0 suppressed or weak, 1 weak candidate, 2 strong): the plain loops over the extended frame");
  m.def("golden_hysteresis_threshold", [](const U8Array& a, int low, int high, int conn) {
    const Image img = image_from_numpy(a);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = golden_hysteresis_threshold(img, low, high, conn);
    }
    return image_to_numpy(out);
  }, py::arg("image"), py::arg("low"), py::arg("high"), py::arg("connectivity") = 8,
     "255 where p > low and the pixel is connected through pixels > low to one > high, else 0");
  m.def("cpu_canny", [view = u8_view, out_of = u8_out](const py::array& a, int low, int high, const std::string& norm,
                                                      const std::string& border, int threads, const py::object& out) {
    const U8View s = view(a, false);
    const CannyNorm n = parse_canny_norm(norm);
    const Border b = parse_border(border);
    check_canny(s.W, s.H, s.C, low, high, (int)n, b);
    py::array o = out_of(out, s.W, s.H);
    const U8View d = view(o, true);
    {
      py::gil_scoped_release nogil;
      cpu_canny(s.p, s.pitch, s.W, s.H, low, high, n, b, d.p, d.pitch, threads > 0 ? threads : cpu_threads());
    }
    return o;
  }, py::arg("image"), py::arg("low"), py::arg("high"), py::arg("norm") = "l1", py::arg("border") = "reflect101",
     py::arg("threads") = 0, py::arg("out") = py::none(),
     "canny on the host executor (row blocks, then cpu_components on the class plane); strided views are used in place");
  m.def("cpu_canny_classes", [view = u8_view, out_of = u8_out](const py::array& a, int low, int high,
                                                              const std::string& norm, const std::string& border,
                                                              int threads, const py::object& out) {
    const U8View s = view(a, false);
    const CannyNorm n = parse_canny_norm(norm);
    const Border b = parse_border(border);
    check_canny(s.W, s.H, s.C, low, high, (int)n, b);
    py::array o = out_of(out, s.W, s.H);
    const U8View d = view(o, true);
    {
      py::gil_scoped_release nogil;
      cpu_canny_classes(s.p, s.pitch, s.W, s.H, low, high, n, b, d.p, d.pitch, threads > 0 ? threads : cpu_threads());
    }
    return o;
  }, py::arg("image"), py::arg("low"), py::arg("high"), py::arg("norm") = "l1", py::arg("border") = "reflect101",
     py::arg("threads") = 0, py::arg("out") = py::none(), "the class plane on the host executor");
  m.def("cpu_hysteresis_threshold", [view = u8_view, out_of = u8_out](const py::array& a, int low, int high, int conn,
                                                                     int threads, const py::object& out) {
    const U8View s = view(a, false);
    check_hysteresis(s.W, s.H, s.C, low, high, conn);
    py::array o = out_of(out, s.W, s.H);
    const U8View d = view(o, true);
    {
      py::gil_scoped_release nogil;
      cpu_hysteresis_threshold(s.p, s.pitch, s.W, s.H, low, high, conn, d.p, d.pitch,
                               threads > 0 ? threads : cpu_threads());
    }
    return o;
  }, py::arg("image"), py::arg("low"), py::arg("high"), py::arg("connectivity") = 8, py::arg("threads") = 0,
     py::arg("out") = py::none(), "hysteresis thresholding on the host executor");
  m.def("canny_device", [](uintptr_t src, int64_t src_pitch, int W, int H, int low, int high, const std::string& norm,
                           const std::string& border, uintptr_t dst, int64_t dst_pitch, uintptr_t stream) {
    const int n = (int)parse_canny_norm(norm), b = (int)parse_border(border);
    py::gil_scoped_release nogil;
    canny_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, low, high, n, b,
                 reinterpret_cast<uint8_t*>(dst), dst_pitch, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("low"), py::arg("high"), py::arg("norm"),
     py::arg("border"), py::arg("dst"), py::arg("dst_pitch"), py::arg("stream") = 0,
     "k_canny_nms, the forest passes of k_ccl_*, k_canny_mark and k_canny_select on a pitched u8 device frame (any "
     "alignment); returns after the call's one synchronisation of the stream");
  m.def("canny_classes_device", [](uintptr_t src, int64_t src_pitch, int W, int H, int low, int high,
                                   const std::string& norm, const std::string& border, uintptr_t dst, int64_t dst_pitch,
                                   uintptr_t stream) {
    const int n = (int)parse_canny_norm(norm), b = (int)parse_border(border);
    py::gil_scoped_release nogil;
    canny_classes_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, low, high, n, b,
                         reinterpret_cast<uint8_t*>(dst), dst_pitch, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("low"), py::arg("high"), py::arg("norm"),
     py::arg("border"), py::arg("dst"), py::arg("dst_pitch"), py::arg("stream") = 0,
     "k_canny_nms alone: the class plane; queued on the stream, no synchronisation");
  m.def("hysteresis_device", [](uintptr_t src, int64_t src_pitch, int W, int H, int low, int high, int conn,
                                uintptr_t dst, int64_t dst_pitch, uintptr_t stream) {
    py::gil_scoped_release nogil;
    hysteresis_device(reinterpret_cast<const uint8_t*>(src), src_pitch, W, H, low, high, conn,
                      reinterpret_cast<uint8_t*>(dst), dst_pitch, as_stream(stream));
  }, py::arg("src"), py::arg("src_pitch"), py::arg("W"), py::arg("H"), py::arg("low"), py::arg("high"),
     py::arg("connectivity"), py::arg("dst"), py::arg("dst_pitch"), py::arg("stream") = 0,
     "k_canny_classify, the forest passes, k_canny_mark and k_canny_select; returns after the call's one "
     "synchronisation of the stream");
  m.def("canny_release_scratch", [] {
    py::gil_scoped_release nogil;
    canny_release_scratch();
  }, "free the cached device scratch of canny and hysteresis thresholding");
  m.def("canny_tile", [] { return py::make_tuple(kCannyTileX, kCannyTileY); }, "k_canny_nms's tile: (tx, ty) pixels");
  m.def("canny_lds", [] {
    py::dict d;
    d["k_canny_nms"] = canny_nms_lds_bytes();
    for (const char* name : {"k_canny_classify", "k_canny_mark", "k_canny_select"}) d[name] = 0;
    return d;
  }, "LDS bytes of each k_canny_* kernel");
  m.attr("CANNY_MAX_THRESHOLD") = kCannyMaxThreshold;
  m.attr("HYSTERESIS_MAX_THRESHOLD") = kHysteresisMaxThreshold;
  m.attr("CANNY_NORMS") = std::vector<std::string>{"l1", "l2"};

  // ---- histogram and the statistic ops' tables ----
  m.def("golden_histogram", [](const U8Array& a) { return hist_to_numpy(golden_histogram(image_from_numpy(a))); },
        py::arg("image"), "int64 counts of shape (C, 256)");
  m.def("cpu_histogram", [](const U8Array& a, int threads) {
    Image img = image_from_numpy(a);
    Histogram h;
    {
      py::gil_scoped_release nogil;
      h = cpu_histogram(img, threads > 0 ? threads : cpu_threads());
    }
    return hist_to_numpy(h);
  }, py::arg("image"), py::arg("threads") = 0, "golden_histogram on the host executor's threads");
  m.def("stat_lut", [](const std::string& token, const I64Array& hist) {
    const std::array<uint8_t, 256> l = stat_lut(stat_op(token), hist_from_numpy(hist));
    return std::vector<int>(l.begin(), l.end());
  }, py::arg("token"), py::arg("hist"),
        "the 256-entry table of equalize | autocontrast[:P] | threshold:otsu for a (C, 256) histogram (channels pooled)");
  m.def("otsu_level", [](const I64Array& hist) { return otsu_level(hist_from_numpy(hist)); }, py::arg("hist"));

  // ---- partition ----
  m.def("plan_rows", [](int H, int world, int min_rows, bool legacy) {
    Partition p = plan_rows(H, world, min_rows, legacy);
    std::vector<std::pair<int, int>> v;
    for (const auto& s : p.stripes) v.emplace_back(s.row0, s.rows);
    return py::make_tuple(v, p.active);
  }, py::arg("H"), py::arg("world"), py::arg("min_rows") = 1, py::arg("legacy") = false);
  m.def("plan_rows_weighted", [](int H, const std::vector<double>& w, int min_rows) {
    Partition p = plan_rows_weighted(H, w, min_rows);
    std::vector<std::pair<int, int>> v;
    for (const auto& s : p.stripes) v.emplace_back(s.row0, s.rows);
    return py::make_tuple(v, p.active);
  }, py::arg("H"), py::arg("weights"), py::arg("min_rows") = 1);
  m.def("plan_dist_split", [](int H, int world, double row_in, double row_out, double root_rows_per_ms,
                              double peer_rows_per_ms, double link_bytes_per_ms, double hbm_bytes_per_ms, int chunks,
                              int min_rows) {
    const DistSplit d = plan_dist_split(H, world, row_in, row_out, root_rows_per_ms, peer_rows_per_ms,
                                        link_bytes_per_ms, hbm_bytes_per_ms, chunks, min_rows);
    py::dict r;
    r["weights"] = d.weights;
    r["rows"] = d.rows;
    r["root_ms"] = d.root_ms;
    r["peer_ms"] = d.peer_ms;
    r["floor_ms"] = d.floor_ms;
    r["predicted_ms"] = d.predicted_ms;
    r["even_ms"] = d.even_ms;
    return r;
  }, py::arg("H"), py::arg("world"), py::arg("row_in_bytes"), py::arg("row_out_bytes"), py::arg("root_rows_per_ms"),
     py::arg("peer_rows_per_ms"), py::arg("link_bytes_per_ms"), py::arg("hbm_bytes_per_ms"), py::arg("chunks") = 8,
     py::arg("min_rows") = 1);

  // ---- comm ----
  py::class_<PyComm>(m, "Comm")
      .def_property_readonly("rank", [](const PyComm& c) { return c.comm->rank(); })
      .def_property_readonly("size", [](const PyComm& c) { return c.comm->size(); })
      .def_property_readonly("backend", [](const PyComm& c) { return std::string(c.comm->backend()); })
      .def("barrier", [](PyComm& c) {
        py::gil_scoped_release nogil;
        c.comm->barrier();
      })
      .def("abort", [](PyComm& c, const std::string& why) { c.comm->abort(why); })
      // brackets for batched halo posts (Engine.post_halo of several engines)
      .def("group_start", [](PyComm& c) { c.comm->group_start(); })
      .def("group_end", [](PyComm& c) {
        py::gil_scoped_release nogil;
        c.comm->group_end();
      })
      .def("identity", [](const PyComm& c) {
        py::dict d;
        for (const auto& kv : c.comm->identity()) d[kv.first.c_str()] = kv.second;
        return d;
      });
  m.def("preconnect_peers", &preconnect_peers, py::arg("rank"), py::arg("world"));
  // Test hook (tests/test_r6_advice.py): two host `local` ranks, rank 1 posts
  // a receive of the wrong size.  Returns the errors of that group, of rank
  // 0's send, and of a second group on rank 1 afterwards (the aborted hub's
  // message, not a stale pending receive or an open group).
  m.def("local_comm_failure_probe", []() {
    py::gil_scoped_release nogil;
    auto hub = make_local_hub(2, false, 30.0);
    auto c0 = make_local_comm(hub, 0);
    auto c1 = make_local_comm(hub, 1);
    std::vector<uint8_t> a(16), b(32);
    std::string e_recv, e_send, e_next;
    std::thread t0([&] {
      try {
        c0->group_start();
        c0->send(a.data(), a.size(), 1, nullptr);
        c0->group_end();
      } catch (const std::exception& e) {
        e_send = e.what();
      }
    });
    try {
      c1->group_start();
      c1->recv(b.data(), b.size(), 0, nullptr);
      c1->group_end();
    } catch (const std::exception& e) {
      e_recv = e.what();
    }
    t0.join();
    try {
      c1->group_start();
      c1->recv(b.data(), 16, 0, nullptr);
      c1->group_end();
    } catch (const std::exception& e) {
      e_next = e.what();
    }
    return std::make_tuple(e_recv, e_send, e_next);
  });
  // the bounded progress loop of the non-blocking communicators, driven by a
  // Python probe (0 done, 1 pending, 2 failed): unit tests of the state machine
  m.def("await_progress", [](const std::string& what, double limit_s, py::function probe, py::object aborted) {
    py::list gave_up;
    std::function<bool()> ab;
    if (!aborted.is_none()) ab = [aborted]() { return aborted().cast<bool>(); };
    const double ms = await_progress(
        what, limit_s,
        [&](std::string* err) {
          const int st = probe().cast<int>();
          if (st == 2) *err = "probe reported failure";
          return st == 0 ? Progress::Done : st == 1 ? Progress::Pending : Progress::Failed;
        },
        ab, [&](const std::string& why) { gave_up.append(why); });
    return ms;
  }, py::arg("what"), py::arg("limit_s"), py::arg("probe"), py::arg("aborted") = py::none());
  // HIP runtime / RCCL / HSA libraries mapped into this process (one of each
  // expected: the extension resolves to the copies torch loaded)
  m.def("last_words_arm", &last_words_arm, py::arg("fd"), py::arg("deadline_s"), py::arg("exit_code") = 3);
  m.def("last_words_set", &last_words_set, py::arg("line"), py::arg("exit_code") = -1);
  m.def("last_words_emit", &last_words_emit);
  m.def("last_words_disarm", &last_words_disarm);
  m.def("runtime_libs", []() {
    py::dict d;
    for (const char* stem : {"librccl", "libamdhip64", "libhsa-runtime64"}) d[stem] = mapped_libraries(stem);
    return d;
  });
  m.def("rccl_unique_id", []() {
    UniqueId id = rccl_unique_id();
    return py::bytes(id.data(), id.size());
  });
  m.def("rccl_version", &rccl_version);
  m.def("probe_link_rate", [](PyComm* c, int device, size_t bytes, int reps) {
    if (!c) return 0.0;
    py::gil_scoped_release nogil;
    return probe_link_rate(c->comm.get(), device, bytes, reps);
  }, py::arg("comm"), py::arg("device"), py::arg("bytes"), py::arg("reps") = 3);
  // Transport check: ring send/recv (one rank: RCCL loopback) in the
  // FrameStream pattern, every received word verified.
  m.def("comm_ring_check", [](PyComm* c, int device, size_t bytes, int frames, int streams, int iters) {
    STRIPE_CHECK(c != nullptr, "comm_ring_check needs a communicator");
    RingCheck r;
    {
      py::gil_scoped_release nogil;
      r = comm_ring_check(c->comm.get(), device, bytes, frames, streams, iters);
    }
    py::dict d;
    d["errors"] = r.errors;
    d["bytes_checked"] = r.bytes_checked;
    d["ms"] = r.ms;
    return d;
  }, py::arg("comm"), py::arg("device"), py::arg("bytes"), py::arg("frames") = 4, py::arg("streams") = 2,
     py::arg("iters") = 500);
  // A HIP stream on a hardware queue of its own: a CU-masked stream (all CUs
  // enabled) gets a dedicated HSA queue, where plain streams share the
  // GPU_MAX_HW_QUEUES queues round-robin -- two frames meant to overlap may
  // otherwise land on one queue and serialise.  Returns the handle (int).
  m.def("dedicated_stream", [](int device, int index) {
    return reinterpret_cast<uintptr_t>(Engine::dedicated_stream(device, index));
  }, py::arg("device"), py::arg("index"));
  m.def("stream_create", [](int device, bool dedicated) {
    HIP_CHECK(hipSetDevice(device));
    hipStream_t s = nullptr;
    if (dedicated) {
      int cus = 0;
      HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
      std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0xFFFFFFFFu);
      HIP_CHECK(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
    } else {
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }
    return reinterpret_cast<uintptr_t>(s);
  }, py::arg("device"), py::arg("dedicated") = true);
  m.def("stream_destroy", [](uintptr_t s) {
    HIP_CHECK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(s)));
    HIP_CHECK(hipStreamDestroy(reinterpret_cast<hipStream_t>(s)));
  }, py::arg("stream"));
  // Same-box streaming floor of the benchmark record: hand-written linear copy
  // of `bytes` rotating over `frames` buffer pairs (csrc/hip/pointwise.hip).
  m.def("copy_roofline", [](int device, int64_t bytes, int frames, int reps) {
    CopyRoofline r;
    {
      py::gil_scoped_release nogil;
      r = copy_roofline(device, bytes, frames, reps);
    }
    py::dict d;
    d["event_ms"] = r.event_ms;
    d["burst_ms"] = r.burst_ms;
    d["bytes"] = r.bytes;
    d["frames"] = r.frames;
    d["store_policy"] = r.policy == 0 ? "default" : "write-through (sc1)";
    return d;
  }, py::arg("device"), py::arg("bytes"), py::arg("frames") = 1, py::arg("reps") = 20);
  // Page-lock an existing host range (e.g. a shared-memory frame every rank
  // downloads its stripe into) so hipMemcpyAsync DMAs it without staging.
  m.def("host_register", [](uintptr_t p, size_t bytes) {
    const hipError_t e = hipHostRegister(reinterpret_cast<void*>(p), bytes, hipHostRegisterPortable);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    return true;
  });
  m.def("host_unregister", [](uintptr_t p) {
    (void)hipHostUnregister(reinterpret_cast<void*>(p));
    (void)hipGetLastError();
  });
  // Device / runtime identity for benchmark records (SURVEY §5 metrics): lets a
  // box-to-box difference be told apart from a regression.  Empty dict when no
  // HIP device is visible.
  m.def("device_info", [](int dev) {
    py::dict d;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= dev) {
      (void)hipGetLastError();
      return d;
    }
    hipDeviceProp_t pr{};
    HIP_CHECK(hipGetDeviceProperties(&pr, dev));
    int rt = 0, drv = 0;
    (void)hipRuntimeGetVersion(&rt);
    (void)hipDriverGetVersion(&drv);
    d["name"] = std::string(pr.name);
    d["gcn_arch"] = std::string(pr.gcnArchName);
    d["cu_count"] = pr.multiProcessorCount;
    d["sclk_max_mhz"] = pr.clockRate / 1000;
    d["mclk_max_mhz"] = pr.memoryClockRate / 1000;
    d["mem_bus_bits"] = pr.memoryBusWidth;
    d["hbm_gib"] = (double)pr.totalGlobalMem / (double)(1ull << 30);
    d["l2_bytes"] = pr.l2CacheSize;
    d["lds_per_cu"] = (int64_t)pr.maxSharedMemoryPerMultiProcessor;
    d["pci_bus_id"] = pr.pciBusID;
    char bdf[32] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, dev) == hipSuccess) d["pci"] = std::string(bdf);
    else (void)hipGetLastError();
    d["hip_runtime"] = rt;
    d["hip_driver"] = drv;
    d["rccl"] = rccl_version();
    return d;
  }, py::arg("device") = 0);
  m.def("make_rccl_comm", [](py::bytes uid, int rank, int world, int device) {
    std::string s(uid);
    STRIPE_CHECK(s.size() == 128, "unique id must be 128 bytes");
    UniqueId id;
    std::memcpy(id.data(), s.data(), 128);
    auto c = std::make_unique<PyComm>();
    {
      py::gil_scoped_release nogil;
      c->comm = make_rccl_comm(id, rank, world, device);
    }
    return c;
  });
  m.def("make_callback_comm", [](int rank, int world, py::function group_start, py::function send,
                                 py::function recv, py::function group_end, py::function barrier, py::object poll) {
    CallbackOps ops;
    if (!poll.is_none()) {
      py::function pf = poll;
      ops.poll = [pf]() {
        py::gil_scoped_acquire g;
        return pf().cast<int>();
      };
    }
    ops.group_start = [group_start]() {
      py::gil_scoped_acquire g;
      group_start();
    };
    ops.send = [send](const void* p, size_t n, int peer) {
      py::gil_scoped_acquire g;
      send((uintptr_t)p, n, peer);
    };
    ops.recv = [recv](void* p, size_t n, int peer) {
      py::gil_scoped_acquire g;
      recv((uintptr_t)p, n, peer);
    };
    ops.group_end = [group_end]() {
      py::gil_scoped_acquire g;
      group_end();
    };
    ops.barrier = [barrier]() {
      py::gil_scoped_acquire g;
      barrier();
    };
    auto c = std::make_unique<PyComm>();
    c->comm = make_callback_comm(rank, world, std::move(ops));
    return c;
  }, py::arg("rank"), py::arg("world"), py::arg("group_start"), py::arg("send"), py::arg("recv"),
     py::arg("group_end"), py::arg("barrier"), py::arg("poll") = py::none());

  // the callback comm's device-buffer face: takes over `host` (left empty)
  m.def("make_staged_comm", [](PyComm* host, int device) {
    STRIPE_CHECK(host && host->comm, "staged comm needs a host communicator");
    auto c = std::make_unique<PyComm>();
    c->comm = make_staged_comm(std::move(host->comm), device);
    return c;
  });
  // `world` in-process ranks over one hub (device = true: device buffers on the
  // current GPU, the `local` backend; false: host buffers).  The caller drives
  // one engine per communicator, one thread each (the engine calls release the GIL).
  m.def("make_local_comms", [](int world, bool device, double timeout_s) {
    STRIPE_CHECK(world >= 1, "make_local_comms needs world >= 1");
    auto hub = make_local_hub(world, device, timeout_s);
    py::list v;
    for (int r = 0; r < world; ++r) {
      auto c = std::make_unique<PyComm>();
      c->comm = make_local_comm(hub, r);
      v.append(py::cast(std::move(c)));
    }
    return v;
  }, py::arg("world"), py::arg("device"), py::arg("timeout_s") = 60.0);

  // ---- engine ----
  py::class_<EngineConfig>(m, "EngineConfig")
      .def(py::init<>())
      .def_readwrite("W", &EngineConfig::W)
      .def_readwrite("H", &EngineConfig::H)
      .def_readwrite("C", &EngineConfig::C)
      .def_readwrite("chain", &EngineConfig::chain)
      .def_readwrite("border", &EngineConfig::border)
      .def_readwrite("halo", &EngineConfig::halo)
      .def_readwrite("legacy_partition", &EngineConfig::legacy_partition)
      .def_readwrite("overlap", &EngineConfig::overlap)
      .def_readwrite("fuse", &EngineConfig::fuse)
      .def_readwrite("device", &EngineConfig::device)
      .def_readwrite("backend", &EngineConfig::backend)
      .def_readwrite("band", &EngineConfig::band)
      .def_readwrite("root_buffers", &EngineConfig::root_buffers)
      .def_readwrite("autotune", &EngineConfig::autotune)
      .def_readwrite("graphs", &EngineConfig::graphs)
      .def_readwrite("held_input", &EngineConfig::held_input)
      .def_readwrite("self_halo", &EngineConfig::self_halo)
      .def_readwrite("cold", &EngineConfig::cold)
      .def_readwrite("pipeline", &EngineConfig::pipeline)
      .def_readwrite("halo_depth", &EngineConfig::halo_depth)
      .def_readwrite("dist_chunks", &EngineConfig::dist_chunks)
      .def_readwrite("row_weights", &EngineConfig::row_weights);

  py::class_<PhaseTimes>(m, "PhaseTimes")
      .def_readonly("run", &PhaseTimes::run)
      .def_readonly("scatter", &PhaseTimes::scatter)
      .def_readonly("gather", &PhaseTimes::gather)
      .def_readonly("load", &PhaseTimes::load)
      .def_readonly("store", &PhaseTimes::store)
      .def_readonly("halo", &PhaseTimes::halo)
      .def_readonly("h2d", &PhaseTimes::h2d)
      .def_readonly("d2h", &PhaseTimes::d2h)
      .def_readonly("e2e", &PhaseTimes::e2e)
      .def("as_dict", [](const PhaseTimes& t) {
        py::dict d;
        d["compute"] = t.run;
        d["scatter"] = t.scatter;
        d["gather"] = t.gather;
        d["load"] = t.load;
        d["store"] = t.store;
        d["halo"] = t.halo;
        d["h2d"] = t.h2d;
        d["d2h"] = t.d2h;
        d["e2e"] = t.e2e;
        return d;
      });
  m.def("fault_point", &fault_point, py::arg("stage"), py::arg("rank"),
        "Raise if STRIPE_FAULT selects this stage/rank (failure-path tests).");
  m.def("comm_timeout_s", &comm_timeout_s);
  m.def("trace_mark", [](const std::string& s) { trace_mark(s.c_str()); });

  py::class_<Engine>(m, "Engine", py::dynamic_attr())
      .def(py::init([](const EngineConfig& cfg, PyComm* comm) {
             py::gil_scoped_release nogil;
             return std::make_unique<Engine>(cfg, comm ? comm->comm.get() : nullptr);
           }),
           py::arg("config"), py::arg("comm") = nullptr, py::keep_alive<1, 3>())
      .def_property_readonly("rank", &Engine::rank)
      .def_property_readonly("world", &Engine::world)
      .def_property_readonly("out_channels", &Engine::out_channels)
      .def_property_readonly("halo_depth", &Engine::halo_depth)
      .def_property_readonly("self_halo", &Engine::self_halo)
      .def_property_readonly("posts_halo", &Engine::posts_halo)
      .def_property("deep_steps", &Engine::deep_steps, [](Engine& e, bool on) {
        py::gil_scoped_release nogil;
        e.set_deep_steps(on);
      })
      .def_property_readonly("exchange_due", &Engine::exchange_due)
      .def("post_halo", [](Engine& e) {
        py::gil_scoped_release nogil;
        e.post_halo();
      })
      .def("run_posted", [](Engine& e) {
        py::gil_scoped_release nogil;
        e.run_posted();
      })
      .def("post_halo_ahead", [](Engine& e, uintptr_t s) {
        py::gil_scoped_release nogil;
        e.post_halo_ahead(as_stream(s));
      }, py::arg("stream"))
      .def_property_readonly("plan", [](const Engine& e) { return e.plan().describe(); })
      .def_property_readonly("partition", [](const Engine& e) { return e.partition().describe(); })
      .def_property_readonly("stripe", [](const Engine& e) {
        return py::make_tuple(e.stripe().row0, e.stripe().rows);
      })
      .def("use_external_stream", [](Engine& e, uintptr_t s) { e.use_external_stream(as_stream(s)); })
      .def("load_synthetic", [](Engine& e, uint64_t seed) {
        py::gil_scoped_release nogil;
        e.load_synthetic(seed);
      })
      .def("load_packed_ptr", [](Engine& e, uintptr_t p, bool dev) {
        py::gil_scoped_release nogil;
        e.load_packed(reinterpret_cast<const void*>(p), dev);
      })
      .def("load_packed", [](Engine& e, const U8Array& a) {
        STRIPE_CHECK((size_t)a.size() == (size_t)e.stripe().rows * e.config().W * e.config().C,
                     "stripe array has the wrong size");
        e.load_packed(a.data(), false);
        e.synchronize();
      })
      .def("load_held_packed_ptr", [](Engine& e, uintptr_t p, bool dev) {
        py::gil_scoped_release nogil;
        e.load_held_packed(reinterpret_cast<const void*>(p), dev);
      })
      .def("load_held_packed", [](Engine& e, const U8Array& a) {
        STRIPE_CHECK((size_t)a.size() == (size_t)e.stripe().rows * e.config().W * e.config().C,
                     "held stripe array has the wrong size");
        e.load_held_packed(a.data(), false);
        e.synchronize();
      })
      .def("load_root", [](Engine& e, const U8Array& a) {
        e.load_root(a.data(), false);
        e.synchronize();
      })
      .def("load_root_synthetic", [](Engine& e, uint64_t seed) {
        py::gil_scoped_release nogil;
        e.load_root_synthetic(seed);
      })
      .def("load_root_ptr", [](Engine& e, uintptr_t p, bool dev) { e.load_root(reinterpret_cast<const void*>(p), dev); })
      .def("scatter", [](Engine& e) {
        py::gil_scoped_release nogil;
        e.scatter();
      })
      .def("run", [](Engine& e, int it) {
        py::gil_scoped_release nogil;
        e.run(it);
      }, py::arg("iterations") = 1)
      .def("rewind", &Engine::rewind)
      .def("histogram", [](Engine& e, bool global) {
        Histogram h;
        {
          py::gil_scoped_release nogil;
          h = e.histogram(global);
        }
        return hist_to_numpy(h);
      }, py::arg("global_") = true,
           "int64 counts (C, 256) of the current image: this rank's rows (global_=False) or the sum over all "
           "ranks (a collective every rank calls)")
      .def("alloc_host_io", &Engine::alloc_host_io)
      .def("host_input", [](py::object self) {
        Engine& e = self.cast<Engine&>();
        STRIPE_CHECK(e.host_in() != nullptr, "call alloc_host_io() first");
        const auto& c = e.config();
        std::vector<py::ssize_t> shape = {e.stripe().rows, c.W};
        if (e.plan().cin != 1) shape.push_back(e.plan().cin);
        return py::array_t<uint8_t>(shape, e.host_in(), self);  // pinned, zero-copy view
      })
      .def("host_output", [](py::object self) {
        Engine& e = self.cast<Engine&>();
        STRIPE_CHECK(e.host_out() != nullptr, "call alloc_host_io() first");
        const auto& c = e.config();
        std::vector<py::ssize_t> shape = {e.stripe().rows, c.W};
        if (e.plan().cout != 1) shape.push_back(e.plan().cout);
        return py::array_t<uint8_t>(shape, e.host_out(), self);
      })
      .def("run_e2e", [](Engine& e, int chunks) {
        py::gil_scoped_release nogil;
        e.run_e2e(chunks);
      }, py::arg("chunks") = 8)
      .def_property_readonly("bands", &Engine::bands)
      .def_property_readonly("caps", &Engine::caps)
      .def_property_readonly("policies", &Engine::policies)
      .def_property_readonly("orders", &Engine::orders)
      .def("run_timed", [](Engine& e, int it, int per, bool rewind_each) {
        py::gil_scoped_release rel;
        return e.run_timed(it, per, rewind_each);
      }, py::arg("iterations"), py::arg("per") = 1, py::arg("rewind_each") = false)
      .def("gather", [](Engine& e) {
        py::gil_scoped_release nogil;
        e.gather();
      })
      .def("run_dist", [](Engine& e, int chunks) {
        py::gil_scoped_release nogil;
        e.run_dist(chunks);
      }, py::arg("chunks") = 8)
      .def("dist_chunks", &Engine::dist_chunks, py::arg("chunks"))
      .def("run_to_host_ptr", [](Engine& e, uintptr_t p, int chunks) {
        py::gil_scoped_release nogil;
        e.run_to_host(reinterpret_cast<void*>(p), chunks);
      }, py::arg("ptr"), py::arg("chunks") = 8)
      .def("set_tuning", &Engine::set_tuning, py::arg("bands"), py::arg("caps"),
           py::arg("policies") = std::vector<int>{}, py::arg("orders") = std::vector<int>{})
      .def("tune", [](Engine& e) {
        py::gil_scoped_release nogil;
        e.tune();
      })
      .def("set_tune_streams", &Engine::set_tune_streams, py::arg("n"),
           "Streams a cold stripe's steps alternate over (1 or 2): the cold tune times its candidates that way.")
      .def("set_tune_reduce", [](Engine& e, py::object f) {
        if (f.is_none()) {
          e.set_tune_reduce({});
          return;
        }
        // called from the (GIL-released) autotune: take the GIL for the call
        // (the function may be dropped where the GIL is released: release the
        // Python reference under the GIL)
        std::shared_ptr<py::object> fn(new py::object(f), [](py::object* o) {
          py::gil_scoped_acquire gil;
          delete o;
        });
        e.set_tune_reduce([fn](float v) {
          py::gil_scoped_acquire gil;
          return (*fn)(v).cast<float>();
        });
      }, py::arg("reduce"),
           "Collective autotune: each candidate's median (ms) goes through reduce(v) -> float (e.g. max over "
           "ranks) before the comparison; None restores the per-rank tune.  Every rank must then tune together.")
      .def_property_readonly("dist_direct", &Engine::dist_direct)
      .def("store_packed_ptr", [](Engine& e, uintptr_t p, bool dev) {
        py::gil_scoped_release nogil;
        e.store_packed(reinterpret_cast<void*>(p), dev);
      })
      .def("store_packed", [](Engine& e) {
        const auto& c = e.config();
        std::vector<py::ssize_t> shape = {e.stripe().rows, c.W};
        if (e.out_channels() != 1) shape.push_back(e.out_channels());
        U8Array a(shape);
        {
          py::gil_scoped_release nogil;
          e.store_packed(a.mutable_data(), false);
          e.synchronize();
        }
        return a;
      })
      .def("store_root", [](Engine& e) {
        const auto& c = e.config();
        std::vector<py::ssize_t> shape = {c.H, c.W};
        if (e.out_channels() != 1) shape.push_back(e.out_channels());
        U8Array a(shape);
        {
          py::gil_scoped_release nogil;
          e.store_root(a.mutable_data(), false);
          e.synchronize();
        }
        return a;
      })
      .def("store_root_ptr", [](Engine& e, uintptr_t p, bool dev) { e.store_root(reinterpret_cast<void*>(p), dev); })
      .def("synchronize", [](Engine& e) {
        py::gil_scoped_release nogil;
        e.synchronize();
      })
      .def_property_readonly("times", [](const Engine& e) { return e.times(); })
      .def_property("stage_timing", &Engine::stage_timing, &Engine::set_stage_timing)
      // "serial" | "overlap" | "pipeline": set = request, get = what run(1) does
      .def_property(
          "halo_schedule",
          [](const Engine& e) {
            static const char* names[] = {"serial", "overlap", "pipeline"};
            return std::string(names[e.halo_schedule()]);
          },
          [](Engine& e, const std::string& s) {
            const int v = s == "serial" ? 0 : s == "overlap" ? 1 : s == "pipeline" ? 2 : -1;
            STRIPE_CHECK(v >= 0, "halo schedule must be serial, overlap or pipeline, got '" << s << "'");
            e.set_halo_schedule(v);
          })
      .def_property_readonly("graph_launches", &Engine::graph_launches);

  m.def("run_local_group", [](const EngineConfig& cfg, int world, const U8Array& a, int iterations) {
    Image img = image_from_numpy(a);
    Image out;
    {
      py::gil_scoped_release nogil;
      out = run_local_group(cfg, world, img, iterations);
    }
    return image_to_numpy(out);
  }, py::arg("config"), py::arg("world"), py::arg("image"), py::arg("iterations") = 1);

  // one process driving several GPUs: one thread per rank, an in-process RCCL
  // communicator over `devices` (ncclCommInitAll), the same run_rank flow
  m.def("run_rccl_group", [](const EngineConfig& cfg, const std::vector<int>& devices, const U8Array& a,
                             int iterations) {
    Image img = image_from_numpy(a);
    Image out;
    {
      py::gil_scoped_release nogil;
      auto owned = make_rccl_comms_all(devices);
      std::vector<Comm*> comms;
      for (auto& c : owned) comms.push_back(c.get());
      out = run_group(cfg, comms, devices, img, iterations);
    }
    return image_to_numpy(out);
  }, py::arg("config"), py::arg("devices"), py::arg("image"), py::arg("iterations") = 1);

  m.attr("kMarginBytes") = kMarginBytes;
  m.attr("kMaxRadius") = kMaxRadius;
  m.def("padded_pitch", &padded_pitch);
}
