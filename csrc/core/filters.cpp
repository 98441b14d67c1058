// Filter catalogue and pointwise numerics.
#include "stripe/filters.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>

#include "stripe/stencil_defs.h"

namespace stripe {

const char* border_name(Border b) {
  switch (b) {
    case Border::Reflect101: return "reflect101";
    case Border::Replicate: return "replicate";
    case Border::Constant: return "constant";
    case Border::Skip: return "skip";
  }
  return "?";
}

Border parse_border(const std::string& s) {
  if (s == "reflect101" || s == "reflect" || s == "default") return Border::Reflect101;
  if (s == "replicate" || s == "clamp") return Border::Replicate;
  if (s == "constant" || s == "zero") return Border::Constant;
  if (s == "skip" || s == "legacy") return Border::Skip;
  fail("unknown border mode '" + s + "' (reflect101|replicate|constant|skip)");
}

namespace {

template <class F>
StencilInfo make_info(StencilId id, const char* name) {
  StencilInfo s;
  s.id = id;
  s.name = name;
  s.K = F::K;
  s.separable = F::SEP;
  s.sobel = F::SOBEL;
  if constexpr (F::SOBEL) s.l2 = F::L2;
  s.div = F::DIV;
  for (int dy = 0; dy < F::K; ++dy)
    for (int dx = 0; dx < F::K; ++dx) s.w.push_back(F::w(dy, dx));
  return s;
}

template <class F>
StencilInfo make_sep(StencilId id, const char* name) {
  StencilInfo s = make_info<F>(id, name);
  for (int i = 0; i < F::K; ++i) s.w1.push_back(F::g(i));
  return s;
}

template <class F>
StencilInfo make_rank(StencilId id, const char* name) {
  static_assert(!F::SEP && !F::SOBEL && F::DIV == 1 && F::RANK != 0, "rank filter definition");
  StencilInfo s;
  s.id = id;
  s.name = name;
  s.K = F::K;
  s.separable = false;
  s.sobel = false;
  s.div = 1;
  s.rank = (Rank)F::RANK;
  return s;
}

template <class F>
StencilInfo make_bilateral(StencilId id, const char* name) {
  static_assert(!F::SEP && !F::SOBEL && F::DIV == 1 && F::BILATERAL != 0, "bilateral filter definition");
  StencilInfo s = make_info<F>(id, name);  // w: the spatial weights
  for (int i = 0; i < F::K; ++i) s.w1.push_back(F::g(i));
  s.bilateral = true;
  return s;
}

const std::vector<StencilInfo>& table() {
  static const std::vector<StencilInfo> t = [] {
    std::vector<StencilInfo> v((size_t)StencilId::kCount);
    v[(int)StencilId::Emboss3] = make_info<sdef::Emboss3>(StencilId::Emboss3, "emboss3");
    v[(int)StencilId::Emboss5] = make_info<sdef::Emboss5>(StencilId::Emboss5, "emboss5");
    v[(int)StencilId::Gaussian3] = make_sep<sdef::Gaussian3>(StencilId::Gaussian3, "gaussian3");
    v[(int)StencilId::Gaussian5] = make_sep<sdef::Gaussian5>(StencilId::Gaussian5, "gaussian5");
    v[(int)StencilId::Gaussian7] = make_sep<sdef::Gaussian7>(StencilId::Gaussian7, "gaussian7");
    v[(int)StencilId::Box3] = make_sep<sdef::Box3>(StencilId::Box3, "box3");
    v[(int)StencilId::Box5] = make_sep<sdef::Box5>(StencilId::Box5, "box5");
    v[(int)StencilId::Sharpen] = make_info<sdef::Sharpen>(StencilId::Sharpen, "sharpen");
    v[(int)StencilId::Laplace] = make_info<sdef::Laplace>(StencilId::Laplace, "laplace");
    v[(int)StencilId::Sobel] = make_info<sdef::Sobel>(StencilId::Sobel, "sobel");
    v[(int)StencilId::SobelL2] = make_info<sdef::SobelL2>(StencilId::SobelL2, "sobel_l2");
    v[(int)StencilId::Median3] = make_rank<sdef::Median3>(StencilId::Median3, "median3");
    v[(int)StencilId::Median5] = make_rank<sdef::Median5>(StencilId::Median5, "median5");
    v[(int)StencilId::Erode3] = make_rank<sdef::Erode3>(StencilId::Erode3, "erode3");
    v[(int)StencilId::Erode5] = make_rank<sdef::Erode5>(StencilId::Erode5, "erode5");
    v[(int)StencilId::Dilate3] = make_rank<sdef::Dilate3>(StencilId::Dilate3, "dilate3");
    v[(int)StencilId::Dilate5] = make_rank<sdef::Dilate5>(StencilId::Dilate5, "dilate5");
    v[(int)StencilId::Bilateral3] = make_bilateral<sdef::Bilateral3>(StencilId::Bilateral3, "bilateral3");
    v[(int)StencilId::Bilateral5] = make_bilateral<sdef::Bilateral5>(StencilId::Bilateral5, "bilateral5");
    return v;
  }();
  return t;
}

std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out;
  std::string cur;
  for (char c : s) {
    if (c == sep) {
      out.push_back(cur);
      cur.clear();
    } else {
      cur.push_back(c);
    }
  }
  out.push_back(cur);
  return out;
}

std::string trim(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b && isspace((unsigned char)s[a])) ++a;
  while (b > a && isspace((unsigned char)s[b - 1])) --b;
  return s.substr(a, b - a);
}

double parse_num(const std::string& s, const std::string& ctx) {
  char* end = nullptr;
  double v = std::strtod(s.c_str(), &end);
  if (s.empty() || end == s.c_str() || *end != '\0') fail("bad number '" + s + "' in '" + ctx + "'");
  return v;
}

// Quantise a colour matrix (row-major m, offsets b) into op.cm (filters.h).
void set_color_matrix(Op& op, const double (&m)[9], const double (&b)[3], const std::string& tok) {
  op.kind = OpKind::ColorMatrix;
  for (int i = 0; i < 9; ++i) {
    const double q = std::nearbyint(m[i] * 4096.0);
    STRIPE_CHECK(std::fabs(q) <= 32767, "'" << tok << "': coefficient " << m[i] << " out of range (|m| < 8)");
    op.cm[i] = (int)q;
  }
  for (int c = 0; c < 3; ++c) {
    STRIPE_CHECK(std::fabs(b[c]) <= 2048, "'" << tok << "': offset " << b[c] << " out of range (|b| <= 2048)");
    op.cm[9 + c] = (int)std::nearbyint(b[c] * 4096.0);
  }
}

// A Q12 coefficient as the decimal that parses back to it (q / 4096 is exact in
// double and has at most 12 fractional digits).
std::string q12_text(int q) {
  std::ostringstream os;
  os.precision(17);
  os << q / 4096.0;
  return os.str();
}

// The shortest decimal that strtod reads back as exactly v: plain digits where
// a few decimals do ("20", "3.5"), 17 significant digits otherwise.
std::string shortest_text(double v) {
  char buf[64];
  for (int dec = 0; dec <= 17; ++dec) {
    std::snprintf(buf, sizeof buf, "%.*f", dec, v);
    if (std::strtod(buf, nullptr) == v) return buf;
  }
  std::snprintf(buf, sizeof buf, "%.17g", v);
  return buf;
}

}  // namespace

std::array<uint8_t, 256> bilateral_range_table(double S) {
  STRIPE_CHECK(S > 0.0, "bilateral range sigma must be positive");
  std::array<uint8_t, 256> r{};
  for (int d = 0; d < 256; ++d)
    r[(size_t)d] = (uint8_t)std::nearbyint(255.0 * std::exp(-(double)(d * d) / (2.0 * S * S)));
  return r;
}

const char* combine_name(CombineKind k) {
  static const char* names[] = {"add", "sub", "rsub", "absdiff", "min", "max", "lincomb", "above"};
  return (int)k >= 0 && (int)k < (int)CombineKind::kCount ? names[(int)k] : "?";
}

const StencilInfo& stencil_info(StencilId id) {
  STRIPE_CHECK((int)id >= 0 && (int)id < (int)StencilId::kCount, "bad stencil id");
  return table()[(int)id];
}

bool stencil_from_name(const std::string& name, StencilId* out) {
  static const std::map<std::string, StencilId> alias = {
      {"emboss", StencilId::Emboss3},    {"emboss3", StencilId::Emboss3},
      {"emboss5", StencilId::Emboss5},   {"gaussian", StencilId::Gaussian5},
      {"gaussian3", StencilId::Gaussian3}, {"gaussian5", StencilId::Gaussian5},
      {"gaussian7", StencilId::Gaussian7}, {"gauss5", StencilId::Gaussian5},
      {"box3", StencilId::Box3},         {"box5", StencilId::Box5},
      {"sharpen", StencilId::Sharpen},   {"laplace", StencilId::Laplace},
      {"laplacian", StencilId::Laplace}, {"sobel", StencilId::Sobel},
      {"edge", StencilId::Sobel},        {"sobel_l2", StencilId::SobelL2},
      {"magnitude", StencilId::SobelL2},
      {"median", StencilId::Median3},    {"median3", StencilId::Median3},
      {"median5", StencilId::Median5},   {"erode", StencilId::Erode3},
      {"erode3", StencilId::Erode3},     {"erode5", StencilId::Erode5},
      {"dilate", StencilId::Dilate3},    {"dilate3", StencilId::Dilate3},
      {"dilate5", StencilId::Dilate5},
      {"bilateral", StencilId::Bilateral5}, {"bilateral3", StencilId::Bilateral3},
      {"bilateral5", StencilId::Bilateral5},
  };
  auto it = alias.find(name);
  if (it == alias.end()) return false;
  *out = it->second;
  return true;
}

const char* rank_name(Rank r) {
  switch (r) {
    case Rank::None: return "none";
    case Rank::Min: return "min";
    case Rank::Max: return "max";
    case Rank::Median: return "median";
  }
  return "?";
}

int Op::radius() const {
  if (kind == OpKind::Stencil) return stencil_info(sid).K / 2;
  if (kind == OpKind::Conv) return K / 2;
  return 0;
}

int Op::channels_out(int cin) const {
  if (kind == OpKind::Gray) return 1;
  if (kind == OpKind::Expand) return 3;
  return cin;
}

std::vector<double> gaussian_1d(int K, double sigma) {
  STRIPE_CHECK(K >= 1 && K % 2 == 1, "gaussian size must be odd, got " << K);
  if (sigma <= 0) sigma = 0.3 * ((K - 1) * 0.5 - 1) + 0.8;  // OpenCV getGaussianKernel rule
  std::vector<double> g(K);
  double s = 0;
  const int R = K / 2;
  for (int i = 0; i < K; ++i) {
    const double x = i - R;
    g[i] = std::exp(-(x * x) / (2 * sigma * sigma));
    s += g[i];
  }
  for (auto& v : g) v /= s;
  return g;
}

static Op make_conv_blur(int K, double sigma, const std::string& text) {
  STRIPE_CHECK(K >= 3 && K % 2 == 1 && K / 2 <= kMaxRadius,
               "blur:K needs odd K in [3, " << 2 * kMaxRadius + 1 << "], got " << K);
  Op op;
  op.kind = OpKind::Conv;
  op.K = K;
  auto g = gaussian_1d(K, sigma);
  op.weights.resize((size_t)K * K);
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) op.weights[(size_t)i * K + j] = (float)(g[i] * g[j]);
  op.sep_h.resize((size_t)K);
  for (int i = 0; i < K; ++i) op.sep_h[(size_t)i] = (float)g[i];
  op.sep_v = op.sep_h;
  op.text = text;
  return op;
}

// Trailing ":exact" / ":lsb" of a float conv token (removed from parts):
// 3 = exact (the default), 2 = every output within 1 LSB of the f64 result.
static int take_precision(std::vector<std::string>& parts) {
  if (parts.size() < 2) return 3;
  const std::string last = trim(parts.back());
  if (last != "exact" && last != "lsb") return 3;
  parts.pop_back();
  return last == "lsb" ? 2 : 3;
}

std::vector<Op> parse_chain(const std::string& spec_in) {
  const std::string spec = trim(spec_in);
  std::vector<Op> ops;
  STRIPE_CHECK(!spec.empty(), "empty filter chain");
  for (const std::string& raw : split(spec, ',')) {
    std::string tok = trim(raw);
    STRIPE_CHECK(!tok.empty(), "empty token in chain '" << spec << "'");
    // presets (SURVEY Appendix A "presets") expand in place; halo/partition
    // flags of a preset are applied by the callers (CLI / models.PRESETS)
    if (tok == "ref-gpu" || tok == "ref-cpu") {
      auto sub = parse_chain(tok == "ref-gpu" ? "gray:ref,contrast:3.5,emboss3@skip"
                                              : "gray:bt601,contrast:3:cv,emboss3");
      ops.insert(ops.end(), sub.begin(), sub.end());
      continue;
    }
    Op op;
    // optional per-op border override: name[:args]@border
    auto at = tok.find('@');
    if (at != std::string::npos) {
      op.has_border = true;
      op.border = parse_border(tok.substr(at + 1));
      tok = tok.substr(0, at);
    }
    auto parts = split(tok, ':');
    const std::string name = parts[0];
    StencilId sid;
    // rank filters come in sizes 3 and 5 only: say so, rather than "unknown filter"
    for (const char* fam : {"median", "erode", "dilate", "open", "close"}) {
      const std::string f = fam;
      if (name.compare(0, f.size(), f) != 0) continue;
      const std::string sz = name.substr(f.size());
      const bool sugar = f == "open" || f == "close";
      STRIPE_CHECK(sz == "3" || sz == "5" || (sz.empty() && !sugar),
                   "'" << name << "': " << f << " takes a window size of 3 or 5 (" << f << "3, " << f << "5)");
      STRIPE_CHECK(parts.size() == 1, "'" << tok << "': " << f << " takes no arguments");
    }
    if (name == "open3" || name == "open5" || name == "close3" || name == "close5") {
      // morphological opening = erode then dilate, closing = dilate then erode;
      // an @border suffix applies to both ops
      const std::string k(1, name.back());
      const std::string suffix = op.has_border ? std::string("@") + border_name(op.border) : "";
      const bool open = name[0] == 'o';
      auto sub = parse_chain((open ? "erode" : "dilate") + k + suffix + "," + (open ? "dilate" : "erode") + k + suffix);
      ops.insert(ops.end(), sub.begin(), sub.end());
      continue;
    }
    // two-image sugar (filters.h): hold, the stencils with the token's @border, one combine op
    {
      const std::string suffix = op.has_border ? std::string("@") + border_name(op.border) : "";
      std::string expansion;
      for (const char* fam : {"gradient", "tophat", "blackhat"}) {
        const std::string f = fam;
        if (name.compare(0, f.size(), f) != 0) continue;
        const std::string k = name.substr(f.size());
        STRIPE_CHECK(k == "3" || k == "5",
                     "'" << name << "': " << f << " takes a window size of 3 or 5 (" << f << "3, " << f << "5)");
        STRIPE_CHECK(parts.size() == 1, "'" << tok << "': " << f << " takes no arguments");
        if (f == "gradient") expansion = "hold,dilate" + k + suffix + ",swap,erode" + k + suffix + ",sub";
        else if (f == "tophat") expansion = "hold,open" + k + suffix + ",sub";
        else expansion = "hold,close" + k + suffix + ",rsub";
      }
      if (name == "unsharp") {
        // unsharp[:S[:K]]  x + S (x - gaussianK(x)) in Q12: qa = -nearbyint(4096 S) on the blur, 4096 - qa on x
        STRIPE_CHECK(parts.size() <= 3, "'" << tok << "': unsharp syntax: unsharp[:S[:K]]");
        const double S = parts.size() > 1 ? parse_num(trim(parts[1]), tok) : 1.0;
        const std::string k = parts.size() > 2 ? trim(parts[2]) : "5";
        STRIPE_CHECK(S > 0.0 && S < 7.0, "'" << tok << "': unsharp amount must be in (0, 7)");
        STRIPE_CHECK(k == "3" || k == "5" || k == "7", "'" << tok << "': unsharp blurs with gaussian3, 5 or 7");
        const int qa = -(int)std::nearbyint(4096.0 * S);
        STRIPE_CHECK(qa != 0 && 4096 - qa <= 32767, "'" << tok << "': unsharp amount must be in (0, 7)");
        expansion = "hold,gaussian" + k + suffix + ",lincomb:" + q12_text(qa) + ":" + q12_text(4096 - qa);
      }
      if (name == "threshold" && parts.size() > 1 && trim(parts[1]) == "adaptive") {
        // threshold:adaptive:K[:C]  x > boxK(x) - C
        STRIPE_CHECK(parts.size() == 3 || parts.size() == 4,
                     "'" << tok << "': adaptive threshold syntax: threshold:adaptive:K[:C]");
        const std::string k = trim(parts[2]);
        STRIPE_CHECK(k == "3" || k == "5", "'" << tok << "': threshold:adaptive takes a window size of 3 or 5");
        const double Cd = parts.size() > 3 ? parse_num(trim(parts[3]), tok) : 0.0;
        STRIPE_CHECK(Cd == std::nearbyint(Cd) && std::fabs(Cd) <= 255,
                     "'" << tok << "': threshold:adaptive offset must be an integer in [-255, 255]");
        expansion = "hold,box" + k + suffix + ",above:" + std::to_string((int)Cd);
      }
      if (!expansion.empty()) {
        auto sub = parse_chain(expansion);
        ops.insert(ops.end(), sub.begin(), sub.end());
        continue;
      }
    }
    if (name == "hold" || name == "save" || name == "swap") {
      STRIPE_CHECK(parts.size() == 1, "'" << tok << "': " << name << " takes no arguments");
      op.kind = name == "swap" ? OpKind::Swap : OpKind::Hold;
      op.text = name == "swap" ? "swap" : "hold";
    } else if (name == "add" || name == "sub" || name == "rsub" || name == "absdiff" || name == "min" ||
               name == "max") {
      STRIPE_CHECK(parts.size() == 1, "'" << tok << "': " << name << " takes no arguments");
      op.kind = OpKind::Combine;
      op.comb = name == "add"    ? CombineKind::Add
                : name == "sub"  ? CombineKind::Sub
                : name == "rsub" ? CombineKind::RSub
                : name == "min"  ? CombineKind::Min
                : name == "max"  ? CombineKind::Max
                                 : CombineKind::AbsDiff;
      op.text = name;
    } else if (name == "lincomb" || name == "blend") {
      // lincomb:a:b[:c] / blend:t  (Q12, filters.h); both spelled canonically as lincomb
      op.kind = OpKind::Combine;
      op.comb = CombineKind::LinComb;
      if (name == "blend") {
        STRIPE_CHECK(parts.size() == 2, "'" << tok << "': blend needs a weight, e.g. blend:0.25");
        const double t = parse_num(trim(parts[1]), tok);
        STRIPE_CHECK(t >= 0.0 && t <= 1.0, "'" << tok << "': blend weight must be in [0, 1]");
        op.cq[0] = (int)std::nearbyint(4096.0 * t);
        op.cq[1] = 4096 - op.cq[0];
      } else {
        STRIPE_CHECK(parts.size() == 3 || parts.size() == 4, "'" << tok << "': lincomb syntax: lincomb:a:b[:c]");
        for (int i = 0; i < 2; ++i) {
          const double a = parse_num(trim(parts[(size_t)i + 1]), tok);
          const double q = std::nearbyint(a * 4096.0);
          STRIPE_CHECK(std::fabs(q) <= 32767, "'" << tok << "': coefficient " << a << " out of range (|a| < 8)");
          op.cq[i] = (int)q;
        }
        if (parts.size() == 4) {
          const double c = parse_num(trim(parts[3]), tok);
          STRIPE_CHECK(std::fabs(c) <= 2048, "'" << tok << "': offset " << c << " out of range (|c| <= 2048)");
          op.cq[2] = (int)std::nearbyint(c * 4096.0);
        }
      }
      op.text = "lincomb:" + q12_text(op.cq[0]) + ":" + q12_text(op.cq[1]) +
                (op.cq[2] != 0 ? ":" + q12_text(op.cq[2]) : std::string());
    } else if (name == "above") {
      STRIPE_CHECK(parts.size() <= 2, "'" << tok << "': above syntax: above[:d]");
      const double d = parts.size() > 1 ? parse_num(trim(parts[1]), tok) : 0.0;
      STRIPE_CHECK(d == std::nearbyint(d) && std::fabs(d) <= 255,
                   "'" << tok << "': above takes an integer offset in [-255, 255]");
      op.kind = OpKind::Combine;
      op.comb = CombineKind::Above;
      op.ival = (int)d;
      op.text = op.ival != 0 ? "above:" + std::to_string(op.ival) : std::string("above");
    } else if (name == "gray" || name == "grayscale" || name == "grey") {
      op.kind = OpKind::Gray;
      op.gray = GrayMode::BT601;
      if (parts.size() > 1) {
        if (parts[1] == "ref") op.gray = GrayMode::Ref;
        else if (parts[1] == "bt601" || parts[1] == "cv") op.gray = GrayMode::BT601;
        else fail("gray mode must be ref|bt601, got '" + parts[1] + "'");
      }
      op.text = op.gray == GrayMode::Ref ? "gray:ref" : "gray:bt601";
    } else if (name == "contrast") {
      op.kind = OpKind::Contrast;
      op.fval = parts.size() > 1 ? (float)parse_num(parts[1], tok) : 3.5f;
      op.round = RoundMode::Trunc;
      if (parts.size() > 2) {
        if (parts[2] == "cv" || parts[2] == "round") op.round = RoundMode::Nearest;
        else if (parts[2] == "ref" || parts[2] == "trunc") op.round = RoundMode::Trunc;
        else fail("contrast rounding must be ref|cv, got '" + parts[2] + "'");
      }
      std::ostringstream os;
      os << "contrast:" << op.fval << (op.round == RoundMode::Nearest ? ":cv" : "");
      op.text = os.str();
    } else if (name == "invert" || name == "negate") {
      op.kind = OpKind::Invert;
      op.text = "invert";
    } else if (name == "brightness" || name == "bright") {
      op.kind = OpKind::Brightness;
      STRIPE_CHECK(parts.size() > 1, "brightness needs a delta, e.g. brightness:40");
      op.ival = (int)parse_num(parts[1], tok);
      op.text = "brightness:" + std::to_string(op.ival);
    } else if (name == "threshold" && parts.size() > 1 && trim(parts[1]) == "otsu") {
      // Otsu's level of the global histogram, chosen at run time (filters.h)
      STRIPE_CHECK(parts.size() == 2, "'" << tok << "': threshold:otsu takes no further arguments");
      op.kind = OpKind::Stat;
      op.stat = StatKind::Otsu;
      op.text = "threshold:otsu";
    } else if (name == "threshold") {
      op.kind = OpKind::Threshold;
      op.ival = parts.size() > 1 ? (int)parse_num(parts[1], tok) : 128;
      op.text = "threshold:" + std::to_string(op.ival);
    } else if (name == "equalize") {
      STRIPE_CHECK(parts.size() == 1, "'" << tok << "': equalize takes no arguments");
      op.kind = OpKind::Stat;
      op.stat = StatKind::Equalize;
      op.text = "equalize";
    } else if (name == "autocontrast") {
      // autocontrast[:P]  P percent of the pixels clipped at each end, in hundredths
      STRIPE_CHECK(parts.size() <= 2, "'" << tok << "': autocontrast syntax: autocontrast[:P]");
      const double P = parts.size() > 1 ? parse_num(trim(parts[1]), tok) : 0.0;
      STRIPE_CHECK(P >= 0.0 && P < 50.0, "'" << tok << "': autocontrast clips 0 <= P < 50 percent per end");
      op.kind = OpKind::Stat;
      op.stat = StatKind::AutoContrast;
      op.ival = (int)std::nearbyint(100.0 * P);
      STRIPE_CHECK(op.ival < 5000, "'" << tok << "': autocontrast clips 0 <= P < 50 percent per end");
      std::ostringstream os;
      os << "autocontrast";
      if (op.ival != 0) os << ":" << op.ival / 100.0;
      op.text = os.str();
    } else if (name == "expand" || name == "gray2rgb") {
      op.kind = OpKind::Expand;
      op.text = "expand";
    } else if (name == "blur" || name == "gblur") {
      // blur:K[:sigma][:exact|:lsb]
      const int digits = take_precision(parts);
      STRIPE_CHECK(parts.size() <= 3, "blur syntax: blur:K[:sigma][:exact|:lsb]");
      const int K = parts.size() > 1 ? (int)parse_num(parts[1], tok) : 31;
      const double sigma = parts.size() > 2 ? parse_num(parts[2], tok) : 0.0;
      Op c = make_conv_blur(K, sigma, tok);
      c.has_border = op.has_border;
      c.border = op.border;
      c.conv_digits = digits;
      op = c;
    } else if (name == "conv") {
      // conv:K:w00;w01;...[:exact|:lsb]  (K*K weights, row-major, correlation)
      STRIPE_CHECK(parts.size() == 3 || parts.size() == 4, "conv syntax: conv:K:w0;w1;...;w(K*K-1)[:exact|:lsb]");
      if (parts.size() == 4) {
        const std::string prec = trim(parts[3]);
        STRIPE_CHECK(prec == "exact" || prec == "lsb", "conv precision must be exact or lsb, got '" << prec << "'");
        op.conv_digits = prec == "lsb" ? 2 : 3;
      }
      op.kind = OpKind::Conv;
      op.K = (int)parse_num(parts[1], tok);
      STRIPE_CHECK(op.K >= 1 && op.K % 2 == 1 && op.K / 2 <= kMaxRadius, "conv K must be odd <= 33");
      for (const auto& w : split(parts[2], ';')) op.weights.push_back((float)parse_num(trim(w), tok));
      STRIPE_CHECK((int)op.weights.size() == op.K * op.K,
                   "conv:" << op.K << " needs " << op.K * op.K << " weights, got " << op.weights.size());
      op.text = tok;
    } else if (name == "sepconv") {
      // sepconv:K:h0;...;h(K-1):v0;...;v(K-1)[:exact|:lsb]  rank-one KxK correlation
      // weights[dy][dx] = v[dy] * h[dx] (separable MFMA path on the GPU)
      op.conv_digits = take_precision(parts);
      STRIPE_CHECK(parts.size() == 4, "sepconv syntax: sepconv:K:h0;...;h(K-1):v0;...;v(K-1)[:exact|:lsb]");
      op.kind = OpKind::Conv;
      op.K = (int)parse_num(parts[1], tok);
      STRIPE_CHECK(op.K >= 1 && op.K % 2 == 1 && op.K / 2 <= kMaxRadius, "sepconv K must be odd <= 33");
      for (const auto& w : split(parts[2], ';')) op.sep_h.push_back((float)parse_num(trim(w), tok));
      for (const auto& w : split(parts[3], ';')) op.sep_v.push_back((float)parse_num(trim(w), tok));
      STRIPE_CHECK((int)op.sep_h.size() == op.K && (int)op.sep_v.size() == op.K,
                   "sepconv:" << op.K << " needs " << op.K << " horizontal and " << op.K << " vertical weights");
      op.weights.resize((size_t)op.K * op.K);
      for (int i = 0; i < op.K; ++i)
        for (int j = 0; j < op.K; ++j) op.weights[(size_t)i * op.K + j] = op.sep_v[(size_t)i] * op.sep_h[(size_t)j];
      op.text = tok;
    } else if (name == "colormatrix") {
      // colormatrix:m00;m01;m02;m10;...;m22[:b0;b1;b2]  row-major, out_c = sum_k m[c][k] in_k + b_c
      STRIPE_CHECK(parts.size() == 2 || parts.size() == 3,
                   "'" << tok << "': colormatrix syntax: colormatrix:m00;m01;...;m22[:b0;b1;b2]");
      double m[9], b[3] = {0, 0, 0};
      const auto ms = split(parts[1], ';');
      STRIPE_CHECK(ms.size() == 9, "'" << tok << "': colormatrix needs 9 coefficients, got " << ms.size());
      for (int i = 0; i < 9; ++i) m[i] = parse_num(trim(ms[(size_t)i]), tok);
      if (parts.size() == 3) {
        const auto bs = split(parts[2], ';');
        STRIPE_CHECK(bs.size() == 3, "'" << tok << "': colormatrix takes 3 offsets, got " << bs.size());
        for (int i = 0; i < 3; ++i) b[i] = parse_num(trim(bs[(size_t)i]), tok);
      }
      set_color_matrix(op, m, b, tok);
      op.text = tok;
    } else if (name == "sepia") {
      STRIPE_CHECK(parts.size() == 1, "'" << tok << "': sepia takes no arguments");
      const double m[9] = {.393, .769, .189, .349, .686, .168, .272, .534, .131}, b[3] = {0, 0, 0};
      set_color_matrix(op, m, b, tok);
      op.text = "sepia";
    } else if (name == "swaprb" || name == "bgr") {
      STRIPE_CHECK(parts.size() == 1, "'" << tok << "': " << name << " takes no arguments");
      const double m[9] = {0, 0, 1, 0, 1, 0, 1, 0, 0}, b[3] = {0, 0, 0};
      set_color_matrix(op, m, b, tok);
      op.text = "swaprb";
    } else if (name == "saturation" || name == "saturate") {
      STRIPE_CHECK(parts.size() == 2, "'" << tok << "': saturation needs a factor, e.g. saturation:1.5");
      const double S = parse_num(trim(parts[1]), tok);
      // off-diagonals (1 - S) L_k; the diagonal takes what is left of 4096, so
      // every row sums to exactly 1.0 and grey pixels are fixed points
      const double L[3] = {.299, .587, .114};
      op.kind = OpKind::ColorMatrix;
      for (int c = 0; c < 3; ++c) {
        int off = 0;
        for (int k = 0; k < 3; ++k) {
          if (k == c) continue;
          const double q = std::nearbyint((1.0 - S) * L[k] * 4096.0);
          STRIPE_CHECK(std::fabs(q) <= 32767, "'" << tok << "': saturation factor out of range");
          op.cm[3 * c + k] = (int)q;
          off += (int)q;
        }
        op.cm[3 * c + c] = 4096 - off;
        STRIPE_CHECK(std::abs(op.cm[3 * c + c]) <= 32767, "'" << tok << "': saturation factor out of range");
      }
      op.fval = (float)S;
      std::ostringstream os;
      os << "saturation:" << op.fval;
      op.text = os.str();
    } else if (name == "ycbcr") {
      // JFIF full-range RGB <-> YCbCr; the inverse folds the -128 terms into the offsets
      const bool inv = parts.size() == 2 && trim(parts[1]) == "inv";
      STRIPE_CHECK(parts.size() == 1 || inv, "'" << tok << "': ycbcr syntax: ycbcr or ycbcr:inv");
      if (!inv) {
        const double m[9] = {.299, .587, .114, -.168736, -.331264, .5, .5, -.418688, -.081312};
        const double b[3] = {0, 128, 128};
        set_color_matrix(op, m, b, tok);
      } else {
        const double m[9] = {1, 0, 1.402, 1, -.344136, -.714136, 1, 1.772, 0};
        const double b[3] = {-1.402 * 128, .344136 * 128 + .714136 * 128, -1.772 * 128};
        set_color_matrix(op, m, b, tok);
      }
      op.text = inv ? "ycbcr:inv" : "ycbcr";
    } else if (name.compare(0, 9, "bilateral") == 0) {
      // bilateral3[:S] / bilateral5[:S] / bilateral[:S]  (filters.h); S is the range sigma
      const std::string sz = name.substr(9);
      STRIPE_CHECK(sz.empty() || sz == "3" || sz == "5",
                   "'" << name << "': bilateral takes a window size of 3 or 5 (bilateral3, bilateral5)");
      STRIPE_CHECK(parts.size() <= 2, "'" << tok << "': bilateral syntax: bilateral3[:S], bilateral5[:S]");
      const double S = parts.size() > 1 ? parse_num(trim(parts[1]), tok) : 25.0;
      STRIPE_CHECK(S > 0.0 && S <= 10000.0, "'" << tok << "': the range sigma must be in (0, 10000]");
      op.kind = OpKind::Stencil;
      op.sid = sz == "3" ? StencilId::Bilateral3 : StencilId::Bilateral5;
      op.sigma = S;
      op.range = bilateral_range_table(S);
      op.text = std::string(stencil_info(op.sid).name) + ":" + shortest_text(S);
    } else if (stencil_from_name(name, &sid)) {
      op.kind = OpKind::Stencil;
      op.sid = sid;
      op.text = stencil_info(sid).name;
    } else {
      fail("unknown filter '" + name +
           "' (gray[:ref|bt601], contrast:F[:cv], invert, brightness:D, threshold:T, expand, "
           "emboss3, emboss5, gaussian3/5/7, box3/5, sharpen, laplace, sobel, sobel_l2, median3/5, "
           "erode3/5, dilate3/5, open3/5, close3/5, bilateral3/5[:S], blur:K[:sigma][:lsb], conv:K:w..[:lsb], sepconv:K:h..:v..[:lsb], "
           "colormatrix:m00;..;m22[:b0;b1;b2], sepia, saturation:S, swaprb, ycbcr[:inv], "
           "equalize, autocontrast[:P], threshold:otsu, "
           "hold, swap, add, sub, rsub, absdiff, min, max, lincomb:a:b[:c], blend:t, above[:d], "
           "gradient3/5, tophat3/5, blackhat3/5, unsharp[:S[:K]], threshold:adaptive:K[:C])");
    }
    STRIPE_CHECK(op.kind != OpKind::Stat || !op.has_border,
                 "'" << raw << "': " << op.text << " is a pointwise op and takes no @border");
    STRIPE_CHECK(!(op.slot() || op.kind == OpKind::Combine) || !op.has_border,
                 "'" << raw << "': " << op.text << " reads no border and takes no @border");
    if (op.has_border) op.text += std::string("@") + border_name(op.border);
    ops.push_back(op);
  }
  return ops;
}

std::string chain_to_string(const std::vector<Op>& ops) {
  std::string s;
  for (size_t i = 0; i < ops.size(); ++i) {
    if (i) s += ",";
    s += ops[i].text;
  }
  return s;
}

// ---------------------------------------------------------------------------
// Pointwise numerics
// ---------------------------------------------------------------------------

static inline uint8_t sat_i(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

#pragma clang fp contract(off)
uint8_t apply_pointwise_u8(const Op& op, uint8_t p) {
  switch (op.kind) {
    case OpKind::Invert:
      return (uint8_t)(255 - p);
    case OpKind::Brightness:
      return sat_i((int)p + op.ival);
    case OpKind::Threshold:
      return p >= op.ival ? 255 : 0;
    case OpKind::Contrast: {
      if (op.round == RoundMode::Trunc) {
        // kernel.cu:50,56: clamp(contrast * (p - 128) + 128) then (uchar) truncation.
        // Spec: f32 multiply then f32 add (no fma).
        volatile float prod = op.fval * (float)((int)p - 128);
        float v = prod + 128.0f;
        if (v < 0.f) v = 0.f;
        if (v > 255.f) v = 255.f;
        return (uint8_t)v;
      }
      // kern.cpp:74: OpenCV folds 3*(x-128)+128 into convertTo(alpha=f, beta=128-128f)
      // evaluated in f32 and saturate_cast (round half to even).
      const float alpha = op.fval;
      const float beta = (float)(128.0 - 128.0 * (double)op.fval);
      volatile float prod = (float)p * alpha;
      float v = prod + beta;
      float r = std::nearbyint(v);
      if (r < 0.f) r = 0.f;
      if (r > 255.f) r = 255.f;
      return (uint8_t)r;
    }
    default:
      fail("apply_pointwise_u8: not a per-channel LUT op: " + op.text);
  }
}

uint8_t gray_pixel(GrayMode m, uint8_t r, uint8_t g, uint8_t b) {
  if (m == GrayMode::Ref) {
    // kernel.cu:40-42 (BGR order there; weights are bound to semantic channels, Q5).
    // (float)x * 0.11 promotes to double; each term truncated to u8 separately.
    return (uint8_t)((uint8_t)((double)(float)b * 0.11) + (uint8_t)((double)(float)g * 0.59) +
                     (uint8_t)((double)(float)r * 0.3));
  }
  // OpenCV COLOR_BGR2GRAY, 8U: fixed point, yuv_shift 14, rounded (kern.cpp:73).
  return (uint8_t)((r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14);
}

// ---------------------------------------------------------------------------
// Statistic ops (rules: filters.h)
// ---------------------------------------------------------------------------
namespace {
// channels pooled: h[v] = sum_c hist[c][v]
std::array<uint64_t, 256> pooled(const Histogram& hist) {
  STRIPE_CHECK((hist.C == 1 || hist.C == 3) && hist.bins.size() == (size_t)256 * hist.C,
               "histogram must hold 256 bins for 1 or 3 channels");
  std::array<uint64_t, 256> h{};
  for (int c = 0; c < hist.C; ++c)
    for (int v = 0; v < 256; ++v) h[(size_t)v] += hist.at(c, v);
  return h;
}
}  // namespace

int otsu_level(const Histogram& hist) {
  const std::array<uint64_t, 256> h = pooled(hist);
  uint64_t N = 0, S = 0;
  for (int v = 0; v < 256; ++v) {
    N += h[(size_t)v];
    S += (uint64_t)v * h[(size_t)v];
  }
  int best_t = 1;
  double best = 0.0;
  uint64_t n0 = 0, S0 = 0;
  for (int t = 1; t < 256; ++t) {
    n0 += h[(size_t)t - 1];
    S0 += (uint64_t)(t - 1) * h[(size_t)t - 1];
    const uint64_t n1 = N - n0;
    double g = 0.0;
    if (n0 != 0 && n1 != 0) {
      // IEEE double, no contraction (the pragma above): every layer calls this one
      const double p = (double)S0 * (double)N;
      const double q = (double)n0 * (double)S;
      const double a = p - q;
      const double num = a * a;
      const double den = (double)n0 * (double)n1;
      g = num / den;
    }
    if (g > best) {  // strict: the smallest t attains the maximum
      best = g;
      best_t = t;
    }
  }
  return best_t;
}

std::array<uint8_t, 256> stat_lut(const Op& op, const Histogram& hist) {
  STRIPE_CHECK(op.kind == OpKind::Stat, "stat_lut: '" << op.text << "' is not a statistic op");
  const std::array<uint64_t, 256> h = pooled(hist);
  std::array<uint8_t, 256> lut{};
  for (int v = 0; v < 256; ++v) lut[(size_t)v] = (uint8_t)v;
  uint64_t cdf[256], N = 0;
  for (int v = 0; v < 256; ++v) {
    N += h[(size_t)v];
    cdf[v] = N;
  }
  if (op.stat == StatKind::Otsu) {
    const int T = otsu_level(hist);
    for (int v = 0; v < 256; ++v) lut[(size_t)v] = v >= T ? 255 : 0;
    return lut;
  }
  if (N == 0) return lut;  // no pixels: identity
  if (op.stat == StatKind::Equalize) {
    int v0 = 0;
    while (h[(size_t)v0] == 0) ++v0;
    const uint64_t c0 = h[(size_t)v0], D = N - c0;
    if (D == 0) return lut;  // one grey level
    for (int v = 0; v < 256; ++v) {
      if (v < v0) {
        lut[(size_t)v] = 0;
        continue;
      }
      const uint64_t q = (510 * (cdf[v] - c0) + D) / (2 * D);
      lut[(size_t)v] = (uint8_t)(q > 255 ? 255 : q);
    }
    return lut;
  }
  // autocontrast
  const uint64_t cut = N * (uint64_t)op.ival / 10000;
  int lo = 0;
  while (lo < 255 && !(cdf[lo] > cut)) ++lo;
  int hi = 255;
  while (hi > 0 && !(N - cdf[hi - 1] > cut)) --hi;  // v = 0 always qualifies: cdf[-1] = 0, cut < N
  if (hi <= lo) return lut;
  const uint64_t d = (uint64_t)(hi - lo);
  for (int v = 0; v < 256; ++v) {
    if (v <= lo) lut[(size_t)v] = 0;
    else if (v >= hi) lut[(size_t)v] = 255;
    else lut[(size_t)v] = (uint8_t)((510 * (uint64_t)(v - lo) + d) / (2 * d));
  }
  return lut;
}
#pragma clang fp contract(on)

bool find_trunc_magic(double w, uint32_t* mult, int* shift) {
  for (int s = 8; s <= 24; ++s) {
    for (int bump = 0; bump <= 1; ++bump) {
      const uint32_t m = (uint32_t)std::floor(w * (double)(1u << s)) + (uint32_t)bump;
      bool ok = true;
      for (int x = 0; x < 256 && ok; ++x) {
        const uint32_t want = (uint32_t)(uint8_t)((double)(float)x * w);
        ok = ((uint32_t)x * m >> s) == want;
      }
      if (ok) {
        *mult = m;
        *shift = s;
        return true;
      }
    }
  }
  return false;
}

}  // namespace stripe
