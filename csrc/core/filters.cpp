// Filter catalogue and pointwise numerics.
#include "stripe/filters.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

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

// The catalogue row of definition F (stencil_defs.h): weighted stencils carry
// w (and w1 when w = w1 (x) w1), rank filters a rank, bilateral filters both
// the spatial weights and their taps.
template <class F>
StencilInfo make_info(StencilId id, std::initializer_list<const char*> names) {
  static_assert(F::RANK == 0 || (!F::SEP && !F::SOBEL && F::DIV == 1 && F::BILATERAL == 0), "rank filter definition");
  static_assert(F::BILATERAL == 0 || (!F::SEP && !F::SOBEL && F::DIV == 1 && F::RANK == 0),
                "bilateral filter definition");
  StencilInfo s;
  s.id = id;
  s.names = names;
  s.name = s.names.front();
  s.K = F::K;
  s.separable = F::SEP;
  s.sobel = F::SOBEL;
  if constexpr (F::SOBEL) s.l2 = F::L2;
  s.div = F::DIV;
  s.rank = (Rank)F::RANK;
  s.bilateral = F::BILATERAL != 0;
  if constexpr (F::RANK == 0)
    for (int dy = 0; dy < F::K; ++dy)
      for (int dx = 0; dx < F::K; ++dx) s.w.push_back(F::w(dy, dx));
  if constexpr ((F::SEP && !F::SOBEL) || F::BILATERAL != 0)
    for (int i = 0; i < F::K; ++i) s.w1.push_back(F::g(i));
  return s;
}

const std::vector<StencilInfo>& table() {
#define STRIPE_INFO_ROW(Id, ...) make_info<sdef::Id>(StencilId::Id, {__VA_ARGS__}),
  static const std::vector<StencilInfo> t = {STRIPE_STENCILS(STRIPE_INFO_ROW)};
#undef STRIPE_INFO_ROW
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
  for (const StencilInfo& s : table())
    for (const char* n : s.names)
      if (name == n) {
        *out = s.id;
        return true;
      }
  return false;
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

// ---------------------------------------------------------------------------
// The token table: every spelling a chain token may start with, its row of the
// catalogue (filter_catalogue) and the function that parses it.
// ---------------------------------------------------------------------------
namespace {

struct Entry;
struct Token {
  const std::string& text;         // the token without its "@border"; error messages quote it
  std::vector<std::string> parts;  // text split at ':'; parts[0] is the head name
  std::string border;              // "@border", canonical, or empty: sugar hands it to its stencils
  const Entry* entry;              // the table row that matched the head name (nullptr: a plain stencil name)
  std::string expansion;           // set by sugar and presets: the chain the token stands for
  const std::string& name() const { return parts[0]; }
};

// Fills `op` (kind, parameters, canonical text without "@border"), or sets t.expansion.
using ParseFn = void (*)(Token& t, Op& op);

struct Entry {
  std::vector<const char*> names;  // head names; none: a catalogue row without a parser of its own
  bool sized;                      // a family named by its window size: matches names that start with names[0]
  const char* syntax;              // catalogue row (nullptr: not listed)
  const char* about;
  ParseFn parse;
  const char* chain = nullptr;     // sugar and presets: what the token stands for ('#': window size and @border)
};
const std::vector<Entry>& entries();

[[noreturn]] void unknown_filter(const std::string& name) {
  std::string s = "unknown filter '" + name + "' (";
  const char* sep = "";
  for (const Entry& e : entries())
    if (e.syntax) {
      s += sep + std::string(e.syntax);
      sep = ", ";
    }
  fail(s + ")");
}

void no_arguments(const Token& t, const std::string& who) {
  STRIPE_CHECK(t.parts.size() == 1, "'" << t.text << "': " << who << " takes no arguments");
}

// The window size of a sized family's token: "3", "5" or, where the bare name
// is a spelling too, "".  Only the bilateral filters take arguments.
std::string window_size(const Token& t, bool bare, bool arguments = false) {
  const std::string f = t.entry->names[0], sz = t.name().substr(f.size());
  STRIPE_CHECK(sz == "3" || sz == "5" || (sz.empty() && bare),
               "'" << t.name() << "': " << f << " takes a window size of 3 or 5 (" << f << "3, " << f << "5)");
  if (!arguments) no_arguments(t, f);
  return sz;
}

void set_op(Op& op, OpKind kind, const char* text) {
  op.kind = kind;
  op.text = text;
}


// Trailing ":exact" / ":lsb" of a float conv token (removed from parts):
// 3 = exact (the default), 2 = every output within 1 LSB of the f64 result.
int take_precision(std::vector<std::string>& parts) {
  if (parts.size() < 2) return 3;
  const std::string last = trim(parts.back());
  if (last != "exact" && last != "lsb") return 3;
  parts.pop_back();
  return last == "lsb" ? 2 : 3;
}

// ---- stencils ----
void p_stencil(Token& t, Op& op) {  // every name of STRIPE_STENCILS; arguments of a plain stencil are ignored
  if (!stencil_from_name(t.name(), &op.sid)) unknown_filter(t.name());
  set_op(op, OpKind::Stencil, stencil_info(op.sid).name);
}

void p_rank(Token& t, Op& op) {  // median / erode / dilate [3|5]
  window_size(t, true);
  p_stencil(t, op);
}

void p_bilateral(Token& t, Op& op) {  // bilateral[3|5][:S]  (filters.h); S is the range sigma
  window_size(t, true, true);
  STRIPE_CHECK(t.parts.size() <= 2, "'" << t.text << "': bilateral syntax: bilateral3[:S], bilateral5[:S]");
  const double S = t.parts.size() > 1 ? parse_num(trim(t.parts[1]), t.text) : 25.0;
  STRIPE_CHECK(S > 0.0 && S <= 10000.0, "'" << t.text << "': the range sigma must be in (0, 10000]");
  p_stencil(t, op);
  op.sigma = S;
  op.range = bilateral_range_table(S);
  op.text += ":" + shortest_text(S);
}

// ---- sugar: the chain a token stands for; its @border goes to the stencils inside ----
void p_sized_sugar(Token& t, Op&) {  // open close gradient tophat blackhat [3|5]
  const std::string k = window_size(t, false) + t.border;
  for (const char* c = t.entry->chain; *c; ++c) t.expansion += *c == '#' ? k : std::string(1, *c);
}

void p_unsharp(Token& t, Op&) {
  // unsharp[:S[:K]]  x + S (x - gaussianK(x)) in Q12: qa = -nearbyint(4096 S) on the blur, 4096 - qa on x
  STRIPE_CHECK(t.parts.size() <= 3, "'" << t.text << "': unsharp syntax: unsharp[:S[:K]]");
  const double S = t.parts.size() > 1 ? parse_num(trim(t.parts[1]), t.text) : 1.0;
  const std::string k = t.parts.size() > 2 ? trim(t.parts[2]) : "5";
  STRIPE_CHECK(S > 0.0 && S < 7.0, "'" << t.text << "': unsharp amount must be in (0, 7)");
  STRIPE_CHECK(k == "3" || k == "5" || k == "7", "'" << t.text << "': unsharp blurs with gaussian3, 5 or 7");
  const int qa = -(int)std::nearbyint(4096.0 * S);
  STRIPE_CHECK(qa != 0 && 4096 - qa <= 32767, "'" << t.text << "': unsharp amount must be in (0, 7)");
  t.expansion = "hold,gaussian" + k + t.border + ",lincomb:" + q12_text(qa) + ":" + q12_text(4096 - qa);
}

// Presets (SURVEY Appendix A "presets"): the bare name only; halo / partition
// flags of a preset are applied by the callers (CLI / models.PRESETS).
void p_preset(Token& t, Op&) {
  if (t.parts.size() != 1 || !t.border.empty()) unknown_filter(t.name());
  t.expansion = t.entry->chain;
}

// ---- two-image ops ----
void p_hold(Token& t, Op& op) { no_arguments(t, t.name()), set_op(op, OpKind::Hold, "hold"); }
void p_swap(Token& t, Op& op) { no_arguments(t, t.name()), set_op(op, OpKind::Swap, "swap"); }

void p_combine(Token& t, Op& op) {  // add sub rsub absdiff min max: the names of combine_name
  no_arguments(t, t.name());
  op.kind = OpKind::Combine;
  for (int k = 0; k < (int)CombineKind::kCount; ++k)
    if (t.name() == combine_name((CombineKind)k)) op.comb = (CombineKind)k;
  op.text = t.name();
}

void set_lincomb_text(Op& op) {  // lincomb and blend are both spelled canonically as lincomb
  op.kind = OpKind::Combine;
  op.comb = CombineKind::LinComb;
  op.text = "lincomb:" + q12_text(op.cq[0]) + ":" + q12_text(op.cq[1]) +
            (op.cq[2] != 0 ? ":" + q12_text(op.cq[2]) : std::string());
}

void p_lincomb(Token& t, Op& op) {  // lincomb:a:b[:c]  (Q12, filters.h)
  STRIPE_CHECK(t.parts.size() == 3 || t.parts.size() == 4, "'" << t.text << "': lincomb syntax: lincomb:a:b[:c]");
  for (int i = 0; i < 2; ++i) {
    const double a = parse_num(trim(t.parts[(size_t)i + 1]), t.text);
    const double q = std::nearbyint(a * 4096.0);
    STRIPE_CHECK(std::fabs(q) <= 32767, "'" << t.text << "': coefficient " << a << " out of range (|a| < 8)");
    op.cq[i] = (int)q;
  }
  if (t.parts.size() == 4) {
    const double c = parse_num(trim(t.parts[3]), t.text);
    STRIPE_CHECK(std::fabs(c) <= 2048, "'" << t.text << "': offset " << c << " out of range (|c| <= 2048)");
    op.cq[2] = (int)std::nearbyint(c * 4096.0);
  }
  set_lincomb_text(op);
}

void p_blend(Token& t, Op& op) {  // blend:t
  STRIPE_CHECK(t.parts.size() == 2, "'" << t.text << "': blend needs a weight, e.g. blend:0.25");
  const double w = parse_num(trim(t.parts[1]), t.text);
  STRIPE_CHECK(w >= 0.0 && w <= 1.0, "'" << t.text << "': blend weight must be in [0, 1]");
  op.cq[0] = (int)std::nearbyint(4096.0 * w);
  op.cq[1] = 4096 - op.cq[0];
  set_lincomb_text(op);
}

void p_above(Token& t, Op& op) {
  STRIPE_CHECK(t.parts.size() <= 2, "'" << t.text << "': above syntax: above[:d]");
  const double d = t.parts.size() > 1 ? parse_num(trim(t.parts[1]), t.text) : 0.0;
  STRIPE_CHECK(d == std::nearbyint(d) && std::fabs(d) <= 255,
               "'" << t.text << "': above takes an integer offset in [-255, 255]");
  op.kind = OpKind::Combine;
  op.comb = CombineKind::Above;
  op.ival = (int)d;
  op.text = op.ival != 0 ? "above:" + std::to_string(op.ival) : std::string("above");
}

// ---- pointwise ----
void p_gray(Token& t, Op& op) {
  op.kind = OpKind::Gray;
  op.gray = GrayMode::BT601;
  if (t.parts.size() > 1) {
    if (t.parts[1] == "ref") op.gray = GrayMode::Ref;
    else if (t.parts[1] == "bt601" || t.parts[1] == "cv") op.gray = GrayMode::BT601;
    else fail("gray mode must be ref|bt601, got '" + t.parts[1] + "'");
  }
  op.text = op.gray == GrayMode::Ref ? "gray:ref" : "gray:bt601";
}

void p_contrast(Token& t, Op& op) {
  op.kind = OpKind::Contrast;
  op.fval = t.parts.size() > 1 ? (float)parse_num(t.parts[1], t.text) : 3.5f;
  op.round = RoundMode::Trunc;
  if (t.parts.size() > 2) {
    if (t.parts[2] == "cv" || t.parts[2] == "round") op.round = RoundMode::Nearest;
    else if (t.parts[2] == "ref" || t.parts[2] == "trunc") op.round = RoundMode::Trunc;
    else fail("contrast rounding must be ref|cv, got '" + t.parts[2] + "'");
  }
  std::ostringstream os;
  os << "contrast:" << op.fval << (op.round == RoundMode::Nearest ? ":cv" : "");
  op.text = os.str();
}

void p_invert(Token&, Op& op) { set_op(op, OpKind::Invert, "invert"); }
void p_expand(Token&, Op& op) { set_op(op, OpKind::Expand, "expand"); }

void p_brightness(Token& t, Op& op) {
  op.kind = OpKind::Brightness;
  STRIPE_CHECK(t.parts.size() > 1, "brightness needs a delta, e.g. brightness:40");
  op.ival = (int)parse_num(t.parts[1], t.text);
  op.text = "brightness:" + std::to_string(op.ival);
}

// threshold[:T] | threshold:otsu | threshold:adaptive:K[:C]
void p_threshold(Token& t, Op& op) {
  const std::string mode = t.parts.size() > 1 ? trim(t.parts[1]) : std::string();
  if (mode == "adaptive") {  // x > boxK(x) - C
    STRIPE_CHECK(t.parts.size() == 3 || t.parts.size() == 4,
                 "'" << t.text << "': adaptive threshold syntax: threshold:adaptive:K[:C]");
    const std::string k = trim(t.parts[2]);
    STRIPE_CHECK(k == "3" || k == "5", "'" << t.text << "': threshold:adaptive takes a window size of 3 or 5");
    const double Cd = t.parts.size() > 3 ? parse_num(trim(t.parts[3]), t.text) : 0.0;
    STRIPE_CHECK(Cd == std::nearbyint(Cd) && std::fabs(Cd) <= 255,
                 "'" << t.text << "': threshold:adaptive offset must be an integer in [-255, 255]");
    t.expansion = "hold,box" + k + t.border + ",above:" + std::to_string((int)Cd);
  } else if (mode == "otsu") {  // Otsu's level of the global histogram, chosen at run time (filters.h)
    STRIPE_CHECK(t.parts.size() == 2, "'" << t.text << "': threshold:otsu takes no further arguments");
    set_op(op, OpKind::Stat, "threshold:otsu");
    op.stat = StatKind::Otsu;
  } else {
    op.kind = OpKind::Threshold;
    op.ival = t.parts.size() > 1 ? (int)parse_num(t.parts[1], t.text) : 128;
    op.text = "threshold:" + std::to_string(op.ival);
  }
}

void p_equalize(Token& t, Op& op) {
  no_arguments(t, "equalize");
  set_op(op, OpKind::Stat, "equalize");
  op.stat = StatKind::Equalize;
}

void p_autocontrast(Token& t, Op& op) {
  // autocontrast[:P]  P percent of the pixels clipped at each end, in hundredths
  STRIPE_CHECK(t.parts.size() <= 2, "'" << t.text << "': autocontrast syntax: autocontrast[:P]");
  const double P = t.parts.size() > 1 ? parse_num(trim(t.parts[1]), t.text) : 0.0;
  STRIPE_CHECK(P >= 0.0 && P < 50.0, "'" << t.text << "': autocontrast clips 0 <= P < 50 percent per end");
  op.kind = OpKind::Stat;
  op.stat = StatKind::AutoContrast;
  op.ival = (int)std::nearbyint(100.0 * P);
  STRIPE_CHECK(op.ival < 5000, "'" << t.text << "': autocontrast clips 0 <= P < 50 percent per end");
  std::ostringstream os;
  os << "autocontrast";
  if (op.ival != 0) os << ":" << op.ival / 100.0;
  op.text = os.str();
}

// ---- float convolutions ----
void p_blur(Token& t, Op& op) {  // blur[:K[:sigma]][:exact|:lsb]
  op.conv_digits = take_precision(t.parts);
  STRIPE_CHECK(t.parts.size() <= 3, "blur syntax: blur:K[:sigma][:exact|:lsb]");
  const int K = t.parts.size() > 1 ? (int)parse_num(t.parts[1], t.text) : 31;
  const double sigma = t.parts.size() > 2 ? parse_num(t.parts[2], t.text) : 0.0;
  STRIPE_CHECK(K >= 3 && K % 2 == 1 && K / 2 <= kMaxRadius,
               "blur:K needs odd K in [3, " << 2 * kMaxRadius + 1 << "], got " << K);
  op.kind = OpKind::Conv;
  op.K = K;
  const auto g = gaussian_1d(K, sigma);
  op.weights.resize((size_t)K * K);
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) op.weights[(size_t)i * K + j] = (float)(g[i] * g[j]);
  op.sep_h.assign(g.begin(), g.end());
  op.sep_v = op.sep_h;
  op.text = t.text;
}

void p_conv(Token& t, Op& op) {
  // conv:K:w00;w01;...[:exact|:lsb]  (K*K weights, row-major, correlation)
  STRIPE_CHECK(t.parts.size() == 3 || t.parts.size() == 4, "conv syntax: conv:K:w0;w1;...;w(K*K-1)[:exact|:lsb]");
  if (t.parts.size() == 4) {
    const std::string prec = trim(t.parts[3]);
    STRIPE_CHECK(prec == "exact" || prec == "lsb", "conv precision must be exact or lsb, got '" << prec << "'");
    op.conv_digits = prec == "lsb" ? 2 : 3;
  }
  op.kind = OpKind::Conv;
  op.K = (int)parse_num(t.parts[1], t.text);
  STRIPE_CHECK(op.K >= 1 && op.K % 2 == 1 && op.K / 2 <= kMaxRadius, "conv K must be odd <= 33");
  for (const auto& w : split(t.parts[2], ';')) op.weights.push_back((float)parse_num(trim(w), t.text));
  STRIPE_CHECK((int)op.weights.size() == op.K * op.K,
               "conv:" << op.K << " needs " << op.K * op.K << " weights, got " << op.weights.size());
  op.text = t.text;
}

void p_sepconv(Token& t, Op& op) {
  // sepconv:K:h0;...;h(K-1):v0;...;v(K-1)[:exact|:lsb]  rank-one KxK correlation
  // weights[dy][dx] = v[dy] * h[dx] (separable MFMA path on the GPU)
  op.conv_digits = take_precision(t.parts);
  STRIPE_CHECK(t.parts.size() == 4, "sepconv syntax: sepconv:K:h0;...;h(K-1):v0;...;v(K-1)[:exact|:lsb]");
  op.kind = OpKind::Conv;
  op.K = (int)parse_num(t.parts[1], t.text);
  STRIPE_CHECK(op.K >= 1 && op.K % 2 == 1 && op.K / 2 <= kMaxRadius, "sepconv K must be odd <= 33");
  for (const auto& w : split(t.parts[2], ';')) op.sep_h.push_back((float)parse_num(trim(w), t.text));
  for (const auto& w : split(t.parts[3], ';')) op.sep_v.push_back((float)parse_num(trim(w), t.text));
  STRIPE_CHECK((int)op.sep_h.size() == op.K && (int)op.sep_v.size() == op.K,
               "sepconv:" << op.K << " needs " << op.K << " horizontal and " << op.K << " vertical weights");
  op.weights.resize((size_t)op.K * op.K);
  for (int i = 0; i < op.K; ++i)
    for (int j = 0; j < op.K; ++j) op.weights[(size_t)i * op.K + j] = op.sep_v[(size_t)i] * op.sep_h[(size_t)j];
  op.text = t.text;
}

// ---- colour matrices ----
void p_colormatrix(Token& t, Op& op) {
  // colormatrix:m00;m01;m02;m10;...;m22[:b0;b1;b2]  row-major, out_c = sum_k m[c][k] in_k + b_c
  STRIPE_CHECK(t.parts.size() == 2 || t.parts.size() == 3,
               "'" << t.text << "': colormatrix syntax: colormatrix:m00;m01;...;m22[:b0;b1;b2]");
  double m[9], b[3] = {0, 0, 0};
  const auto ms = split(t.parts[1], ';');
  STRIPE_CHECK(ms.size() == 9, "'" << t.text << "': colormatrix needs 9 coefficients, got " << ms.size());
  for (int i = 0; i < 9; ++i) m[i] = parse_num(trim(ms[(size_t)i]), t.text);
  if (t.parts.size() == 3) {
    const auto bs = split(t.parts[2], ';');
    STRIPE_CHECK(bs.size() == 3, "'" << t.text << "': colormatrix takes 3 offsets, got " << bs.size());
    for (int i = 0; i < 3; ++i) b[i] = parse_num(trim(bs[(size_t)i]), t.text);
  }
  set_color_matrix(op, m, b, t.text);
  op.text = t.text;
}

void p_sepia(Token& t, Op& op) {
  no_arguments(t, "sepia");
  const double m[9] = {.393, .769, .189, .349, .686, .168, .272, .534, .131}, b[3] = {0, 0, 0};
  set_color_matrix(op, m, b, t.text);
  op.text = "sepia";
}

void p_swaprb(Token& t, Op& op) {
  no_arguments(t, t.name());
  const double m[9] = {0, 0, 1, 0, 1, 0, 1, 0, 0}, b[3] = {0, 0, 0};
  set_color_matrix(op, m, b, t.text);
  op.text = "swaprb";
}

void p_saturation(Token& t, Op& op) {
  STRIPE_CHECK(t.parts.size() == 2, "'" << t.text << "': saturation needs a factor, e.g. saturation:1.5");
  const double S = parse_num(trim(t.parts[1]), t.text);
  // off-diagonals (1 - S) L_k; the diagonal takes what is left of 4096, so
  // every row sums to exactly 1.0 and grey pixels are fixed points
  const double L[3] = {.299, .587, .114};
  op.kind = OpKind::ColorMatrix;
  for (int c = 0; c < 3; ++c) {
    int off = 0;
    for (int k = 0; k < 3; ++k) {
      if (k == c) continue;
      const double q = std::nearbyint((1.0 - S) * L[k] * 4096.0);
      STRIPE_CHECK(std::fabs(q) <= 32767, "'" << t.text << "': saturation factor out of range");
      op.cm[3 * c + k] = (int)q;
      off += (int)q;
    }
    op.cm[3 * c + c] = 4096 - off;
    STRIPE_CHECK(std::abs(op.cm[3 * c + c]) <= 32767, "'" << t.text << "': saturation factor out of range");
  }
  op.fval = (float)S;
  std::ostringstream os;
  os << "saturation:" << op.fval;
  op.text = os.str();
}

void p_ycbcr(Token& t, Op& op) {
  // JFIF full-range RGB <-> YCbCr; the inverse folds the -128 terms into the offsets
  const bool inv = t.parts.size() == 2 && trim(t.parts[1]) == "inv";
  STRIPE_CHECK(t.parts.size() == 1 || inv, "'" << t.text << "': ycbcr syntax: ycbcr or ycbcr:inv");
  if (!inv) {
    const double m[9] = {.299, .587, .114, -.168736, -.331264, .5, .5, -.418688, -.081312};
    const double b[3] = {0, 128, 128};
    set_color_matrix(op, m, b, t.text);
  } else {
    const double m[9] = {1, 0, 1.402, 1, -.344136, -.714136, 1, 1.772, 0};
    const double b[3] = {-1.402 * 128, .344136 * 128 + .714136 * 128, -1.772 * 128};
    set_color_matrix(op, m, b, t.text);
  }
  op.text = inv ? "ycbcr:inv" : "ycbcr";
}

// In catalogue order.  A row without names documents spellings that another
// entry parses (threshold) or that need none: the plain stencil names reach
// p_stencil through STRIPE_STENCILS.
const std::vector<Entry>& entries() {
  static const std::vector<Entry> t = {
      // pointwise
      {{"gray", "grayscale", "grey"}, false, "gray[:ref|bt601]",
       "grayscale (ref: kernel.cu:31-44 weights/truncation; bt601: OpenCV, kern.cpp:73)", p_gray},
      {{"contrast"}, false, "contrast:F[:cv]",
       "trunc(clamp(F*(p-128)+128)) (kernel.cu:49-58); ':cv' = OpenCV rounding (kern.cpp:74)", p_contrast},
      {{"invert", "negate"}, false, "invert", "255 - p", p_invert},
      {{"brightness", "bright"}, false, "brightness:D", "sat(p + D)", p_brightness},
      {{"threshold"}, false, "threshold:T", "p >= T ? 255 : 0", p_threshold},
      {{"expand", "gray2rgb"}, false, "expand", "gray -> 3 identical channels (GRAY2BGR, kernel.cu:210)", p_expand},
      // colour matrices (3 -> 3 channels, Q12 fixed point: sat((q.p + qb + 2048) >> 12))
      {{"colormatrix"}, false, "colormatrix:m00;m01;..;m22[:b0;b1;b2]",
       "out_c = sum_k m[c][k] in_k + b_c on (R, G, B), row-major; |m| < 8, |b| <= 2048", p_colormatrix},
      {{"sepia"}, false, "sepia", "the sepia tone matrix [[.393,.769,.189],[.349,.686,.168],[.272,.534,.131]]",
       p_sepia},
      {{"saturation", "saturate"}, false, "saturation:S (saturate:S)",
       "mix with the BT.601 luma: 0 = gray, 1 = identity, > 1 = more colour; gray pixels stay", p_saturation},
      {{"swaprb", "bgr"}, false, "swaprb (bgr)", "swap the R and B channels (RGB <-> BGR)", p_swaprb},
      {{"ycbcr"}, false, "ycbcr / ycbcr:inv", "JFIF full-range RGB -> (Y, Cb, Cr) and back", p_ycbcr},
      // statistic ops (filters.h): each costs one read-only histogram pass (k_hist), one small all-reduce and
      // one host synchronisation
      {{"equalize"}, false, "equalize",
       "histogram equalisation (OpenCV equalizeHist, exact): v0 = first v with h[v] > 0, c0 = h[v0], "
       "D = N - c0; D == 0: identity; else 0 for v < v0 and min(255, (510 (cdf[v] - c0) + D) / (2 D))",
       p_equalize},
      {{"autocontrast"}, false, "autocontrast[:P]",
       "contrast stretch clipping P percent (0 <= P < 50, default 0) of the pixels per end: "
       "Pq = nearbyint(100 P), cut = N Pq / 10000; lo = first v with cdf[v] > cut, hi = last v "
       "with N - cdf[v-1] > cut; hi <= lo: identity; else 0 for v <= lo, 255 for v >= hi, "
       "(510 (v - lo) + (hi - lo)) / (2 (hi - lo)) between",
       p_autocontrast},
      {{}, false, "threshold:otsu",
       "p >= T ? 255 : 0 with Otsu's T: the smallest t in 1..255 maximising "
       "(S0 N - n0 S)^2 / (n0 n1) in double (n0, S0: count and sum below t; one grey level: T = 1)",
       nullptr},
      // stencils
      {{}, false, "emboss3 / emboss5", "kernel.cu:64-94 filters (3x3 and diagonal 5x5)", nullptr},
      {{}, false, "gaussian3/5/7", "binomial Gaussian, integer, rounded", nullptr},
      {{}, false, "box3 / box5", "box mean, rounded", nullptr},
      {{}, false, "sharpen", "[[0,-1,0],[-1,5,-1],[0,-1,0]]", nullptr},
      {{}, false, "laplace", "[[0,1,0],[1,-4,1],[0,1,0]]", nullptr},
      {{}, false, "sobel", "sat(|Gx| + |Gy|)", nullptr},
      {{}, false, "sobel_l2 / magnitude", "sat(round(sqrt(Gx^2 + Gy^2))), exact integer rounding", nullptr},
      {{"median"}, true, "median3 / median5 (median)", "element K*K/2 of the sorted KxK window, per channel", p_rank},
      {{"erode"}, true, "erode3 / erode5 (erode)",
       "minimum of the KxK window; border pixels are window members "
       "(@constant: the zeros outside the frame darken its edge)",
       p_rank},
      {{"dilate"}, true, "dilate3 / dilate5 (dilate)", "maximum of the KxK window", p_rank},
      {{"open"}, true, "open3 / open5", "erodeK,dilateK (an @border suffix applies to both)", p_sized_sugar,
       "erode#,dilate#"},
      {{"close"}, true, "close3 / close5", "dilateK,erodeK", p_sized_sugar, "dilate#,erode#"},
      {{"bilateral"}, true, "bilateral3[:S] / bilateral5[:S] (bilateral)",
       "edge-preserving smoothing, per channel: binomial taps times "
       "r[|p - centre|], r[d] = rint(255 exp(-d^2 / (2 S^2))), "
       "out = (sum w p + D/2) / D exactly; S = range sigma in grey "
       "levels, 0 < S <= 10000, default 25 (S >= 4096: gaussianK)",
       p_bilateral},
      {{"blur", "gblur"}, false, "blur:K[:sigma][:lsb]",
       "KxK float Gaussian (separable MFMA path), K <= 33; :lsb = every output within 1 LSB, "
       "2.5x fewer MFMAs",
       p_blur},
      {{"conv"}, false, "conv:K:w0;w1;...[:lsb]",
       "generic KxK float correlation (MFMA path); :lsb = within 1 LSB, 2/3 of the MFMAs", p_conv},
      {{"sepconv"}, false, "sepconv:K:h..:v..[:lsb]", "rank-one KxK float correlation v (x) h (separable MFMA path)",
       p_sepconv},
      {{}, false, "...@border", "per-stencil border: reflect101 | replicate | constant | skip", nullptr},
      // two-image ops: X the current image, H the held one (same channels), every rule per byte
      {{"hold", "save"}, false, "hold (save)",
       "the current image also becomes the held image (moves no pixels; a second hold replaces the first)", p_hold},
      {{"swap"}, false, "swap", "current and held exchange roles (moves no pixels)", p_swap},
      {{"add"}, false, "add", "min(255, X + H)", p_combine},
      {{"sub"}, false, "sub", "max(0, H - X)  (held minus current)", p_combine},
      {{"rsub"}, false, "rsub", "max(0, X - H)", p_combine},
      {{"absdiff"}, false, "absdiff", "|X - H|", p_combine},
      {{"min", "max"}, false, "min / max", "byte minimum / maximum of X and H", p_combine},
      {{"lincomb"}, false, "lincomb:a:b[:c]",
       "sat((qa X + qb H + qc + 2048) >> 12), q = nearbyint(4096 .): |a|, |b| < 8, |c| <= 2048", p_lincomb},
      {{"blend"}, false, "blend:t",
       "lincomb with qa = nearbyint(4096 t), qb = 4096 - qa, 0 <= t <= 1 (equal images are fixed points)", p_blend},
      {{"above"}, false, "above[:d]", "H - X + d > 0 ? 255 : 0, integer d in [-255, 255]", p_above},
      {{"gradient"}, true, "gradient3 / gradient5", "morphological gradient: hold,dilateK,swap,erodeK,sub",
       p_sized_sugar, "hold,dilate#,swap,erode#,sub"},
      {{"tophat"}, true, "tophat3 / tophat5", "x - open(x): hold,openK,sub", p_sized_sugar, "hold,open#,sub"},
      {{"blackhat"}, true, "blackhat3 / blackhat5", "close(x) - x: hold,closeK,rsub", p_sized_sugar,
       "hold,close#,rsub"},
      {{"unsharp"}, false, "unsharp[:S[:K]]",
       "x + S (x - gaussianK(x)): hold,gaussianK,lincomb:-S:1+S; S in (0, 7) default 1, K in 3|5|7 "
       "default 5; flat regions stay",
       p_unsharp},
      {{}, false, "threshold:adaptive:K[:C]",
       "x > boxK(x) - C ? 255 : 0 (OpenCV ADAPTIVE_THRESH_MEAN_C): hold,boxK,above:C; K in 3|5", nullptr},
      // presets: not catalogue rows
      {{"ref-gpu"}, false, nullptr, nullptr, p_preset, "gray:ref,contrast:3.5,emboss3@skip"},
      {{"ref-cpu"}, false, nullptr, nullptr, p_preset, "gray:bt601,contrast:3:cv,emboss3"},
  };
  return t;
}

const Entry* find_entry(const std::string& name) {
  for (const Entry& e : entries())
    for (const char* n : e.names)
      if (e.sized ? name.compare(0, std::strlen(n), n) == 0 : name == n) return &e;
  return nullptr;
}

}  // namespace

std::vector<std::pair<std::string, std::string>> filter_catalogue() {
  std::vector<std::pair<std::string, std::string>> rows;
  for (const Entry& e : entries())
    if (e.syntax) rows.emplace_back(e.syntax, e.about);
  return rows;
}

std::vector<Op> parse_chain(const std::string& spec_in) {
  const std::string spec = trim(spec_in);
  std::vector<Op> ops;
  STRIPE_CHECK(!spec.empty(), "empty filter chain");
  for (const std::string& raw : split(spec, ',')) {
    std::string tok = trim(raw);
    STRIPE_CHECK(!tok.empty(), "empty token in chain '" << spec << "'");
    Op op;
    // optional per-op border override: name[:args]@border
    const auto at = tok.find('@');
    if (at != std::string::npos) {
      op.has_border = true;
      op.border = parse_border(tok.substr(at + 1));
      tok = tok.substr(0, at);
    }
    Token t{tok, split(tok, ':'), op.has_border ? std::string("@") + border_name(op.border) : "", nullptr, ""};
    t.entry = find_entry(t.name());
    (t.entry ? t.entry->parse : p_stencil)(t, op);
    if (!t.expansion.empty()) {  // sugar and presets expand in place
      const auto sub = parse_chain(t.expansion);
      ops.insert(ops.end(), sub.begin(), sub.end());
      continue;
    }
    STRIPE_CHECK(op.kind != OpKind::Stat || !op.has_border,
                 "'" << raw << "': " << op.text << " is a pointwise op and takes no @border");
    STRIPE_CHECK(!(op.slot() || op.kind == OpKind::Combine) || !op.has_border,
                 "'" << raw << "': " << op.text << " reads no border and takes no @border");
    op.text += t.border;
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
