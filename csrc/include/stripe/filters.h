// Filter catalogue: the exact numeric specification of every operation
// (SURVEY Appendix A).  Shared by the CPU golden path, the chain compiler and,
// through stencil_defs.h, the HIP kernels.  The spellings a chain token may
// take, with a one-line description each, are the parser's token table
// (filters.cpp, filter_catalogue); the stencil names are STRIPE_STENCILS.
//
// Reference filters:
//   gray:ref      kernel.cu:31-44   Y = trunc(B*.11)+trunc(G*.59)+trunc(R*.3) (double)
//   gray:bt601    kern.cpp:73       OpenCV BGR2GRAY fixed point (>>14, rounded)
//   contrast:3.5  kernel.cu:49-58   trunc(clamp(3.5f*(p-128)+128))
//   contrast:3:cv kern.cpp:74       saturate_cast(3p-256) (OpenCV MatExpr folding)
//   emboss3/5     kernel.cu:64-94, kern.cpp:62-75
// North-star filters (BASELINE.json): invert, brightness, gaussian, sobel, sharpen,
// large-kernel blur.  Extras: gaussian3/7, box3/5, laplace, threshold, expand.
// Rank filters: median3/5, erode3/5, dilate3/5 over the square K x K window of
// the border-extended image (border pixels are window members like any other:
// with @constant the zeros outside the frame take part, so erode3@constant
// darkens the frame edge - unlike OpenCV's morphology default, which ignores
// them); open3/5 = erode,dilate and close3/5 = dilate,erode are parser sugar.
// Colour matrices (colormatrix:..., sepia, saturation:S, swaprb, ycbcr[:inv]):
// a 3x3 matrix and an offset on the (R, G, B) pixel in Q12 fixed point,
//   out_c = sat_u8((sum_k q[c][k] * p_k + qb[c] + 2048) >> 12)   (>>: floor)
// with q = nearbyint(m * 4096) and qb = nearbyint(b * 4096) (double, ties to
// even), |q| <= 32767 (|m| < 8) and |b| <= 2048: every sum fits 27 bits.
//
// Statistic ops (equalize, autocontrast[:P], threshold:otsu): a per-byte table
// computed from the GLOBAL histogram of the image as it enters the op (the
// whole frame over all ranks, after every earlier op).  On RGB the three
// channel histograms are pooled, h[v] = sum_c hist[c][v], and the one table is
// applied to all three channels (no hue shift).  With N = sum h and
// cdf[v] = sum_{u <= v} h[u], all in unsigned 64-bit integers (stat_lut):
//   equalize      v0 = smallest v with h[v] > 0, c0 = h[v0], D = N - c0.
//                 D == 0 (one grey level): identity.  Else lut[v] = 0 for
//                 v < v0 and min(255, (510 (cdf[v] - c0) + D) / (2 D)) after:
//                 OpenCV's equalizeHist rule, rounded exactly.
//   autocontrast  P percent of the pixels clipped at each end, 0 <= P < 50,
//                 Pq = nearbyint(100 P), cut = floor(N Pq / 10000).  lo =
//                 smallest v with cdf[v] > cut, hi = largest v with
//                 N - cdf[v-1] > cut (cdf[-1] = 0).  hi <= lo: identity.  Else
//                 0 for v <= lo, 255 for v >= hi and
//                 (510 (v - lo) + (hi - lo)) / (2 (hi - lo)) in between.
//   threshold:otsu  p >= T ? 255 : 0 with T = otsu_level: for t = 1..255,
//                 n0 = sum_{v<t} h, S0 = sum_{v<t} v h, n1 = N - n0,
//                 S = sum v h; g(t) = 0 when n0 == 0 or n1 == 0, else
//                 a a / ((double)n0 (double)n1), a = (double)S0 (double)N -
//                 (double)n0 (double)S, in IEEE double without contraction;
//                 T = the smallest t that attains the maximum (one grey
//                 level: T = 1).
//
// Two-image ops.  X is the current image, H the held image (same channel count);
// every rule is per byte.  Slot ops move no pixels:
//   hold (save)   the current image also becomes the held image (a second hold
//                 replaces the first)
//   swap          current and held exchange roles
// Combine ops (OpKind::Combine, combine_u8) read X and H and write a new current
// image; H stays held:
//   add           min(255, X + H)
//   sub           max(0, H - X)            (held minus current)
//   rsub          max(0, X - H)
//   absdiff       |X - H|
//   min, max      byte minimum / maximum
//   lincomb:a:b[:c]  sat_u8((qa X + qb H + qc + 2048) >> 12), >> = floor, with
//                 qa = nearbyint(4096 a), qb = nearbyint(4096 b), |q| <= 32767,
//                 qc = nearbyint(4096 c), |c| <= 2048: the colour matrix's Q12
//                 rule and ranges; the sum fits 26 bits
//   blend:t       lincomb with qa = nearbyint(4096 t), qb = 4096 - qa, 0 <= t <= 1
//                 (equal images are fixed points)
//   above[:d]     H - X + d > 0 ? 255 : 0, integer d in [-255, 255], default 0
// Parser sugar (an @border suffix goes to the stencils inside):
//   gradient3/5   hold,dilateK,swap,erodeK,sub
//   tophat3/5     hold,openK,sub
//   blackhat3/5   hold,closeK,rsub
//   unsharp[:S[:K]]  hold,gaussianK,lincomb with qa = -nearbyint(4096 S),
//                 qb = 4096 - qa; S defaults to 1 (0 < S < 7), K in {3,5,7}
//                 defaults to 5; flat regions are fixed points
//   threshold:adaptive:K[:C]  hold,boxK,above:C, K in {3,5}, C defaults to 0:
//                 OpenCV's ADAPTIVE_THRESH_MEAN_C on boxK's own rounding
//
// Bilateral filters (bilateral3[:S], bilateral5[:S], bilateral[:S] = bilateral5):
// an edge-preserving smoother, per channel, over the K x K window of the
// border-extended, prologue-applied image.  S is the range sigma in grey
// levels, 0 < S <= 10000, default 25.  With c the centre pixel and p(dy,dx) the
// window pixels:
//   ws(dy,dx) = g[dy] g[dx]             g: the binomial taps of gaussianK
//   r[d]      = rint(255 exp(-d^2 / (2 S^2)))   d = 0..255, computed once by
//               the parser in double (bilateral_range_table); no other layer
//               calls exp
//   w = ws r[|p - c|],  D = sum w,  N = sum w p
//   out = (N + (D >> 1)) / D            floor division (bilateral_finish)
// D >= ws(centre) 255 > 0 and D <= 256 * 255 = 65280 (u16); every w <= 36 * 255;
// N + (D >> 1) < 2^24; out <= 255 without a clamp.  Flat images are fixed
// points; for S >= 4096 every r[d] is 255 and the rule is gaussianK's own
// (sum + DIV/2) / DIV.  On RGB it is per channel, not OpenCV's joint colour
// distance.
#pragma once

#include <array>
#include <string>
#include <utility>
#include <vector>

#include "stripe/common.h"
#include "stripe/stencil_defs.h"

namespace stripe {

enum class OpKind : int {
  Gray = 0,
  Contrast,
  Invert,
  Brightness,
  Threshold,
  Expand,   // 1 -> 3 channels (GRAY2BGR, kernel.cu:210)
  Stencil,  // integer stencil with compile-time coefficients (stencil_defs.h)
  Conv,     // float KxK convolution (blur:K, conv:...), MFMA path on GPU
  ColorMatrix,  // 3 -> 3 channels: out_c = sat((sum_k q[c][k] p_k + qb[c] + 2048) >> 12)
  Stat,     // per-byte table built at run time from the global histogram (Op::stat)
  Hold,     // slot op: the current image also becomes the held image
  Swap,     // slot op: current and held exchange roles
  Combine,  // two-input pointwise op on (current, held) (Op::comb)
};

enum class CombineKind : int { Add = 0, Sub, RSub, AbsDiff, Min, Max, LinComb, Above, kCount };
const char* combine_name(CombineKind k);

enum class StatKind : int { Equalize = 0, AutoContrast = 1, Otsu = 2 };

// 256 counts per channel, [c * 256 + v]; C = 1 or 3 (0: empty).
struct Histogram {
  int C = 0;
  std::vector<uint64_t> bins;

  Histogram() = default;
  explicit Histogram(int c) : C(c), bins((size_t)256 * c, 0) {}
  uint64_t at(int c, int v) const { return bins[(size_t)c * 256 + v]; }
  uint64_t total() const {
    uint64_t n = 0;
    for (uint64_t b : bins) n += b;
    return n;
  }
};

enum class GrayMode : int { BT601 = 0, Ref = 1 };
enum class RoundMode : int { Trunc = 0, Nearest = 1 };

// One value per row of STRIPE_STENCILS (stencil_defs.h), in its order.
enum class StencilId : int {
#define STRIPE_STENCIL_ID(Id, ...) Id,
  STRIPE_STENCILS(STRIPE_STENCIL_ID)
#undef STRIPE_STENCIL_ID
  kCount
};

// Rank (order-statistic) filters over the K x K window: no weights, the output
// is the minimum (erode), maximum (dilate) or the element K*K/2 of the sorted
// window (median).
enum class Rank : int { None = 0, Min, Max, Median };
const char* rank_name(Rank r);

struct StencilInfo {
  StencilId id;
  const char* name;                // canonical spelling: names[0]
  std::vector<const char*> names;  // every spelling (STRIPE_STENCILS)
  int K;                 // window size (odd)
  bool separable;        // weights = w1 (x) w1
  bool sobel;            // sat(|Gx|+|Gy|), or with l2: sat(round(sqrt(Gx^2 + Gy^2)))
  bool l2 = false;
  int div;               // out = sat(floor((sum + div/2) / div)) (div==1: sat(sum))
  std::vector<int> w;    // K*K row-major [dy][dx] (correlation, like filter2D)
  std::vector<int> w1;   // separable 1-D taps
  Rank rank = Rank::None;  // rank filter: w / w1 empty, div 1
  // bilateral filter: w = the spatial weights ws, w1 = g, div 1; the range
  // table travels with the op and the pass (Op::range, Pass::range)
  bool bilateral = false;
};

const StencilInfo& stencil_info(StencilId id);
bool stencil_from_name(const std::string& name, StencilId* out);

struct Op {
  OpKind kind = OpKind::Gray;
  GrayMode gray = GrayMode::BT601;
  RoundMode round = RoundMode::Trunc;
  float fval = 0.f;  // contrast factor
  int ival = 0;      // brightness delta / threshold / autocontrast Pq (hundredths of a percent)
  StatKind stat = StatKind::Equalize;  // OpKind::Stat
  StencilId sid = StencilId::Gaussian5;
  int cm[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // colour matrix: q row-major, then qb (kColorShift)
  CombineKind comb = CombineKind::Add;  // OpKind::Combine
  int cq[3] = {0, 0, 0};                // lincomb / blend: qa, qb, qc (kColorShift); above: d in ival
  double sigma = 0.0;                   // bilateral: the range sigma S
  std::array<uint8_t, 256> range{};     // bilateral: r[d] (bilateral_range_table)
  int K = 0;                  // conv window
  std::vector<float> weights; // conv: K*K f32 weights
  std::vector<float> sep_h, sep_v;  // conv: 1-D factors when weights[dy][dx] = sep_v[dy] * sep_h[dx]
  // conv precision on the MFMA path: 3 = weights as 24-bit fixed point (an
  // output differs from the f64 result only within ~1e-4 of a rounding tie),
  // 2 = 16-bit ("conv:K:w..:lsb", every output within 1 LSB, 2/3 of the MFMAs)
  int conv_digits = 3;
  std::string text;           // canonical spelling
  bool has_border = false;    // per-op border override ("gaussian5@replicate")
  Border border = Border::Reflect101;

  bool pointwise() const { return kind != OpKind::Stencil && kind != OpKind::Conv; }
  bool slot() const { return kind == OpKind::Hold || kind == OpKind::Swap; }
  int radius() const;
  int channels_out(int cin) const;
};

// Parse "gray:ref,contrast:3.5,emboss3" (also presets "ref-gpu", "ref-cpu").
std::vector<Op> parse_chain(const std::string& spec);
// The (syntax, one-line description) rows of the parser's token table, in its order.
std::vector<std::pair<std::string, std::string>> filter_catalogue();
std::string chain_to_string(const std::vector<Op>& ops);

// Colour matrix arithmetic (the one definition every layer mirrors).
constexpr int kColorShift = 12;
inline uint8_t color_matrix_channel(const int* cm, int c, int r, int g, int b) {
  const int v = (cm[3 * c] * r + cm[3 * c + 1] * g + cm[3 * c + 2] * b + cm[9 + c] + (1 << (kColorShift - 1))) >>
                kColorShift;  // arithmetic shift: floor
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// Combine arithmetic (rules at the top of this file; the one definition every
// layer calls): byte x of the current image, byte h of the held image.
inline uint8_t combine_rule(CombineKind k, const int* cq, int d, uint8_t x, uint8_t h) {
  const int X = x, H = h;
  int v = 0;
  switch (k) {
    case CombineKind::Add: v = X + H; break;
    case CombineKind::Sub: v = H - X; break;
    case CombineKind::RSub: v = X - H; break;
    case CombineKind::AbsDiff: v = X > H ? X - H : H - X; break;
    case CombineKind::Min: v = X < H ? X : H; break;
    case CombineKind::Max: v = X > H ? X : H; break;
    case CombineKind::LinComb:
      v = (cq[0] * X + cq[1] * H + cq[2] + (1 << (kColorShift - 1))) >> kColorShift;  // arithmetic shift: floor
      break;
    case CombineKind::Above: return H - X + d > 0 ? 255 : 0;
    default: break;
  }
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
inline uint8_t combine_u8(const Op& op, uint8_t x, uint8_t h) { return combine_rule(op.comb, op.cq, op.ival, x, h); }

// Bilateral filter (rule at the top of this file).  The range table of sigma S
// (the parser's one call), and the rounded quotient of a pixel's sums.
std::array<uint8_t, 256> bilateral_range_table(double S);
inline uint8_t bilateral_finish(uint32_t N, uint32_t D) { return (uint8_t)((N + (D >> 1)) / D); }

// Statistic ops (rules at the top of this file): the table of `op`
// (OpKind::Stat) for an image with histogram `h` (channels pooled), and Otsu's
// level T in [1, 255].  The one definition every layer calls.
std::array<uint8_t, 256> stat_lut(const Op& op, const Histogram& h);
int otsu_level(const Histogram& h);

// Gaussian weights exactly as specified for blur:K (OpenCV getGaussianKernel sigma rule).
std::vector<double> gaussian_1d(int K, double sigma);

// ---- pointwise semantics (u8 -> u8 per channel) ----
uint8_t apply_pointwise_u8(const Op& op, uint8_t p);
// Gray conversion of one pixel given semantic R, G, B (PPM order).
uint8_t gray_pixel(GrayMode m, uint8_t r, uint8_t g, uint8_t b);

// Exact integer replacement of trunc((double)x * w) for x in [0,255]:
// returns (mult, shift) with (x*mult)>>shift == trunc(x*w) for all x, or false.
bool find_trunc_magic(double w, uint32_t* mult, int* shift);

}  // namespace stripe
