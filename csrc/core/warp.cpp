// Affine warp rule (see warp.h): the parsers, the quantiser, the rotation
// matrix and the golden loop.
#include "stripe/warp.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stripe/common.h"

namespace stripe {

namespace spec {
bool parse_number(const std::string& s, double* v) {
  if (s.empty() || s.size() > 64) return false;
  for (char c : s)
    if (c == 'x' || c == 'X' || c == 'p' || c == 'P' || std::isspace((unsigned char)c)) return false;
  char* end = nullptr;
  *v = std::strtod(s.c_str(), &end);
  return end == s.c_str() + s.size();
}

int parse_uint(const std::string& s) {
  if (s.empty() || s.size() > 5) return -1;
  int v = 0;
  for (char c : s) {
    if (c < '0' || c > '9') return -1;
    v = v * 10 + (c - '0');
  }
  return v <= kWarpMaxSize ? v : -1;
}

std::string num(double v) {
  char buf[40];
  std::snprintf(buf, sizeof buf, "%.17g", v);
  double back = 0;
  for (int pass = 0; pass < 2; ++pass)
    for (int p = 1; p < 17; ++p) {
      char t[40];
      std::snprintf(t, sizeof t, "%.*g", p, v);
      if ((pass == 1 || !std::strchr(t, 'e')) && parse_number(t, &back) && back == v) return t;
    }
  return buf;
}
}  // namespace spec

using namespace spec;

namespace {
inline uint8_t tap(const Image& in, int iy, int ix, int ch, const WarpMap& m) {
  if (m.border == WarpBorder::Replicate) {
    iy = std::min(std::max(iy, 0), in.H - 1);
    ix = std::min(std::max(ix, 0), in.W - 1);
  } else if (ix < 0 || iy < 0 || ix >= in.W || iy >= in.H) {
    return m.fill;
  }
  return in.row(iy)[(size_t)ix * in.C + ch];
}
}  // namespace

const char* warp_mode_name(WarpMode m) { return m == WarpMode::Nearest ? "nearest" : "bilinear"; }
const char* warp_border_name(WarpBorder b) { return b == WarpBorder::Replicate ? "replicate" : "constant"; }

WarpMode parse_warp_mode(const std::string& token) {
  if (token == "bilinear") return WarpMode::Bilinear;
  if (token == "nearest") return WarpMode::Nearest;
  fail("warp: unknown mode '" + token + "' (bilinear | nearest)");
}

void parse_warp_border(const std::string& token, WarpBorder* border, uint8_t* fill) {
  *fill = 0;
  if (token == "replicate") {
    *border = WarpBorder::Replicate;
    return;
  }
  if (token == "constant") {
    *border = WarpBorder::Constant;
    return;
  }
  if (token.compare(0, 9, "constant:") == 0) {
    const int v = parse_uint(token.substr(9));
    STRIPE_CHECK(v >= 0 && v <= 255, "warp border '" << token << "': the fill value must be an integer in 0..255");
    *border = WarpBorder::Constant;
    *fill = (uint8_t)v;
    return;
  }
  fail("warp: unknown border '" + token + "' (constant[:V] | replicate)");
}

WarpMap warp_quantise(const double M[6], bool inverse, int W, int H, int W2, int H2, WarpMode mode, WarpBorder border,
                      uint8_t fill, const std::string& token) {
  const std::string what = "warp '" + token + "': ";
  STRIPE_CHECK(W >= 1 && W <= kWarpMaxSize && H >= 1 && H <= kWarpMaxSize,
               what << "source size " << W << "x" << H << " outside 1.." << kWarpMaxSize);
  STRIPE_CHECK(W2 >= 1 && W2 <= kWarpMaxSize && H2 >= 1 && H2 <= kWarpMaxSize,
               what << "destination size " << W2 << "x" << H2 << " outside 1.." << kWarpMaxSize);
  for (int i = 0; i < 6; ++i) STRIPE_CHECK(std::isfinite(M[i]), what << "non-finite number in the matrix");
  const double det = M[0] * M[4] - M[1] * M[3];
  STRIPE_CHECK(std::isfinite(det) && det != 0.0, what << "singular matrix (determinant " << det << ")");
  double inv[6];
  if (inverse) {
    for (int i = 0; i < 6; ++i) inv[i] = M[i];
  } else {
    inv[0] = M[4] / det, inv[1] = -M[1] / det, inv[2] = (M[1] * M[5] - M[2] * M[4]) / det;
    inv[3] = -M[3] / det, inv[4] = M[0] / det, inv[5] = (M[2] * M[3] - M[0] * M[5]) / det;
  }
  WarpMap m;
  for (int i = 0; i < 2; ++i) {
    for (int j = 0; j < 2; ++j) {
      const double v = inv[3 * i + j];
      // the range holds for the quantised value too: 64 - 2^-30 rounds to 2^30, which no layer takes
      STRIPE_CHECK(std::isfinite(v) && std::fabs(v) < kWarpMaxLinear &&
                       std::fabs(std::nearbyint(std::ldexp(v, kWarpQ))) < std::ldexp(kWarpMaxLinear, kWarpQ),
                   what << "inverse map coefficient " << v << " outside (-64, 64)");
      m.A[i][j] = (int32_t)std::nearbyint(std::ldexp(v, kWarpQ));
    }
    const double o = inv[3 * i + 2];
    STRIPE_CHECK(std::isfinite(o) && std::fabs(o) < kWarpMaxOffset &&
                     std::fabs(std::nearbyint(std::ldexp(o, kWarpQ))) < std::ldexp(kWarpMaxOffset, kWarpQ),
                 what << "inverse map offset " << o << " outside (-2^20, 2^20)");
    m.B[i] = (int64_t)std::nearbyint(std::ldexp(o, kWarpQ));
  }
  m.W2 = W2, m.H2 = H2;
  m.mode = mode, m.border = border, m.fill = fill;
  return m;
}

Rotation rotate_matrix(double deg, bool fit, int W, int H) {
  STRIPE_CHECK(std::isfinite(deg), "rotate: non-finite angle");
  STRIPE_CHECK(W >= 1 && W <= kWarpMaxSize && H >= 1 && H <= kWarpMaxSize,
               "rotate: size " << W << "x" << H << " outside 1.." << kWarpMaxSize);
  double r = std::fmod(deg, 360.0);
  if (r < 0) r += 360.0;
  double c, s;
  if (r == 0.0 || r == 360.0) c = 1, s = 0;
  else if (r == 90.0) c = 0, s = 1;
  else if (r == 180.0) c = -1, s = 0;
  else if (r == 270.0) c = 0, s = -1;
  else c = std::cos(r * (M_PI / 180.0)), s = std::sin(r * (M_PI / 180.0));
  Rotation o;
  o.W2 = W, o.H2 = H;
  if (fit) {
    o.W2 = std::max(1, (int)std::ceil(W * std::fabs(c) + H * std::fabs(s) - 1e-6));
    o.H2 = std::max(1, (int)std::ceil(W * std::fabs(s) + H * std::fabs(c) - 1e-6));
  }
  const double csx = (W - 1) * 0.5, csy = (H - 1) * 0.5, cdx = (o.W2 - 1) * 0.5, cdy = (o.H2 - 1) * 0.5;
  o.minv[0] = c, o.minv[1] = -s, o.minv[2] = csx - c * cdx + s * cdy;
  o.minv[3] = s, o.minv[4] = c, o.minv[5] = csy - s * cdx - c * cdy;
  return o;
}

WarpSpec parse_warp_spec(const std::string& token) {
  const std::string what = "warp spec '" + token + "': ";
  WarpSpec w;
  const size_t colon = token.find(':');
  const std::string mat = token.substr(0, colon);
  size_t pos = 0;
  for (int i = 0; i < 6; ++i) {
    const size_t semi = mat.find(';', pos);
    STRIPE_CHECK((semi == std::string::npos) == (i == 5), what << "expected six numbers a;b;c;d;e;f[:WxH]");
    STRIPE_CHECK(parse_number(mat.substr(pos, semi == std::string::npos ? semi : semi - pos), &w.M[i]),
                 what << "expected six numbers a;b;c;d;e;f[:WxH]");
    STRIPE_CHECK(std::isfinite(w.M[i]), what << "non-finite number in the matrix");
    pos = semi + 1;
  }
  if (colon != std::string::npos) {
    const std::string size = token.substr(colon + 1);
    const size_t x = size.find('x');
    STRIPE_CHECK(x != std::string::npos, what << "expected a size WxH after ':'");
    w.W2 = parse_uint(size.substr(0, x));
    w.H2 = parse_uint(size.substr(x + 1));
    STRIPE_CHECK(w.W2 >= 1 && w.H2 >= 1, what << "destination size outside 1.." << kWarpMaxSize);
  }
  return w;
}

RotateSpec parse_rotate_spec(const std::string& token) {
  const std::string what = "rotate spec '" + token + "': ";
  RotateSpec r;
  const size_t colon = token.find(':');
  STRIPE_CHECK(parse_number(token.substr(0, colon), &r.deg), what << "expected DEG[:same|fit]");
  STRIPE_CHECK(std::isfinite(r.deg), what << "non-finite angle");
  if (colon != std::string::npos) {
    const std::string f = token.substr(colon + 1);
    STRIPE_CHECK(f == "same" || f == "fit", what << "expected DEG[:same|fit]");
    r.fit = f == "fit";
  }
  return r;
}

std::string rotate_token(const RotateSpec& r) { return "rotate:" + num(r.deg) + (r.fit ? ":fit" : ":same"); }

std::string warp_token(const WarpSpec& s, int W2, int H2) {
  std::string t = "affine:";
  for (int i = 0; i < 6; ++i) t += (i ? ";" : "") + num(s.M[i]);
  return t + ":" + std::to_string(W2) + "x" + std::to_string(H2);
}

Image golden_warp(const Image& in, const WarpMap& m) {
  STRIPE_CHECK(in.C == 1 || in.C == 3, "warp: image must have 1 or 3 channels, got C = " << in.C);
  STRIPE_CHECK(in.W >= 1 && in.H >= 1 && in.W <= kWarpMaxSize && in.H <= kWarpMaxSize,
               "warp: source size " << in.W << "x" << in.H << " outside 1.." << kWarpMaxSize);
  STRIPE_CHECK(m.W2 >= 1 && m.H2 >= 1 && m.W2 <= kWarpMaxSize && m.H2 <= kWarpMaxSize,
               "warp: destination size " << m.W2 << "x" << m.H2 << " outside 1.." << kWarpMaxSize);
  Image out(m.W2, m.H2, in.C, NoInit{});
  for (int y = 0; y < m.H2; ++y)
    for (int x = 0; x < m.W2; ++x) {
      const int64_t sx = warp_sx(m, x, y), sy = warp_sy(m, x, y);
      uint8_t* o = out.row(y) + (size_t)x * in.C;
      if (m.mode == WarpMode::Nearest) {
        const int ix = (int)((sx + (1 << 23)) >> 24), iy = (int)((sy + (1 << 23)) >> 24);
        for (int ch = 0; ch < in.C; ++ch) o[ch] = tap(in, iy, ix, ch, m);
      } else {
        const int64_t X = (sx + (1 << 15)) >> 16, Y = (sy + (1 << 15)) >> 16;
        const int ix = (int)(X >> 8), iy = (int)(Y >> 8);
        const uint32_t fx = (uint32_t)(X & 255), fy = (uint32_t)(Y & 255);
        for (int ch = 0; ch < in.C; ++ch)
          o[ch] = (uint8_t)warp_bilinear(tap(in, iy, ix, ch, m), tap(in, iy, ix + 1, ch, m), tap(in, iy + 1, ix, ch, m),
                                         tap(in, iy + 1, ix + 1, ch, m), fx, fy);
      }
    }
  return out;
}

}  // namespace stripe
