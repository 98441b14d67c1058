// Mesh warp rule (see remap.h): the mesh builders, their parsers and the golden loop.
#include "stripe/remap.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "stripe/common.h"

namespace stripe {

using namespace spec;  // parse_number, parse_uint, num (warp.h)

namespace {
// "a<sep>b<sep>...": between lo and hi numbers
bool split_numbers(const std::string& s, char sep, int lo, int hi, std::vector<double>* out) {
  out->clear();
  size_t pos = 0;
  for (;;) {
    const size_t e = s.find(sep, pos);
    double v;
    if (!parse_number(s.substr(pos, e == std::string::npos ? e : e - pos), &v)) return false;
    out->push_back(v);
    if ((int)out->size() > hi) return false;
    if (e == std::string::npos) break;
    pos = e + 1;
  }
  return (int)out->size() >= lo;
}

// ":WxH" behind `colon` (npos: none)
void parse_size(const std::string& token, size_t colon, const std::string& what, int* W2, int* H2) {
  *W2 = *H2 = 0;
  if (colon == std::string::npos) return;
  const std::string size = token.substr(colon + 1);
  const size_t x = size.find('x');
  STRIPE_CHECK(x != std::string::npos, what << "expected a size WxH after ':'");
  *W2 = parse_uint(size.substr(0, x));
  *H2 = parse_uint(size.substr(x + 1));
  STRIPE_CHECK(*W2 >= 1 && *H2 >= 1, what << "destination size outside 1.." << kWarpMaxSize);
}

void check_sizes(const std::string& what, int W, int H, int W2, int H2) {
  STRIPE_CHECK(W >= 1 && W <= kWarpMaxSize && H >= 1 && H <= kWarpMaxSize,
               what << "source size " << W << "x" << H << " outside 1.." << kWarpMaxSize);
  STRIPE_CHECK(W2 >= 1 && W2 <= kWarpMaxSize && H2 >= 1 && H2 <= kWarpMaxSize,
               what << "destination size " << W2 << "x" << H2 << " outside 1.." << kWarpMaxSize);
}

int32_t node_of(double pos, const std::string& what) {
  const double lim = std::ldexp(1.0, kRemapNodeBits);
  STRIPE_CHECK(std::isfinite(pos), what << "non-finite source position");
  const double q = std::nearbyint(std::ldexp(pos, kRemapQ));
  STRIPE_CHECK(std::fabs(pos) < lim && std::fabs(q) < std::ldexp(lim, kRemapQ),
               what << "a node at " << pos << " lies at or beyond 2^" << kRemapNodeBits << " pixels");
  return (int32_t)q;
}

// nodes of a map pos(x, y) -> (px, py) over the grid of a spacing
template <class F>
Mesh build_mesh(int s, int W2, int H2, const std::string& what, F&& pos) {
  Mesh m;
  m.shift = s, m.W2 = W2, m.H2 = H2;
  const int gw = m.gw(), gh = m.gh();
  m.nodes.resize((size_t)gw * gh * 2);
  for (int i = 0; i < gh; ++i)
    for (int j = 0; j < gw; ++j) {
      double px, py;
      pos((double)j * (1 << s), (double)i * (1 << s), &px, &py);
      m.nodes[((size_t)i * gw + j) * 2] = node_of(px, what);
      m.nodes[((size_t)i * gw + j) * 2 + 1] = node_of(py, what);
    }
  return m;
}

inline uint8_t tap(const Image& in, int64_t iy, int64_t ix, int ch, const RemapMesh& m) {
  if (m.border == WarpBorder::Replicate) {
    iy = std::min<int64_t>(std::max<int64_t>(iy, 0), in.H - 1);
    ix = std::min<int64_t>(std::max<int64_t>(ix, 0), in.W - 1);
  } else if (ix < 0 || iy < 0 || ix >= in.W || iy >= in.H) {
    return m.fill;
  }
  return in.row((int)iy)[(size_t)ix * in.C + ch];
}
}  // namespace

int remap_shift(int spacing, const std::string& token) {
  for (int s = 0; s <= kRemapMaxShift; ++s)
    if (spacing == 1 << s) return s;
  fail("remap '" + token + "': spacing " + std::to_string(spacing) + " is not a power of two in 1..64");
}

void check_mesh(const RemapMesh& m, int64_t count, bool check_nodes, const std::string& token) {
  const std::string what = "remap '" + token + "': ";
  STRIPE_CHECK(m.W2 >= 1 && m.W2 <= kWarpMaxSize && m.H2 >= 1 && m.H2 <= kWarpMaxSize,
               what << "destination size " << m.W2 << "x" << m.H2 << " outside 1.." << kWarpMaxSize);
  STRIPE_CHECK(m.shift >= 0 && m.shift <= kRemapMaxShift, what << "spacing is not a power of two in 1..64");
  STRIPE_CHECK(m.nodes, what << "empty mesh");
  const int64_t want = (int64_t)m.gh() * m.gw() * 2;
  STRIPE_CHECK(count == want, what << "a mesh of spacing " << (1 << m.shift) << " for " << m.W2 << "x" << m.H2
                                   << " has shape " << m.gh() << "x" << m.gw() << "x2 (" << want
                                   << " integers), got " << count);
  STRIPE_CHECK((int)m.mode >= 0 && (int)m.mode < 2 && (int)m.border >= 0 && (int)m.border < 2,
               what << "bad mode or border");
  if (check_nodes) {
    const int64_t lim = int64_t(1) << (kRemapNodeBits + kRemapQ);
    for (int64_t k = 0; k < want; ++k)
      STRIPE_CHECK(m.nodes[k] > -lim && m.nodes[k] < lim,
                   what << "a node at " << std::ldexp((double)m.nodes[k], -kRemapQ) << " lies at or beyond 2^"
                        << kRemapNodeBits << " pixels");
  }
}

Mesh perspective_mesh(const double Hm[9], bool inverse, int W, int H, int W2, int H2, int spacing,
                      const std::string& token) {
  const std::string what = "remap '" + token + "': ";
  check_sizes(what, W, H, W2, H2);
  for (int k = 0; k < 9; ++k) STRIPE_CHECK(std::isfinite(Hm[k]), what << "non-finite number in the matrix");
  const double det = Hm[0] * (Hm[4] * Hm[8] - Hm[5] * Hm[7]) - Hm[1] * (Hm[3] * Hm[8] - Hm[5] * Hm[6]) +
                     Hm[2] * (Hm[3] * Hm[7] - Hm[4] * Hm[6]);
  STRIPE_CHECK(std::isfinite(det) && det != 0.0, what << "singular matrix (determinant " << det << ")");
  double q[9];
  if (inverse) {
    std::memcpy(q, Hm, sizeof q);
  } else {
    const double adj[9] = {Hm[4] * Hm[8] - Hm[5] * Hm[7], Hm[2] * Hm[7] - Hm[1] * Hm[8], Hm[1] * Hm[5] - Hm[2] * Hm[4],
                           Hm[5] * Hm[6] - Hm[3] * Hm[8], Hm[0] * Hm[8] - Hm[2] * Hm[6], Hm[2] * Hm[3] - Hm[0] * Hm[5],
                           Hm[3] * Hm[7] - Hm[4] * Hm[6], Hm[1] * Hm[6] - Hm[0] * Hm[7], Hm[0] * Hm[4] - Hm[1] * Hm[3]};
    for (int k = 0; k < 9; ++k) {
      q[k] = adj[k] / det;
      STRIPE_CHECK(std::isfinite(q[k]), what << "singular matrix (determinant " << det << ")");
    }
  }
  // The grid of a spacing extends to ((gw - 1) S, (gh - 1) S).  w is linear, so it is positive on the
  // extent iff it is at the four corners; the sign of the matrix is free.
  auto corners_ok = [&](int s, double* sign, double* wmin, double F[2]) {
    const double ex = (double)(remap_grid(W2, s) - 1) * (1 << s), ey = (double)(remap_grid(H2, s) - 1) * (1 << s);
    int pos = 0, neg = 0;
    double wm = INFINITY;
    F[0] = F[1] = 0;
    for (int k = 0; k < 4; ++k) {
      const double x = k & 1 ? ex : 0, y = k & 2 ? ey : 0;
      const double w = q[6] * x + q[7] * y + q[8];
      pos += w > 0, neg += w < 0;
      wm = std::min(wm, std::fabs(w));
      F[0] = std::max(F[0], std::fabs((q[0] * x + q[1] * y + q[2]) / w));
      F[1] = std::max(F[1], std::fabs((q[3] * x + q[4] * y + q[5]) / w));
    }
    *sign = neg == 4 ? -1.0 : 1.0;
    *wmin = wm;
    return pos == 4 || neg == 4;
  };
  int s = -1;
  double sign = 1, wmin = 0, F[2];
  if (spacing != 0) {
    s = remap_shift(spacing, token);
    STRIPE_CHECK(corners_ok(s, &sign, &wmin, F), what << "the horizon crosses the destination");
  } else {
    for (int c = kRemapMaxShift; c >= 0 && s < 0; --c) {
      if (!corners_ok(c, &sign, &wmin, F)) continue;  // (a smaller grid may stay on one side)
      if (c == 0) {
        s = 0;
        break;
      }
      const double g = std::fabs(q[6]), h = std::fabs(q[7]);
      bool ok = true;
      for (int r = 0; r < 2; ++r) {
        const double d2 = 2.0 * (g * (std::fabs(q[3 * r]) + F[r] * g) + h * (std::fabs(q[3 * r + 1]) + F[r] * h)) /
                          (wmin * wmin);
        ok = ok && std::ldexp(1.0, 2 * c) / 8.0 * d2 <= std::ldexp(1.0, -10);
      }
      if (ok) s = c;
    }
    STRIPE_CHECK(s >= 0, what << "the horizon crosses the destination");
  }
  return build_mesh(s, W2, H2, what, [&](double x, double y, double* px, double* py) {
    const double w = sign * (q[6] * x + q[7] * y + q[8]);
    *px = sign * (q[0] * x + q[1] * y + q[2]) / w;
    *py = sign * (q[3] * x + q[4] * y + q[5]) / w;
  });
}

void perspective_from_points(const double src[8], const double dst[8], double Hm[9], const std::string& token) {
  const std::string what = "remap '" + token + "': ";
  for (int k = 0; k < 8; ++k)
    STRIPE_CHECK(std::isfinite(src[k]) && std::isfinite(dst[k]), what << "non-finite number in the points");
  // a x + b y + c - u (g x + h y) = u,  d x + e y + f - v (g x + h y) = v
  double A[8][9];
  double scale = 1;
  for (int k = 0; k < 4; ++k) {
    const double x = src[2 * k], y = src[2 * k + 1], u = dst[2 * k], v = dst[2 * k + 1];
    const double r0[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, u}, r1[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, v};
    std::memcpy(A[2 * k], r0, sizeof r0);
    std::memcpy(A[2 * k + 1], r1, sizeof r1);
    scale = std::max({scale, std::fabs(x), std::fabs(y), std::fabs(u), std::fabs(v)});
  }
  // Gaussian elimination with partial pivoting on rows scaled to unit largest entry
  for (int r = 0; r < 8; ++r) {
    double mx = 0;
    for (int c = 0; c < 8; ++c) mx = std::max(mx, std::fabs(A[r][c]));
    STRIPE_CHECK(mx > 0, what << "degenerate point set");
    for (int c = 0; c < 9; ++c) A[r][c] /= mx;
  }
  for (int c = 0; c < 8; ++c) {
    int p = c;
    for (int r = c + 1; r < 8; ++r)
      if (std::fabs(A[r][c]) > std::fabs(A[p][c])) p = r;
    STRIPE_CHECK(std::fabs(A[p][c]) > 1e-12, what << "degenerate point set (three points on a line, or equal points)");
    if (p != c)
      for (int k = 0; k < 9; ++k) std::swap(A[p][k], A[c][k]);
    for (int r = 0; r < 8; ++r) {
      if (r == c) continue;
      const double f = A[r][c] / A[c][c];
      if (f != 0)
        for (int k = c; k < 9; ++k) A[r][k] -= f * A[c][k];
    }
  }
  for (int k = 0; k < 8; ++k) {
    Hm[k] = A[k][8] / A[k][k];
    STRIPE_CHECK(std::isfinite(Hm[k]), what << "degenerate point set");
  }
  Hm[8] = 1;
  const double det = Hm[0] * (Hm[4] * Hm[8] - Hm[5] * Hm[7]) - Hm[1] * (Hm[3] * Hm[8] - Hm[5] * Hm[6]) +
                     Hm[2] * (Hm[3] * Hm[7] - Hm[4] * Hm[6]);
  STRIPE_CHECK(std::isfinite(det) && std::fabs(det) > 1e-12 / (scale * scale),
               what << "degenerate point set (three points on a line, or equal points)");
}

QuadSpec parse_quad_spec(const std::string& token) {
  const std::string what = "quad spec '" + token + "': ";
  QuadSpec qs;
  const size_t colon = token.find(':');
  const std::string body = token.substr(0, colon);
  size_t pos = 0;
  for (int k = 0; k < 4; ++k) {
    const size_t semi = body.find(';', pos);
    STRIPE_CHECK((semi == std::string::npos) == (k == 3), what << "expected four points x0,y0;x1,y1;x2,y2;x3,y3[:WxH]");
    std::vector<double> xy;
    STRIPE_CHECK(split_numbers(body.substr(pos, semi == std::string::npos ? semi : semi - pos), ',', 2, 2, &xy),
                 what << "expected four points x0,y0;x1,y1;x2,y2;x3,y3[:WxH]");
    STRIPE_CHECK(std::isfinite(xy[0]) && std::isfinite(xy[1]), what << "non-finite number in the points");
    qs.pts[2 * k] = xy[0], qs.pts[2 * k + 1] = xy[1];
    pos = semi + 1;
  }
  parse_size(token, colon, what, &qs.W2, &qs.H2);
  if (qs.W2 == 0) quad_default_size(qs.pts, &qs.W2, &qs.H2, token);
  return qs;
}

void quad_default_size(const double p[8], int* W2, int* H2, const std::string& token) {
  for (int k = 0; k < 8; ++k) STRIPE_CHECK(std::isfinite(p[k]), "remap '" << token << "': non-finite number in the points");
  auto dist = [&](int a, int b) { return std::hypot(p[2 * a] - p[2 * b], p[2 * a + 1] - p[2 * b + 1]); };
  const double w = std::rint(std::max(dist(1, 0), dist(2, 3))) + 1, h = std::rint(std::max(dist(3, 0), dist(2, 1))) + 1;
  STRIPE_CHECK(w >= 1 && w <= kWarpMaxSize && h >= 1 && h <= kWarpMaxSize,
               "remap '" << token << "': destination size " << w << "x" << h << " outside 1.." << kWarpMaxSize);
  *W2 = (int)w, *H2 = (int)h;
}

void quad_matrix(const double pts[8], int W2, int H2, double Hm[9], const std::string& token) {
  STRIPE_CHECK(W2 >= 1 && W2 <= kWarpMaxSize && H2 >= 1 && H2 <= kWarpMaxSize,
               "remap '" << token << "': destination size " << W2 << "x" << H2 << " outside 1.." << kWarpMaxSize);
  // a side of one pixel keeps its corners apart: the matrix of a 1-pixel axis is that of a 2-pixel one
  const double ex = std::max(W2 - 1, 1), ey = std::max(H2 - 1, 1);
  const double dst[8] = {0, 0, ex, 0, ex, ey, 0, ey};
  perspective_from_points(pts, dst, Hm, token);
}

PerspectiveSpec parse_perspective_spec(const std::string& token) {
  const std::string what = "perspective spec '" + token + "': ";
  PerspectiveSpec p;
  const size_t colon = token.find(':');
  std::vector<double> v;
  STRIPE_CHECK(split_numbers(token.substr(0, colon), ';', 9, 9, &v), what << "expected nine numbers h00;...;h22[:WxH]");
  for (int k = 0; k < 9; ++k) {
    STRIPE_CHECK(std::isfinite(v[k]), what << "non-finite number in the matrix");
    p.Hm[k] = v[k];
  }
  parse_size(token, colon, what, &p.W2, &p.H2);
  return p;
}

RadialSpec parse_undistort_spec(const std::string& token) {
  const std::string what = "undistort spec '" + token + "': ";
  std::vector<double> v;
  STRIPE_CHECK(split_numbers(token, ';', 1, 5, &v) && v.size() != 4, what << "expected k1[;k2[;f[;cx;cy]]]");
  for (double d : v) STRIPE_CHECK(std::isfinite(d), what << "non-finite number");
  RadialSpec r;
  r.k1 = v[0];
  if (v.size() > 1) r.k2 = v[1];
  if (v.size() > 2) r.has_f = true, r.f = v[2];
  if (v.size() > 3) r.has_centre = true, r.cx = v[3], r.cy = v[4];
  return r;
}

RadialSpec radial_resolve(const RadialSpec& r, int W, int H) {
  RadialSpec o = r;
  if (!o.has_f) o.f = 0.5 * std::hypot((double)W, (double)H);
  if (!o.has_centre) o.cx = (W - 1) * 0.5, o.cy = (H - 1) * 0.5;
  o.has_f = o.has_centre = true;
  return o;
}

std::string perspective_token(const double Hm[9], int W2, int H2) {
  std::string t = "perspective:";
  for (int i = 0; i < 9; ++i) t += (i ? ";" : "") + num(Hm[i]);
  return t + ":" + std::to_string(W2) + "x" + std::to_string(H2);
}

std::string quad_token(const double pts[8], int W2, int H2) {
  std::string t = "quad:";
  for (int i = 0; i < 4; ++i) t += (i ? ";" : "") + num(pts[2 * i]) + "," + num(pts[2 * i + 1]);
  return t + ":" + std::to_string(W2) + "x" + std::to_string(H2);
}

std::string undistort_token(const RadialSpec& r) {
  return "undistort:" + num(r.k1) + ";" + num(r.k2) + ";" + num(r.f) + ";" + num(r.cx) + ";" + num(r.cy);
}

Mesh radial_mesh(const RadialSpec& r, int W, int H, int spacing, const std::string& token) {
  const std::string what = "remap '" + token + "': ";
  check_sizes(what, W, H, W, H);
  const RadialSpec rr = radial_resolve(r, W, H);
  const double f = rr.f, cx = rr.cx, cy = rr.cy;
  STRIPE_CHECK(std::isfinite(r.k1) && std::isfinite(r.k2) && std::isfinite(f) && std::isfinite(cx) && std::isfinite(cy),
               what << "non-finite number");
  STRIPE_CHECK(f > 0, what << "the focal length must be positive, got f = " << f);
  int s = -1;
  if (spacing != 0) {
    s = remap_shift(spacing, token);
  } else {
    for (int c = kRemapMaxShift; c >= 0 && s < 0; --c) {
      const double ex = (double)(remap_grid(W, c) - 1) * (1 << c), ey = (double)(remap_grid(H, c) - 1) * (1 << c);
      const double rho = std::hypot(std::max(std::fabs(cx), std::fabs(ex - cx)), std::max(std::fabs(cy), std::fabs(ey - cy))) / f;
      const double d2 = (8 * std::fabs(r.k1) * rho + 32 * std::fabs(r.k2) * rho * rho * rho) / f;
      if (c == 0 || std::ldexp(1.0, 2 * c) / 8.0 * d2 <= std::ldexp(1.0, -10)) s = c;
    }
  }
  return build_mesh(s, W, H, what, [&](double x, double y, double* px, double* py) {
    const double xn = (x - cx) / f, yn = (y - cy) / f, r2 = xn * xn + yn * yn, k = 1 + r.k1 * r2 + r.k2 * r2 * r2;
    *px = cx + f * xn * k;
    *py = cy + f * yn * k;
  });
}

Image golden_remap(const Image& in, const RemapMesh& m) {
  STRIPE_CHECK(in.C == 1 || in.C == 3, "remap: image must have 1 or 3 channels, got C = " << in.C);
  STRIPE_CHECK(in.W >= 1 && in.H >= 1 && in.W <= kWarpMaxSize && in.H <= kWarpMaxSize,
               "remap: source size " << in.W << "x" << in.H << " outside 1.." << kWarpMaxSize);
  check_mesh(m, (int64_t)m.gh() * m.gw() * 2, true);
  const int s = m.shift, gw = m.gw();
  Image out(m.W2, m.H2, in.C, NoInit{});
  for (int y = 0; y < m.H2; ++y)
    for (int x = 0; x < m.W2; ++x) {
      const int64_t Px = remap_P(m.nodes, gw, s, x, y, 0), Py = remap_P(m.nodes, gw, s, x, y, 1);
      uint8_t* o = out.row(y) + (size_t)x * in.C;
      if (m.mode == WarpMode::Nearest) {
        const int64_t ix = (Px + (int64_t(1) << (11 + 2 * s))) >> (12 + 2 * s);
        const int64_t iy = (Py + (int64_t(1) << (11 + 2 * s))) >> (12 + 2 * s);
        for (int ch = 0; ch < in.C; ++ch) o[ch] = tap(in, iy, ix, ch, m);
      } else {
        const int64_t X = (Px + (int64_t(1) << (3 + 2 * s))) >> (4 + 2 * s);
        const int64_t Y = (Py + (int64_t(1) << (3 + 2 * s))) >> (4 + 2 * s);
        const int64_t ix = X >> 8, iy = Y >> 8;
        const uint32_t fx = (uint32_t)(X & 255), fy = (uint32_t)(Y & 255);
        for (int ch = 0; ch < in.C; ++ch)
          o[ch] = (uint8_t)warp_bilinear(tap(in, iy, ix, ch, m), tap(in, iy, ix + 1, ch, m), tap(in, iy + 1, ix, ch, m),
                                         tap(in, iy + 1, ix + 1, ch, m), fx, fy);
      }
    }
  return out;
}

}  // namespace stripe
