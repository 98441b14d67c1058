// Distance transform: checks, the golden two-step definition, its derived forms
// and the disc morphology built from them (the rule: stripe/distance.h).
#include "stripe/distance.h"

#include <algorithm>
#include <cmath>

#include "stripe/common.h"

namespace stripe {

bool parse_distance_to(const std::string& token) {
  if (token == "background") return false;
  if (token == "foreground") return true;
  fail("distance: to must be background or foreground, got '" + token + "'");
}

DiskOp parse_disk_op(const std::string& token) {
  if (token == "erode") return DiskOp::Erode;
  if (token == "dilate") return DiskOp::Dilate;
  if (token == "open") return DiskOp::Open;
  if (token == "close") return DiskOp::Close;
  fail("distance: the disc operation must be erode, dilate, open or close, got '" + token + "'");
}

void check_distance(int W, int H, int C) {
  STRIPE_CHECK(C == 1, "distance: needs a 1-channel image, got C = " << C << "; convert first (gray, threshold, ...)");
  STRIPE_CHECK(W >= 1 && H >= 1, "distance: empty image (" << W << "x" << H << ")");
  STRIPE_CHECK(W <= kDistanceMaxSide && H <= kDistanceMaxSide,
               "distance: " << W << "x" << H << " has a side above " << kDistanceMaxSide);
}

int32_t check_radius(double r) {
  STRIPE_CHECK(std::isfinite(r) && r >= 0.0, "distance: the radius must be finite and not negative, got " << r);
  const double t = std::floor(r * r);
  return t >= (double)(INT32_MAX - 1) ? INT32_MAX - 1 : (int32_t)t;
}

void check_distance_mode(int mode, int64_t t) {
  STRIPE_CHECK(mode >= 0 && mode <= (int)DistanceMode::MaskWithin, "distance: unknown mode " << mode);
  STRIPE_CHECK(t >= 0 && t < INT32_MAX, "distance: the threshold must lie in 0..2^31 - 2, got " << t);
}

void golden_distance(const Image& img, bool to_foreground, std::vector<int32_t>* out) {
  check_distance(img.W, img.H, img.C);
  const int W = img.W, H = img.H;
  const uint8_t* s = img.data.data();
  constexpr int64_t kNoSite = -1;
  // g(x, y): the vertical distance to the nearest site of column x, from one down and one up scan
  std::vector<int64_t> g((size_t)W * H, kNoSite);
  for (int x = 0; x < W; ++x) {
    int64_t d = kNoSite;
    for (int y = 0; y < H; ++y) {
      const bool site = (s[(size_t)y * W + x] != 0) == to_foreground;
      d = site ? 0 : (d == kNoSite ? kNoSite : d + 1);
      g[(size_t)y * W + x] = d;
    }
    d = kNoSite;
    for (int y = H - 1; y >= 0; --y) {
      const bool site = (s[(size_t)y * W + x] != 0) == to_foreground;
      d = site ? 0 : (d == kNoSite ? kNoSite : d + 1);
      int64_t& e = g[(size_t)y * W + x];
      if (d != kNoSite && (e == kNoSite || d < e)) e = d;
    }
  }
  // d2(x, y) = min over all x' of (x - x')^2 + g(x', y)^2
  out->assign((size_t)W * H, kDistanceNone);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int64_t best = kDistanceNone;
      for (int c = 0; c < W; ++c) {
        const int64_t gv = g[(size_t)y * W + c];
        if (gv == kNoSite) continue;
        best = std::min(best, (int64_t)(x - c) * (x - c) + gv * gv);
      }
      (*out)[(size_t)y * W + x] = (int32_t)best;
    }
}

Image golden_distance_u8(const Image& img, bool to_foreground) {
  std::vector<int32_t> d;
  golden_distance(img, to_foreground, &d);
  Image out(img.W, img.H, 1);
  for (size_t p = 0; p < d.size(); ++p) out.data[p] = distance_u8(d[p]);
  return out;
}

Image golden_distance_mask(const Image& img, bool to_foreground, int32_t t, bool keep_above) {
  check_distance_mode((int)DistanceMode::MaskAbove, t);
  std::vector<int32_t> d;
  golden_distance(img, to_foreground, &d);
  Image out(img.W, img.H, 1);
  for (size_t p = 0; p < d.size(); ++p) out.data[p] = distance_mask(d[p], t, keep_above);
  return out;
}

Image golden_disk_morph(const Image& img, DiskOp op, double radius) {
  check_distance(img.W, img.H, img.C);
  const int32_t t = check_radius(radius);
  switch (op) {
    case DiskOp::Erode: return golden_distance_mask(img, false, t, true);
    case DiskOp::Dilate: return golden_distance_mask(img, true, t, false);
    case DiskOp::Open: return golden_distance_mask(golden_distance_mask(img, false, t, true), true, t, false);
    case DiskOp::Close: return golden_distance_mask(golden_distance_mask(img, true, t, false), false, t, true);
  }
  fail("distance: unknown disc operation");
}

}  // namespace stripe
