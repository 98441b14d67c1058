// Canny edge detection and hysteresis thresholding: checks, parsers and the
// golden loops (the rule: stripe/canny.h).
#include "stripe/canny.h"

#include <vector>

namespace stripe {

CannyNorm parse_canny_norm(const std::string& token) {
  if (token == "l1") return CannyNorm::L1;
  if (token == "l2") return CannyNorm::L2;
  fail("canny: the norm must be l1 or l2, got '" + token + "'");
}

const char* canny_norm_name(CannyNorm n) { return n == CannyNorm::L2 ? "l2" : "l1"; }

void check_thresholds(int64_t low, int64_t high, int max) {
  STRIPE_CHECK(low >= 0 && low <= high && high <= max, "canny: the thresholds must be integers with 0 <= low <= high <= "
                                                           << max << ", got low = " << low << ", high = " << high);
}

namespace {
void check_canny_frame(int W, int H, int C) {
  STRIPE_CHECK(C == 1, "canny: needs a 1-channel image, got C = " << C << "; convert first (gray, threshold, ...)");
  STRIPE_CHECK(W >= 1 && H >= 1, "canny: empty image (" << W << "x" << H << ")");
  STRIPE_CHECK((int64_t)W * H <= kComponentsMaxPixels, "canny: " << W << "x" << H << " pixels exceed 2^31 - 2");
}
}  // namespace

void check_canny(int W, int H, int C, int64_t low, int64_t high, int norm, Border border) {
  check_canny_frame(W, H, C);
  check_thresholds(low, high, kCannyMaxThreshold);
  STRIPE_CHECK(norm == (int)CannyNorm::L1 || norm == (int)CannyNorm::L2, "canny: unknown norm " << norm);
  STRIPE_CHECK(border == Border::Reflect101 || border == Border::Replicate || border == Border::Constant,
               "canny: the border must be reflect101, replicate or constant (skip has no gradient at the frame edge)");
}

void check_hysteresis(int W, int H, int C, int64_t low, int64_t high, int conn) {
  check_canny_frame(W, H, C);
  check_thresholds(low, high, kHysteresisMaxThreshold);
  STRIPE_CHECK(conn == 4 || conn == 8, "canny: connectivity must be 4 or 8, got " << conn);
}

Image golden_canny_classes(const Image& img, int low, int high, CannyNorm norm, Border border) {
  check_canny(img.W, img.H, img.C, low, high, (int)norm, border);
  const int W = img.W, H = img.H;
  const bool l2 = norm == CannyNorm::L2;
  const uint32_t lo = l2 ? (uint32_t)low * low : (uint32_t)low, hi = l2 ? (uint32_t)high * high : (uint32_t)high;
  // the extended frame, written out: one pixel on every side is all the gradient of a frame pixel reads
  const size_t We = (size_t)W + 2, He = (size_t)H + 2;
  std::vector<uint8_t> P(We * He);
  for (size_t y = 0; y < He; ++y) {
    const int sy = border_index((int)y - 1, H, border);
    for (size_t x = 0; x < We; ++x) {
      const int sx = border_index((int)x - 1, W, border);
      P[y * We + x] = sy < 0 || sx < 0 ? 0 : img.data[(size_t)sy * W + sx];
    }
  }
  // the magnitude plane with a frame of zeros (a position outside the frame has magnitude 0), and the sectors
  std::vector<uint32_t> M(We * He, 0u);
  std::vector<uint8_t> S((size_t)W * H);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const uint8_t* p = P.data() + (size_t)y * We + x;  // the top left of the 3 x 3 neighbourhood
      const int a = p[0], b = p[1], c = p[2], d = p[We], f = p[We + 2], g = p[2 * We], h = p[2 * We + 1],
                i = p[2 * We + 2];
      const int gx = (c + 2 * f + i) - (a + 2 * d + g), gy = (g + 2 * h + i) - (a + 2 * b + c);
      M[(size_t)(y + 1) * We + x + 1] = canny_magnitude(gx, gy, l2);
      S[(size_t)y * W + x] = (uint8_t)canny_sector(gx, gy);
    }
  Image out(W, H, 1);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int s = S[(size_t)y * W + x], dx = canny_dx(s), dy = canny_dy(s);
      const uint32_t* m = M.data() + (size_t)(y + 1) * We + x + 1;
      const uint32_t before = *(m - (ptrdiff_t)dy * (ptrdiff_t)We - dx), after = *(m + (ptrdiff_t)dy * (ptrdiff_t)We + dx);
      out.data[(size_t)y * W + x] = canny_class(*m, before, after, s, lo, hi);
    }
  return out;
}

Image golden_hysteresis(const Image& cls, int conn) {
  check_canny_frame(cls.W, cls.H, cls.C);
  STRIPE_CHECK(conn == 4 || conn == 8, "canny: connectivity must be 4 or 8, got " << conn);
  const int W = cls.W, H = cls.H;
  Image out(W, H, 1);  // zeros; 255 doubles as "visited"
  const uint8_t* c = cls.data.data();
  static const int dx[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, dy[8] = {0, 0, -1, 1, -1, -1, 1, 1};
  std::vector<int64_t> stack;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int64_t p = (int64_t)y * W + x;
      if (c[p] < 2 || out.data[(size_t)p] != 0) continue;
      out.data[(size_t)p] = 255;
      stack.push_back(p);
      while (!stack.empty()) {
        const int64_t q = stack.back();
        stack.pop_back();
        const int qy = (int)(q / W), qx = (int)(q - (int64_t)qy * W);
        for (int k = 0; k < conn; ++k) {
          const int nx = qx + dx[k], ny = qy + dy[k];
          if (nx < 0 || ny < 0 || nx >= W || ny >= H) continue;
          const int64_t r = (int64_t)ny * W + nx;
          if (c[r] == 0 || out.data[(size_t)r] != 0) continue;
          out.data[(size_t)r] = 255;
          stack.push_back(r);
        }
      }
    }
  return out;
}

Image golden_canny(const Image& img, int low, int high, CannyNorm norm, Border border) {
  return golden_hysteresis(golden_canny_classes(img, low, high, norm, border), 8);
}

Image golden_hysteresis_threshold(const Image& img, int low, int high, int conn) {
  check_hysteresis(img.W, img.H, img.C, low, high, conn);
  Image cls(img.W, img.H, 1);
  for (size_t p = 0; p < cls.data.size(); ++p) cls.data[p] = hysteresis_class(img.data[p], (uint32_t)low, (uint32_t)high);
  return golden_hysteresis(cls, conn);
}

}  // namespace stripe
