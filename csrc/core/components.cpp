// Connected components: checks, the golden flood fill, the statistics table and
// the area filter (the rule: stripe/components.h).
#include "stripe/components.h"

#include <algorithm>
#include <cstring>

#include "stripe/common.h"

namespace stripe {

int parse_connectivity(const std::string& token) {
  if (token == "4") return 4;
  if (token == "8") return 8;
  fail("components: connectivity must be 4 or 8, got '" + token + "'");
}

void check_components(int W, int H, int C, int conn) {
  STRIPE_CHECK(C == 1, "components: needs a 1-channel image, got C = " << C
                           << "; convert first (gray, threshold, ...)");
  STRIPE_CHECK(W >= 1 && H >= 1, "components: empty image (" << W << "x" << H << ")");
  STRIPE_CHECK((int64_t)W * H <= kComponentsMaxPixels,
               "components: " << W << "x" << H << " pixels exceed 2^31 - 2");
  STRIPE_CHECK(conn == 4 || conn == 8, "components: connectivity must be 4 or 8, got " << conn);
}

void check_area_bounds(int64_t amin, int64_t amax) {
  STRIPE_CHECK(amin >= 1, "components: min_area must be at least 1, got " << amin);
  STRIPE_CHECK(amax >= amin, "components: max_area " << amax << " < min_area " << amin);
}

int golden_components(const Image& img, int conn, std::vector<int32_t>* labels) {
  check_components(img.W, img.H, img.C, conn);
  const int W = img.W, H = img.H;
  labels->assign((size_t)W * H, 0);
  int32_t* L = labels->data();
  const uint8_t* s = img.data.data();
  static const int dx[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, dy[8] = {0, 0, -1, 1, -1, -1, 1, 1};
  std::vector<int64_t> stack;
  int n = 0;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int64_t p = (int64_t)y * W + x;
      if (s[p] == 0 || L[p] != 0) continue;
      L[p] = ++n;
      stack.push_back(p);
      while (!stack.empty()) {
        const int64_t q = stack.back();
        stack.pop_back();
        const int qy = (int)(q / W), qx = (int)(q - (int64_t)qy * W);
        for (int k = 0; k < conn; ++k) {
          const int nx = qx + dx[k], ny = qy + dy[k];
          if (nx < 0 || ny < 0 || nx >= W || ny >= H) continue;
          const int64_t r = (int64_t)ny * W + nx;
          if (s[r] == 0 || L[r] != 0) continue;
          L[r] = n;
          stack.push_back(r);
        }
      }
    }
  return n;
}

std::vector<int64_t> component_stats(const int32_t* labels, int64_t lp, int W, int H, int N) {
  STRIPE_CHECK(labels && W >= 1 && H >= 1 && lp >= W && N >= 0, "components: bad label plane");
  std::vector<int64_t> t((size_t)(N + 1) * kStatCols, 0);
  for (int l = 0; l <= N; ++l) t[(size_t)l * kStatCols + 1] = t[(size_t)l * kStatCols + 2] = INT64_MAX;
  for (int y = 0; y < H; ++y) {
    const int32_t* r = labels + (int64_t)y * lp;
    for (int x = 0; x < W; ++x) {
      const int32_t l = r[x];
      STRIPE_CHECK(l >= 0 && l <= N, "components: label " << l << " outside 0.." << N);
      int64_t* e = t.data() + (size_t)l * kStatCols;
      e[0] += 1;
      e[1] = std::min<int64_t>(e[1], x), e[2] = std::min<int64_t>(e[2], y);
      e[3] = std::max<int64_t>(e[3], x + 1), e[4] = std::max<int64_t>(e[4], y + 1);
      e[5] += x, e[6] += y;
    }
  }
  for (int l = 0; l <= N; ++l) {
    int64_t* e = t.data() + (size_t)l * kStatCols;
    if (e[0] == 0) e[1] = e[2] = 0;
  }
  return t;
}

Image golden_area_filter(const Image& img, int conn, int64_t amin, int64_t amax) {
  check_components(img.W, img.H, img.C, conn);
  check_area_bounds(amin, amax);
  std::vector<int32_t> labels;
  const int N = golden_components(img, conn, &labels);
  const std::vector<int64_t> t = component_stats(labels.data(), img.W, img.W, img.H, N);
  Image out(img.W, img.H, 1);
  for (size_t p = 0; p < labels.size(); ++p) {
    const int64_t a = t[(size_t)labels[p] * kStatCols];
    out.data[p] = labels[p] != 0 && a >= amin && a <= amax ? img.data[p] : 0;
  }
  return out;
}

}  // namespace stripe
