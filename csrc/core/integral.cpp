// Integral images: checks, the golden integral and the golden window loop (the
// rule: stripe/integral.h).
#include "stripe/integral.h"

#include <cmath>

namespace stripe {

WindowOp parse_window_op(const std::string& token) {
  if (token == "box") return WindowOp::Box;
  if (token == "std") return WindowOp::Std;
  if (token == "mean") return WindowOp::Mean;
  if (token == "niblack") return WindowOp::Niblack;
  if (token == "sauvola") return WindowOp::Sauvola;
  fail("integral: the window operation must be box, std, mean, niblack or sauvola, got '" + token + "'");
}

const char* window_op_name(WindowOp op) {
  switch (op) {
    case WindowOp::Box: return "box";
    case WindowOp::Std: return "std";
    case WindowOp::Mean: return "mean";
    case WindowOp::Niblack: return "niblack";
    case WindowOp::Sauvola: return "sauvola";
  }
  return "?";
}

int window_kq(double k) {
  STRIPE_CHECK(std::isfinite(k) && std::fabs(k) <= (double)kWindowMaxAbsK,
               "integral: k must be finite with |k| <= " << kWindowMaxAbsK << ", got " << k);
  return (int)std::nearbyint(4096.0 * k);
}

void check_integral(int W, int H, int C) {
  STRIPE_CHECK(C == 1, "integral: needs a 1-channel image, got C = " << C << "; convert first (gray, threshold, ...)");
  STRIPE_CHECK(W >= 1 && H >= 1, "integral: empty image (" << W << "x" << H << ")");
  STRIPE_CHECK(W <= kIntegralMaxSide && H <= kIntegralMaxSide,
               "integral: " << W << "x" << H << " has a side above " << kIntegralMaxSide);
}

void check_window(int op, int K, Border border, int C, int64_t kq) {
  STRIPE_CHECK(op >= 0 && op < kWindowOps, "integral: unknown window operation " << op);
  const WindowOp o = (WindowOp)op;
  STRIPE_CHECK(K >= 1 && K % 2 == 1, "integral: the window must be odd and at least 1, got " << K);
  const int kmax = window_uses_squares(o) ? kWindowMaxKSquares : kWindowMaxK;
  STRIPE_CHECK(K <= kmax, "integral: window " << K << " is above " << kmax << ", the limit of " << window_op_name(o));
  STRIPE_CHECK(border == Border::Reflect101 || border == Border::Replicate || border == Border::Constant,
               "integral: the border must be reflect101, replicate or constant (skip has no window sums)");
  STRIPE_CHECK(C >= -kWindowMaxAbsC && C <= kWindowMaxAbsC,
               "integral: c must lie in -" << kWindowMaxAbsC << ".." << kWindowMaxAbsC << ", got " << C);
  STRIPE_CHECK(o == WindowOp::Mean || o == WindowOp::Niblack || C == 0,
               "integral: " << window_op_name(o) << " takes no c, got " << C);
  STRIPE_CHECK(kq >= -4096 * kWindowMaxAbsK && kq <= 4096 * kWindowMaxAbsK,
               "integral: k must be finite with |k| <= " << kWindowMaxAbsK << ", got kq = " << kq);
  STRIPE_CHECK(o == WindowOp::Niblack || o == WindowOp::Sauvola || kq == 0,
               "integral: " << window_op_name(o) << " takes no k, got kq = " << kq);
}

void golden_integral(const Image& img, bool squared, std::vector<int32_t>* out) {
  check_integral(img.W, img.H, img.C);
  const int W = img.W, H = img.H;
  const size_t tp = (size_t)W + 1;
  out->assign(tp * ((size_t)H + 1), 0);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const uint32_t p = img.data[(size_t)y * W + x], v = squared ? p * p : p;
      const uint32_t up = (uint32_t)(*out)[(size_t)y * tp + x + 1], left = (uint32_t)(*out)[(size_t)(y + 1) * tp + x],
                     diag = (uint32_t)(*out)[(size_t)y * tp + x];
      (*out)[(size_t)(y + 1) * tp + x + 1] = (int32_t)(v + up + left - diag);  // wraps modulo 2^32
    }
}

Image golden_window(const Image& img, const WindowSpec& spec, Border border) {
  check_integral(img.W, img.H, img.C);
  check_window((int)spec.op, spec.K, border, spec.C, spec.kq);
  const int W = img.W, H = img.H, K = spec.K, R = K / 2;
  const int We = W + 2 * R, He = H + 2 * R;
  // the extended frame, written out
  std::vector<uint8_t> P((size_t)We * He);
  for (int y = 0; y < He; ++y) {
    const int sy = border_index(y - R, H, border);
    for (int x = 0; x < We; ++x) {
      const int sx = border_index(x - R, W, border);
      P[(size_t)y * We + x] = sy < 0 || sx < 0 ? 0 : img.data[(size_t)sy * W + sx];
    }
  }
  // per extended row and output column the K-wide sums, then per pixel K of them
  std::vector<uint64_t> ha((size_t)W * He), hb((size_t)W * He);
  for (int y = 0; y < He; ++y)
    for (int x = 0; x < W; ++x) {
      uint64_t a = 0, b = 0;
      for (int i = 0; i < K; ++i) {
        const uint64_t p = P[(size_t)y * We + x + i];
        a += p, b += p * p;
      }
      ha[(size_t)y * W + x] = a, hb[(size_t)y * W + x] = b;
    }
  Image out(W, H, 1);
  const uint32_t N = (uint32_t)K * (uint32_t)K;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      uint64_t a = 0, b = 0;
      for (int j = 0; j < K; ++j) a += ha[(size_t)(y + j) * W + x], b += hb[(size_t)(y + j) * W + x];
      // b stays below 2^32 only within the squares limit; box and mean do not read it
      out.data[(size_t)y * W + x] =
          window_rule((int)spec.op, img.data[(size_t)y * W + x], (uint32_t)a, (uint32_t)b, N, spec.C, spec.kq);
    }
  return out;
}

}  // namespace stripe
