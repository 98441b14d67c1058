// Resize rule (see resize.h): the tap tables, the spec parser and the golden loop.
// Integer arithmetic only: no double and no exp.
#include "stripe/resize.h"

#include <algorithm>
#include <numeric>

namespace stripe {

const char* resize_mode_name(ResizeMode m) {
  switch (m) {
    case ResizeMode::Auto: return "auto";
    case ResizeMode::Nearest: return "nearest";
    case ResizeMode::Bilinear: return "bilinear";
    case ResizeMode::Area: return "area";
  }
  return "?";
}

ResizeMode parse_resize_mode(const std::string& s) {
  if (s == "auto") return ResizeMode::Auto;
  if (s == "nearest") return ResizeMode::Nearest;
  if (s == "bilinear" || s == "linear") return ResizeMode::Bilinear;
  if (s == "area") return ResizeMode::Area;
  fail("resize: unknown mode '" + s + "' (auto | nearest | bilinear | area)");
}

namespace {
// all of s as a decimal size in [1, kResizeMaxSize]; 0 otherwise
int parse_size(const std::string& s) {
  if (s.empty() || s.size() > 5) return 0;
  int v = 0;
  for (char c : s) {
    if (c < '0' || c > '9') return 0;
    v = v * 10 + (c - '0');
  }
  return v <= kResizeMaxSize ? v : 0;
}
}  // namespace

ResizeSpec parse_resize_spec(const std::string& token) {
  const std::string what = "resize spec '" + token + "': ";
  const size_t colon = token.find(':');
  const std::string size = token.substr(0, colon);
  const size_t x = size.find('x');
  STRIPE_CHECK(x != std::string::npos, what << "expected WxH[:mode]");
  ResizeSpec r;
  r.W = parse_size(size.substr(0, x));
  r.H = parse_size(size.substr(x + 1));
  STRIPE_CHECK(r.W >= 1 && r.H >= 1, what << "W and H must be integers in 1.." << kResizeMaxSize);
  if (colon != std::string::npos) {
    try {
      r.mode = parse_resize_mode(token.substr(colon + 1));
    } catch (const Error& e) {
      fail(what + e.what());
    }
  }
  return r;
}

ResizeTaps resize_taps(int n_in, int n_out, ResizeMode mode) {
  STRIPE_CHECK(n_in >= 1 && n_in <= kResizeMaxSize, "resize: n_in " << n_in << " outside 1.." << kResizeMaxSize);
  STRIPE_CHECK(n_out >= 1 && n_out <= kResizeMaxSize, "resize: n_out " << n_out << " outside 1.." << kResizeMaxSize);
  if (mode == ResizeMode::Auto)
    mode = n_out < n_in ? ResizeMode::Area : n_out > n_in ? ResizeMode::Bilinear : ResizeMode::Nearest;
  ResizeTaps t;
  t.n_in = n_in;
  t.n_out = n_out;
  t.first.resize((size_t)n_out);
  t.offset.assign((size_t)n_out + 1, 0);
  const int64_t ni = n_in, no = n_out;
  auto one_tap = [&](int o, int64_t i) {
    t.first[(size_t)o] = (int32_t)i;
    t.w.push_back((uint16_t)kResizeOne);
  };
  if (mode == ResizeMode::Nearest) {
    for (int o = 0; o < n_out; ++o) {
      one_tap(o, (2 * (int64_t)o + 1) * ni / (2 * no));
      t.offset[(size_t)o + 1] = (int32_t)t.w.size();
    }
  } else if (mode == ResizeMode::Bilinear) {
    const int64_t den = 2 * no;
    for (int o = 0; o < n_out; ++o) {
      const int64_t num = (2 * (int64_t)o + 1) * ni - no;
      const int64_t i0 = num >= 0 ? num / den : -((-num + den - 1) / den);
      const int64_t r = num - i0 * den;
      const int64_t w1 = (65536 * r + den) / (2 * den);
      const int64_t a = std::min(std::max<int64_t>(i0, 0), ni - 1), b = std::min(std::max<int64_t>(i0 + 1, 0), ni - 1);
      if (a == b) {
        one_tap(o, a);
      } else {
        t.first[(size_t)o] = (int32_t)a;
        t.w.push_back((uint16_t)(kResizeOne - w1));
        t.w.push_back((uint16_t)w1);
      }
      t.offset[(size_t)o + 1] = (int32_t)t.w.size();
    }
  } else {
    STRIPE_CHECK(n_out <= n_in, "resize: mode area cannot grow an axis (n_in " << n_in << " -> n_out " << n_out
                                                                                << "); use bilinear or auto");
    STRIPE_CHECK(ni <= (int64_t)kResizeMaxFactor * no,
                 "resize: area factor n_in / n_out = " << n_in << " / " << n_out << " exceeds the limit of "
                                                       << kResizeMaxFactor << "; resize in two steps");
    std::vector<int64_t> rem;
    std::vector<int> order;
    for (int o = 0; o < n_out; ++o) {
      // in units of 1 / n_out: cell o is [o n_in, (o + 1) n_in), pixel i is [i n_out, (i + 1) n_out)
      const int64_t c0 = (int64_t)o * ni, c1 = c0 + ni;
      const int64_t i_lo = c0 / no, i_hi = (c1 - 1) / no;
      const int n = (int)(i_hi - i_lo + 1);
      t.first[(size_t)o] = (int32_t)i_lo;
      rem.resize((size_t)n);
      order.resize((size_t)n);
      int64_t sum = 0;
      const size_t base = t.w.size();
      for (int k = 0; k < n; ++k) {
        const int64_t i = i_lo + k;
        const int64_t L = std::min(c1, (i + 1) * no) - std::max(c0, i * no);
        const int64_t q = (int64_t)kResizeOne * L;
        t.w.push_back((uint16_t)(q / ni));
        rem[(size_t)k] = q % ni;
        sum += q / ni;
      }
      // the missing units, one each, to the largest remainders (ties to the lower index)
      std::iota(order.begin(), order.end(), 0);
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rem[(size_t)a] > rem[(size_t)b]; });
      const int64_t miss = kResizeOne - sum;
      STRIPE_CHECK(miss >= 0 && miss <= n, "resize: area weights of output " << o << " do not close");
      for (int k = 0; k < (int)miss; ++k) ++t.w[base + (size_t)order[(size_t)k]];
      t.offset[(size_t)o + 1] = (int32_t)t.w.size();
    }
  }
  for (int o = 0; o < n_out; ++o) {
    const int c = t.count(o);
    t.max_count = std::max(t.max_count, c);
    STRIPE_CHECK(c >= 1 && t.first[(size_t)o] >= 0 && t.first[(size_t)o] + c <= n_in, "resize: taps outside the axis");
    STRIPE_CHECK(o == 0 || (t.first[(size_t)o] >= t.first[(size_t)o - 1] &&
                            t.first[(size_t)o] + c >= t.first[(size_t)o - 1] + t.count(o - 1)),
                 "resize: taps not monotone");
  }
  return t;
}

Image golden_resize(const Image& in, int W2, int H2, ResizeMode mode) {
  STRIPE_CHECK(in.C == 1 || in.C == 3, "resize: image must have 1 or 3 channels, got C = " << in.C);
  STRIPE_CHECK(in.W >= 1 && in.H >= 1, "resize: empty image");
  const ResizeTaps tx = resize_taps(in.W, W2, mode), ty = resize_taps(in.H, H2, mode);
  const int C = in.C;
  Image out(W2, H2, C, NoInit{});
  for (int oy = 0; oy < H2; ++oy) {
    for (int ox = 0; ox < W2; ++ox) {
      for (int c = 0; c < C; ++c) {
        uint32_t acc = 0;
        for (int v = 0; v < ty.count(oy); ++v) {
          const uint8_t* row = in.row(ty.first[(size_t)oy] + v);
          uint32_t h = 0;
          for (int u = 0; u < tx.count(ox); ++u)
            h += (uint32_t)tx.w[(size_t)tx.offset[(size_t)ox] + u] * row[(size_t)(tx.first[(size_t)ox] + u) * C + c];
          h = (h + 64) >> 7;
          acc += (uint32_t)ty.w[(size_t)ty.offset[(size_t)oy] + v] * h;
        }
        out.row(oy)[(size_t)ox * C + c] = (uint8_t)((acc + (1u << 22)) >> 23);
      }
    }
  }
  return out;
}

}  // namespace stripe
