// Fast host executor (see cpu_exec.h).  Every formula mirrors golden_pass
// (golden.cpp) term for term; only the loop structure differs.
#include "stripe/cpu_exec.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>

#include "stripe/canny.h"
#include "stripe/components.h"
#include "stripe/distance.h"
#include "stripe/integral.h"
#include "stripe/orient.h"
#include "stripe/rank_net.h"
#include "stripe/remap.h"
#include "stripe/resize.h"
#include "stripe/warp.h"

namespace stripe {

int cpu_threads(int ranks_per_host) {
  if (const char* e = std::getenv("STRIPE_CPU_THREADS")) return std::max(1, std::atoi(e));
  const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
  return std::max(1, std::min(64, hw / std::max(1, ranks_per_host)));
}

namespace {

inline uint8_t sat(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// round(sqrt(n)) for n >= 0, exactly (as golden.cpp)
inline int isqrt_round(int n) {
  int k = (int)std::sqrt((double)n);
  while (k * k > n) --k;
  while ((k + 1) * (k + 1) <= n) ++k;
  return n > k * k + k ? k + 1 : k;
}

// Hot loops, each cloned for AVX2 and a baseline x86-64 target (the loader
// picks the AVX2 clone where the CPU has it; this file is host-only C++).
#define STRIPE_SIMD __attribute__((target_clones("avx2", "default")))

// Colour matrix sweep over n RGB pixels: golden apply_prog's formula
// (color_matrix_channel) in i32, q = 9 coefficients then 3 offsets.
STRIPE_SIMD void cmat_sweep(const uint8_t* __restrict s, uint8_t* __restrict o, const int32_t* __restrict q, int n) {
  const int32_t h = 1 << (kColorShift - 1);
  for (int x = 0; x < n; ++x) {
    const int32_t r = s[3 * x], g = s[3 * x + 1], b = s[3 * x + 2];
    for (int c = 0; c < 3; ++c) {
      const int32_t v = (q[3 * c] * r + q[3 * c + 1] * g + q[3 * c + 2] * b + q[9 + c] + h) >> kColorShift;
      o[3 * x + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
  }
}

// The pointwise program as byte tables: per pixel out = post((gray | cmat)(pre(px))).
struct ProgTables {
  int cin = 3, cmid = 3;
  bool gray = false, ref = false, copy = false;
  bool cmat = false, cm_pre = false, cm_post = false;
  int32_t cm[12];
  uint8_t pre[256], lut[256];         // lut: post(pre(v)) (no gray) or post(v) (gray)
  uint8_t tr[256], tg[256], tb[256];  // gray:ref: the per-channel truncated terms of pre(v)

  ProgTables(const PointwiseProgram& pr, int cin_) : cin(cin_) {
    gray = pr.gray;
    cmid = gray ? 1 : cin;
    ref = pr.gmode == GrayMode::Ref;
    cmat = pr.cmat;
    cm_pre = cmat && pr.has_pre;
    cm_post = cmat && pr.has_post;
    for (int i = 0; i < 12; ++i) cm[i] = pr.cm[(size_t)i];
    copy = !gray && !cmat;
    for (int v = 0; v < 256; ++v) {
      pre[v] = pr.has_pre ? pr.pre[v] : (uint8_t)v;
      if (cmat) {
        lut[v] = pr.has_post ? pr.post[v] : (uint8_t)v;
      } else if (!gray) {
        lut[v] = pr.has_post ? pr.post[pre[v]] : pre[v];
        copy = copy && lut[v] == v;
      } else {
        lut[v] = pr.has_post ? pr.post[v] : (uint8_t)v;
        // gray_pixel(Ref, r, g, b) = trunc terms summed (<= 254): separable per channel
        tr[v] = gray_pixel(GrayMode::Ref, pre[v], 0, 0);
        tg[v] = gray_pixel(GrayMode::Ref, 0, pre[v], 0);
        tb[v] = gray_pixel(GrayMode::Ref, 0, 0, pre[v]);
      }
    }
  }

  // n pixels of cin bytes -> n pixels of cmid bytes
  void row(const uint8_t* src, int n, uint8_t* dst) const {
    if (cmat) {
      uint8_t t[3 * 256];  // pre-LUT pixels of one block
      for (int x0 = 0; x0 < n; x0 += 256) {
        const int m = std::min(256, n - x0);
        const uint8_t* s = src + (size_t)3 * x0;
        uint8_t* d = dst + (size_t)3 * x0;
        if (cm_pre) {
          for (int i = 0; i < 3 * m; ++i) t[i] = pre[s[i]];
          s = t;
        }
        cmat_sweep(s, d, cm, m);
        if (cm_post)
          for (int i = 0; i < 3 * m; ++i) d[i] = lut[d[i]];
      }
    } else if (!gray) {
      const int nb = n * cin;
      if (copy) {
        std::memcpy(dst, src, (size_t)nb);
      } else {
        for (int i = 0; i < nb; ++i) dst[i] = lut[src[i]];
      }
    } else if (ref) {
      for (int x = 0; x < n; ++x) dst[x] = lut[tr[src[3 * x]] + tg[src[3 * x + 1]] + tb[src[3 * x + 2]]];
    } else {
      for (int x = 0; x < n; ++x) {
        const int r = pre[src[3 * x]], g = pre[src[3 * x + 1]], b = pre[src[3 * x + 2]];
        dst[x] = lut[(r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14];
      }
    }
  }
};

// Run f(ya, yb) over [y0, y1) split into up to `threads` contiguous blocks
// (at least ~256 KiB of output each: thread start-up costs tens of us).
template <class F>
void parallel_rows(int y0, int y1, int64_t row_bytes, int threads, F&& f) {
  const int n = y1 - y0;
  if (n <= 0) return;
  const int64_t work = (int64_t)n * std::max<int64_t>(1, row_bytes);
  int T = (int)std::min<int64_t>({(int64_t)threads, (int64_t)n, std::max<int64_t>(1, work >> 18)});
  T = std::max(1, T);
  if (T == 1) {
    f(y0, y1);
    return;
  }
  // a worker's exception (or a thread that fails to start) must surface in
  // the caller as a C++ exception, not std::terminate: the first error is
  // kept and rethrown after every started worker has joined
  std::vector<std::exception_ptr> err((size_t)T);
  auto guarded = [&f, &err](int t, int ya, int yb) {
    try {
      f(ya, yb);
    } catch (...) {
      err[(size_t)t] = std::current_exception();
    }
  };
  std::vector<std::thread> th;
  th.reserve((size_t)T - 1);
  try {
    for (int t = 1; t < T; ++t)
      th.emplace_back(guarded, t, y0 + (int)((int64_t)n * t / T), y0 + (int)((int64_t)n * (t + 1) / T));
  } catch (...) {
    err[0] = std::current_exception();  // thread creation failed: the started workers still join
  }
  if (!err[0]) guarded(0, y0, y0 + (int)((int64_t)n / T));
  for (auto& t : th) t.join();
  for (auto& e : err)
    if (e) std::rethrow_exception(e);
}

// Prologued local row y with R border pixels each side ((W + 2R) * cmid bytes),
// all zeros for a constant-border row outside the image (golden build_cache).
void ext_row(const Pass& p, const ProgTables& pt, ConstView in, int W, RowGeom g, int y, uint8_t* dst) {
  const int R = p.R, C = p.cmid;
  const Border b = p.border;
  int gy = g.row0 + y;
  if (gy < 0 || gy >= g.Hg) {
    const int m = border_index(gy, g.Hg, b);
    if (m < 0) {
      std::memset(dst, 0, (size_t)(W + 2 * R) * C);
      return;
    }
    gy = m;
  }
  pt.row(in.origin + (int64_t)(gy - g.row0) * in.pitch, W, dst + (size_t)R * C);
  // the program is per pixel: the border pixel at x is the prologued pixel border_index(x)
  for (int k = 1; k <= R; ++k) {
    for (int side = 0; side < 2; ++side) {
      const int x = side ? W - 1 + k : -k;
      const int m = border_index(x, W, b);
      uint8_t* d = dst + (size_t)(x + R) * C;
      if (m < 0) std::memset(d, 0, (size_t)C);
      else std::memcpy(d, dst + (size_t)(m + R) * C, (size_t)C);
    }
  }
}

STRIPE_SIMD void tap_u8(int32_t* __restrict a, const uint8_t* __restrict s, int w, int n) {
  for (int i = 0; i < n; ++i) a[i] += w * (int32_t)s[i];
}
// unsigned 16-bit sums: the caller guarantees no wrap (non-negative taps, sum * 255 < 2^16)
STRIPE_SIMD void tap_u8_u16(uint16_t* __restrict a, const uint8_t* __restrict s, int w, int n) {
  for (int i = 0; i < n; ++i) a[i] = (uint16_t)(a[i] + (uint16_t)w * (uint16_t)s[i]);
}
STRIPE_SIMD void tap_u16(int32_t* __restrict a, const uint16_t* __restrict s, int w, int n) {
  for (int i = 0; i < n; ++i) a[i] += w * (int32_t)s[i];
}
STRIPE_SIMD void finish_shift(const int32_t* __restrict a, uint8_t* __restrict o, int h, int sh, int n) {
  for (int i = 0; i < n; ++i) {
    const int v = (a[i] + h) >> sh;  // sums >= 0: floor division by 2^sh
    o[i] = (uint8_t)(v > 255 ? 255 : v);
  }
}
STRIPE_SIMD void finish_sat(const int32_t* __restrict a, uint8_t* __restrict o, int n) {
  for (int i = 0; i < n; ++i) o[i] = (uint8_t)(a[i] < 0 ? 0 : (a[i] > 255 ? 255 : a[i]));
}
STRIPE_SIMD void finish_sobel(const int32_t* __restrict a, const int32_t* __restrict b, uint8_t* __restrict o, int n) {
  for (int i = 0; i < n; ++i) {
    const int v = (a[i] < 0 ? -a[i] : a[i]) + (b[i] < 0 ? -b[i] : b[i]);
    o[i] = (uint8_t)(v > 255 ? 255 : v);
  }
}

// Rank filters: byte-wise min / max sweeps over whole extended rows.
STRIPE_SIMD void min_into(uint8_t* __restrict d, const uint8_t* __restrict s, int n) {
  for (int i = 0; i < n; ++i) d[i] = s[i] < d[i] ? s[i] : d[i];
}
STRIPE_SIMD void max_into(uint8_t* __restrict d, const uint8_t* __restrict s, int n) {
  for (int i = 0; i < n; ++i) d[i] = s[i] > d[i] ? s[i] : d[i];
}
// compare-exchange: (a, b) <- (min, max), element by element
STRIPE_SIMD void cex_u8(uint8_t* __restrict a, uint8_t* __restrict b, int n) {
  for (int i = 0; i < n; ++i) {
    const uint8_t lo = a[i] < b[i] ? a[i] : b[i], hi = a[i] < b[i] ? b[i] : a[i];
    a[i] = lo;
    b[i] = hi;
  }
}

// One output row (E bytes) of a rank filter from the K extended ring rows
// (EW bytes each, any order: the window's order statistics do not depend on it).
// erode / dilate: vertical min / max of the rows, then horizontal min / max of
// the K shifted views.  median: the columns of K are sorted by a network of
// row-wide compare-exchanges (ranknet::ColSort), then ranknet::Select runs
// over the K*K views (sorted column dx, element r) = sorted row r shifted by
// dx pixels.  `work` holds K*EW + K*K*E bytes.
template <int K>
void rank_row(Rank rank, const uint8_t* const* rows, int C, int E, int EW, uint8_t* work, uint8_t* o) {
  if (rank != Rank::Median) {
    uint8_t* v = work;
    std::memcpy(v, rows[0], (size_t)EW);
    for (int dy = 1; dy < K; ++dy) (rank == Rank::Min ? min_into : max_into)(v, rows[dy], EW);
    std::memcpy(o, v, (size_t)E);
    for (int dx = 1; dx < K; ++dx) (rank == Rank::Min ? min_into : max_into)(o, v + (size_t)dx * C, E);
    return;
  }
  uint8_t* col[K];
  for (int r = 0; r < K; ++r) {
    col[r] = work + (size_t)r * EW;
    std::memcpy(col[r], rows[r], (size_t)EW);
  }
  using CS = ranknet::ColSort<K>;
  for (int k = 0; k < CS::N; ++k) cex_u8(col[CS::at(k).i], col[CS::at(k).j], EW);
  uint8_t* wire[K * K];
  for (int dx = 0; dx < K; ++dx)
    for (int r = 0; r < K; ++r) {
      wire[dx * K + r] = work + (size_t)K * EW + (size_t)(dx * K + r) * E;
      std::memcpy(wire[dx * K + r], col[r] + (size_t)dx * C, (size_t)E);
    }
  using SN = ranknet::Select<K>;
  for (int k = 0; k < SN::N; ++k) {
    const ranknet::Step s = SN::at(k);
    if (s.mode == ranknet::kBoth) cex_u8(wire[s.i], wire[s.j], E);
    else if (s.mode == ranknet::kMin) min_into(wire[s.i], wire[s.j], E);
    else max_into(wire[s.j], wire[s.i], E);
  }
  std::memcpy(o, wire[SN::kOut], (size_t)E);
}

// One output row (E bytes) of a bilateral filter (filters.h) from the K extended
// ring rows in window order: per tap a table lookup and two integer
// accumulations, then the rounded quotient.  D and N hold E sums each.
void bilateral_row(const StencilInfo& si, const uint8_t* range, const uint8_t* const* rows, int K, int C, int E,
                   uint32_t* D, uint32_t* N, uint8_t* o) {
  const int R = K / 2;
  const uint8_t* cen = rows[R] + (size_t)R * C;
  std::fill(D, D + E, 0u);
  std::fill(N, N + E, 0u);
  for (int dy = 0; dy < K; ++dy)
    for (int dx = 0; dx < K; ++dx) {
      const uint8_t* s = rows[dy] + (size_t)dx * C;
      const uint32_t ws = (uint32_t)si.w[(size_t)dy * K + dx];
      for (int i = 0; i < E; ++i) {
        const int d = (int)s[i] - (int)cen[i];
        const uint32_t w = ws * range[d < 0 ? -d : d];
        D[i] += w;
        N[i] += w * s[i];
      }
    }
  for (int i = 0; i < E; ++i) o[i] = bilateral_finish(N[i], D[i]);
}

void stencil_rows(const Pass& p, const ProgTables& pt, ConstView in, MutView out, int W, RowGeom g, int ya, int yb) {
  const StencilInfo& si = stencil_info(p.sid);
  const int K = p.K, R = p.R, C = p.cmid;
  const int E = W * C, EW = (W + 2 * R) * C;
  const bool rank = si.rank != Rank::None;
  std::vector<uint32_t> bsum(si.bilateral ? (size_t)2 * E : 0);
  STRIPE_CHECK(!rank || K == 3 || K == 5, "rank filters come in sizes 3 and 5");
  std::vector<uint8_t> rwork(rank ? (size_t)K * EW + (size_t)K * K * E : 0);
  std::vector<int> wy;
  if (si.sobel) {
    wy.resize((size_t)K * K);
    for (int dy = 0; dy < K; ++dy)
      for (int dx = 0; dx < K; ++dx) wy[(size_t)dy * K + dx] = si.w[(size_t)dx * K + dy];
  }
  // rank-one windows (gaussian / box): s = sum_dy w1[dy] sum_dx w1[dx] p, the same
  // integer as the K x K sum, as a vertical pass into u16 sums (no wrap: taps >= 0,
  // sum(w1) * 255 < 2^16) and a horizontal pass over them
  bool sep = si.separable && !si.sobel && (int)si.w1.size() == K;
  int w1sum = 0;
  for (int i = 0; sep && i < K; ++i) {
    sep = si.w1[(size_t)i] >= 0;
    w1sum += si.w1[(size_t)i];
    for (int j = 0; sep && j < K; ++j) sep = si.w[(size_t)i * K + j] == si.w1[(size_t)i] * si.w1[(size_t)j];
  }
  sep = sep && w1sum * 255 < 65536;
  int sh = -1;  // div as a shift when it is a power of two
  for (int k = 0; k < 31; ++k)
    if (si.div == (1 << k)) sh = k;

  std::vector<uint8_t> ring((size_t)K * EW);
  std::vector<int32_t> acc(rank ? 0 : (size_t)E), acc2(si.sobel ? (size_t)E : 0);
  std::vector<uint16_t> vs(sep ? (size_t)EW : 0);
  std::vector<uint8_t> res((size_t)E);
  auto slot = [&](int y) { return ring.data() + (size_t)((y - (ya - R)) % K) * EW; };
  for (int y = ya - R; y < ya + R; ++y) ext_row(p, pt, in, W, g, y, slot(y));
  for (int y = ya; y < yb; ++y) {
    ext_row(p, pt, in, W, g, y + R, slot(y + R));
    uint8_t* o = res.data();
    if (rank) {
      const uint8_t* rows[5];
      for (int dy = 0; dy < K; ++dy) rows[dy] = slot(y + dy - R);
      if (K == 3) rank_row<3>(si.rank, rows, C, E, EW, rwork.data(), o);
      else rank_row<5>(si.rank, rows, C, E, EW, rwork.data(), o);
    } else if (si.bilateral) {
      const uint8_t* rows[5];
      STRIPE_CHECK(K <= 5, "bilateral filters come in sizes 3 and 5");
      for (int dy = 0; dy < K; ++dy) rows[dy] = slot(y + dy - R);
      bilateral_row(si, p.range.data(), rows, K, C, E, bsum.data(), bsum.data() + E, o);
    } else {
      std::fill(acc.begin(), acc.end(), 0);
      int32_t* a = acc.data();
      if (sep) {
        std::fill(vs.begin(), vs.end(), (uint16_t)0);
        for (int dy = 0; dy < K; ++dy) tap_u8_u16(vs.data(), slot(y + dy - R), si.w1[(size_t)dy], EW);
        for (int dx = 0; dx < K; ++dx) tap_u16(a, vs.data() + (size_t)dx * C, si.w1[(size_t)dx], E);
      } else {
        if (si.sobel) std::fill(acc2.begin(), acc2.end(), 0);
        for (int dy = 0; dy < K; ++dy) {
          const uint8_t* r = slot(y + dy - R);
          for (int dx = 0; dx < K; ++dx) {
            const uint8_t* s = r + (size_t)dx * C;
            const int w = si.w[(size_t)dy * K + dx];
            if (w != 0) tap_u8(a, s, w, E);
            if (si.sobel && wy[(size_t)dy * K + dx] != 0) tap_u8(acc2.data(), s, wy[(size_t)dy * K + dx], E);
          }
        }
      }
      const int32_t* a2 = acc2.data();
      if (si.sobel && si.l2) {
        for (int i = 0; i < E; ++i) o[i] = sat(isqrt_round(a[i] * a[i] + a2[i] * a2[i]));
      } else if (si.sobel) {
        finish_sobel(a, a2, o, E);
      } else if (si.div > 1 && sh >= 0) {
        finish_shift(a, o, si.div / 2, sh, E);
      } else if (si.div > 1) {
        const int d = si.div, h = si.div / 2;  // sums >= 0 for the smoothing filters
        for (int i = 0; i < E; ++i) o[i] = sat((a[i] + h) / d);
      } else {
        finish_sat(a, o, E);
      }
    }
    if (p.border == Border::Skip) {  // golden.cpp:133 (the reference's interior-only bounds)
      const int gy = g.row0 + y;
      const uint8_t* center = slot(y) + (size_t)R * C;
      if (gy <= R || gy >= g.Hg - R) {
        std::memcpy(o, center, (size_t)E);
      } else {
        for (int x = 0; x < W; ++x)
          if (x <= R || x >= W - R) std::memcpy(o + (size_t)x * C, center + (size_t)x * C, (size_t)C);
      }
    }
    if (p.has_epi)
      for (int i = 0; i < E; ++i) o[i] = p.epi[o[i]];
    uint8_t* dst = out.origin + (int64_t)y * out.pitch;
    if (p.epi_expand) {
      for (int x = 0; x < W; ++x) dst[3 * x] = dst[3 * x + 1] = dst[3 * x + 2] = o[x];
    } else {
      std::memcpy(dst, o, (size_t)E);
    }
  }
}

// Combine pass: a row-wide byte sweep per op, combine_rule's arithmetic term for term.
STRIPE_SIMD void combine_sweep(CombineKind k, const int* cq, int d, const uint8_t* __restrict x,
                               const uint8_t* __restrict h, uint8_t* __restrict o, int64_t n) {
  switch (k) {
    case CombineKind::Add:
      for (int64_t i = 0; i < n; ++i) {
        const int v = x[i] + h[i];
        o[i] = (uint8_t)(v > 255 ? 255 : v);
      }
      break;
    case CombineKind::Sub:
      for (int64_t i = 0; i < n; ++i) o[i] = (uint8_t)(h[i] > x[i] ? h[i] - x[i] : 0);
      break;
    case CombineKind::RSub:
      for (int64_t i = 0; i < n; ++i) o[i] = (uint8_t)(x[i] > h[i] ? x[i] - h[i] : 0);
      break;
    case CombineKind::AbsDiff:
      for (int64_t i = 0; i < n; ++i) o[i] = (uint8_t)(x[i] > h[i] ? x[i] - h[i] : h[i] - x[i]);
      break;
    case CombineKind::Min:
      for (int64_t i = 0; i < n; ++i) o[i] = x[i] < h[i] ? x[i] : h[i];
      break;
    case CombineKind::Max:
      for (int64_t i = 0; i < n; ++i) o[i] = x[i] > h[i] ? x[i] : h[i];
      break;
    case CombineKind::LinComb: {
      const int32_t qa = cq[0], qb = cq[1], q0 = cq[2] + (1 << (kColorShift - 1));
      for (int64_t i = 0; i < n; ++i) {
        const int32_t v = (qa * (int32_t)x[i] + qb * (int32_t)h[i] + q0) >> kColorShift;
        o[i] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
      }
      break;
    }
    case CombineKind::Above:
      for (int64_t i = 0; i < n; ++i) o[i] = (int)h[i] - (int)x[i] + d > 0 ? 255 : 0;
      break;
    default:
      break;
  }
}

void combine_rows(const Pass& p, ConstView in, ConstView in2, MutView out, int W, int ya, int yb) {
  const int64_t E = (int64_t)W * p.cin;
  for (int y = ya; y < yb; ++y) {
    uint8_t* dst = out.origin + (int64_t)y * out.pitch;
    combine_sweep(p.comb, p.cq, p.cd, in.origin + (int64_t)y * in.pitch, in2.origin + (int64_t)y * in2.pitch, dst, E);
    if (p.pro.has_post)
      for (int64_t i = 0; i < E; ++i) dst[i] = p.pro.post[dst[i]];
  }
}

void pointwise_rows(const Pass& p, const ProgTables& pt, ConstView in, MutView out, int W, int ya, int yb) {
  std::vector<uint8_t> tmp(p.pro.expand ? (size_t)W * pt.cmid : 0);
  for (int y = ya; y < yb; ++y) {
    const uint8_t* src = in.origin + (int64_t)y * in.pitch;
    uint8_t* dst = out.origin + (int64_t)y * out.pitch;
    if (!p.pro.expand) {
      pt.row(src, W, dst);
    } else {
      pt.row(src, W, tmp.data());  // expand follows a 1-channel program
      for (int x = 0; x < W; ++x) dst[3 * x] = dst[3 * x + 1] = dst[3 * x + 2] = tmp[(size_t)x];
    }
  }
}

}  // namespace

void cpu_pass(const Pass& p, ConstView in, MutView out, int W, RowGeom g, int y0, int y1, int threads,
              ConstView in2) {
  STRIPE_CHECK(!p.pro.has_stat, "statistic op not resolved (resolve_stat) before the pass runs");
  if (y1 <= y0) return;
  const int64_t row_bytes = (int64_t)W * p.cout;
  if (p.kind == PassKind::Combine) {
    STRIPE_CHECK(in2.origin != nullptr, "combine pass without a held image");
    parallel_rows(y0, y1, row_bytes, threads, [&](int ya, int yb) { combine_rows(p, in, in2, out, W, ya, yb); });
    return;
  }
  if (p.kind == PassKind::Conv) {  // float windows: the golden f64 sums themselves, row-parallel
    parallel_rows(y0, y1, row_bytes * p.K * p.K, threads,
                  [&](int ya, int yb) { golden_pass(p, in, out, W, g, ya, yb); });
    return;
  }
  STRIPE_CHECK(!p.pro.gray || p.cin == 3, "gray needs 3 channels");
  STRIPE_CHECK(!p.pro.expand || p.kind == PassKind::Pointwise, "expand inside a stencil prologue");
  const ProgTables pt(p.pro, p.cin);
  if (p.kind == PassKind::Pointwise) {
    parallel_rows(y0, y1, row_bytes, threads, [&](int ya, int yb) { pointwise_rows(p, pt, in, out, W, ya, yb); });
    return;
  }
  STRIPE_CHECK(pt.cmid == p.cmid, "prologue channels " << pt.cmid << " != stencil channels " << p.cmid);
  parallel_rows(y0, y1, row_bytes * p.K, threads,
                [&](int ya, int yb) { stencil_rows(p, pt, in, out, W, g, ya, yb); });
}

Histogram cpu_histogram(ConstView in, int W, int C, int rows, int threads) {
  STRIPE_CHECK(C == 1 || C == 3, "histogram needs 1 or 3 channels");
  Histogram h(C);
  std::mutex mu;
  parallel_rows(0, rows, (int64_t)W * C, threads, [&](int ya, int yb) {
    // a row block's private table (u32 per row: a row holds < 2^31 bytes)
    std::vector<uint64_t> t((size_t)256 * C, 0);
    uint32_t r[3][256];
    for (int y = ya; y < yb; ++y) {
      const uint8_t* s = in.origin + (int64_t)y * in.pitch;
      std::memset(r, 0, sizeof r);
      if (C == 1) {
        for (int x = 0; x < W; ++x) ++r[0][s[x]];
      } else {
        for (int x = 0; x < W; ++x) {
          ++r[0][s[3 * (size_t)x]];
          ++r[1][s[3 * (size_t)x + 1]];
          ++r[2][s[3 * (size_t)x + 2]];
        }
      }
      for (int c = 0; c < C; ++c)
        for (int v = 0; v < 256; ++v) t[(size_t)c * 256 + v] += r[c][v];
    }
    std::lock_guard<std::mutex> lk(mu);  // the blocks' tables summed at the end
    for (size_t i = 0; i < t.size(); ++i) h.bins[i] += t[i];
  });
  return h;
}

Histogram cpu_histogram(const Image& img, int threads) {
  return cpu_histogram(ConstView{img.data.data(), img.row_bytes()}, img.W, img.C, img.H, threads);
}

Image cpu_apply_plan(const Image& in, const Plan& plan, int threads, const Image* held_in) {
  STRIPE_CHECK(in.C == plan.cin, "image has " << in.C << " channels, chain expects " << plan.cin);
  STRIPE_CHECK((plan.held_c != 0) == (held_in != nullptr), "the chain was compiled " << (plan.held_c ? "for" : "without")
                                                               << " an external held image");
  STRIPE_CHECK(!held_in || (held_in->W == in.W && held_in->H == in.H && held_in->C == plan.held_c),
               "the held image must have the input's size and " << plan.held_c << " channel(s)");
  if (plan.passes.empty()) return in;
  if (plan.branched()) {
    // current and held images are shared, never copied: hold and swap move pointers
    std::shared_ptr<const Image> cur(&in, [](const Image*) {}), held;
    if (held_in) held = std::shared_ptr<const Image>(held_in, [](const Image*) {});
    for (const Pass& pp : plan.passes) {
      for (char a : pp.slots) {
        if (a == 'h') held = cur;
        else std::swap(cur, held);
      }
      const Pass resolved = pp.data_dependent() ? resolve_stat(pp, cpu_histogram(*cur, threads)) : Pass{};
      const Pass& p = pp.data_dependent() ? resolved : pp;
      auto nxt = std::make_shared<Image>(in.W, in.H, p.cout, NoInit{});
      const ConstView hv = held ? ConstView{held->data.data(), held->row_bytes()} : ConstView{};
      cpu_pass(p, ConstView{cur->data.data(), cur->row_bytes()}, MutView{nxt->data.data(), nxt->row_bytes()}, in.W,
               RowGeom{0, in.H}, 0, in.H, threads, hv);
      cur = nxt;
    }
    return *cur;
  }
  Image cur;  // the first pass reads the input in place (no copy of the frame)
  const Image* src = &in;
  for (const Pass& pp : plan.passes) {
    // a statistic op: the table of this pass's input, the whole intermediate image
    const Pass resolved = pp.data_dependent() ? resolve_stat(pp, cpu_histogram(*src, threads)) : Pass{};
    const Pass& p = pp.data_dependent() ? resolved : pp;
    Image nxt(in.W, in.H, p.cout, NoInit{});  // cpu_pass writes every row of [0, H)
    cpu_pass(p, ConstView{src->data.data(), src->row_bytes()}, MutView{nxt.data.data(), nxt.row_bytes()}, in.W,
             RowGeom{0, in.H}, 0, in.H, threads);
    cur = std::move(nxt);
    src = &cur;
  }
  return cur;
}

// ---- resize (stripe/resize.h) ----
namespace {
// h'(y, .) of one source row: E2 = W2 * C values in 8.8 fixed point
template <int C>
void resize_hrow(const ResizeTaps& tx, const uint8_t* row, uint16_t* h) {
  const int W2 = tx.n_out;
  if (tx.max_count == 1) {
    for (int ox = 0; ox < W2; ++ox) {
      const uint8_t* p = row + (size_t)tx.first[(size_t)ox] * C;
      for (int c = 0; c < C; ++c) h[(size_t)ox * C + c] = (uint16_t)(((uint32_t)kResizeOne * p[c] + 64) >> 7);
    }
    return;
  }
  for (int ox = 0; ox < W2; ++ox) {
    const uint16_t* w = tx.w.data() + tx.offset[(size_t)ox];
    const int n = tx.offset[(size_t)ox + 1] - tx.offset[(size_t)ox];
    const uint8_t* p = row + (size_t)tx.first[(size_t)ox] * C;
    uint32_t a[C] = {};
    for (int u = 0; u < n; ++u)
      for (int c = 0; c < C; ++c) a[c] += (uint32_t)w[u] * p[(size_t)u * C + c];
    for (int c = 0; c < C; ++c) h[(size_t)ox * C + c] = (uint16_t)((a[c] + 64) >> 7);
  }
}

STRIPE_SIMD void resize_vacc(uint32_t* acc, const uint16_t* h, uint32_t w, int n) {
  for (int i = 0; i < n; ++i) acc[i] += w * h[i];
}
STRIPE_SIMD void resize_vout(const uint32_t* acc, uint8_t* out, int n) {
  for (int i = 0; i < n; ++i) out[i] = (uint8_t)((acc[i] + (1u << 22)) >> 23);
}
}  // namespace

void cpu_resize(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch, int W2,
                int H2, ResizeMode mode, int threads) {
  STRIPE_CHECK(C == 1 || C == 3, "resize: image must have 1 or 3 channels, got C = " << C);
  STRIPE_CHECK(src && dst && W >= 1 && H >= 1, "resize: empty image");
  STRIPE_CHECK(src_pitch >= (int64_t)W * C && dst_pitch >= (int64_t)W2 * C, "resize: pitch smaller than a row");
  const ResizeTaps tx = resize_taps(W, W2, mode), ty = resize_taps(H, H2, mode);
  const int E2 = W2 * C;
  // a block's work is its source rows as much as its output rows
  const int64_t row_bytes = (int64_t)E2 + (int64_t)W * C * std::max(1, H / H2);
  parallel_rows(0, H2, row_bytes, std::max(1, threads), [&](int oa, int ob) {
    // ring of the h' rows one output row needs; every source row of the block
    // is reduced once, in order, when the first output row that reads it comes up
    const int R = ty.max_count;
    std::vector<uint16_t> ring((size_t)R * E2);
    std::vector<uint32_t> acc((size_t)E2);
    int next = ty.first[(size_t)oa];
    for (int oy = oa; oy < ob; ++oy) {
      const int f = ty.first[(size_t)oy], n = ty.count(oy);
      next = std::max(next, f);
      for (; next < f + n; ++next) {
        uint16_t* h = ring.data() + (size_t)(next % R) * E2;
        if (C == 1) resize_hrow<1>(tx, src + (int64_t)next * src_pitch, h);
        else resize_hrow<3>(tx, src + (int64_t)next * src_pitch, h);
      }
      std::fill(acc.begin(), acc.end(), 0u);
      for (int v = 0; v < n; ++v)
        resize_vacc(acc.data(), ring.data() + (size_t)((f + v) % R) * E2, ty.w[(size_t)ty.offset[(size_t)oy] + v], E2);
      resize_vout(acc.data(), dst + (int64_t)oy * dst_pitch, E2);
    }
  });
}

Image cpu_resize(const Image& in, int W2, int H2, ResizeMode mode, int threads) {
  STRIPE_CHECK(in.C == 1 || in.C == 3, "resize: image must have 1 or 3 channels, got C = " << in.C);
  STRIPE_CHECK(W2 >= 1 && W2 <= kResizeMaxSize && H2 >= 1 && H2 <= kResizeMaxSize,
               "resize: size " << W2 << "x" << H2 << " outside 1.." << kResizeMaxSize);
  Image out(W2, H2, in.C, NoInit{});
  cpu_resize(in.data.data(), in.row_bytes(), in.W, in.H, in.C, out.data.data(), out.row_bytes(), W2, H2, mode,
             threads);
  return out;
}

// ---- orientation and crop (stripe/orient.h) ----
namespace {
// one output row of a non-transposing op: a copy, or the row's pixels in reverse order
template <int C>
void orient_row(const uint8_t* __restrict s, uint8_t* __restrict d, int w, bool fx) {
  if (!fx) {
    std::memcpy(d, s, (size_t)w * C);
    return;
  }
  const uint8_t* p = s + (size_t)(w - 1) * C;
  for (int x = 0; x < w; ++x, p -= C, d += C)
    for (int c = 0; c < C; ++c) d[c] = p[c];
}

// output rows [ya, yb) of a transposing op, tile by tile: within a tile the
// source is read along its rows and the destination written down a column of
// at most kCpuOrientTile rows, both of which stay in the cache
template <int C>
void orient_transposed(const uint8_t* src, int64_t sp, int w, int h, uint8_t* dst, int64_t dp, bool fx, bool fy, int ya,
                       int yb) {
  constexpr int TS = kCpuOrientTile;
  for (int y0 = ya; y0 < yb; y0 += TS) {
    const int y1 = std::min(y0 + TS, yb);
    for (int x0 = 0; x0 < h; x0 += TS) {  // the output is h pixels wide
      const int x1 = std::min(x0 + TS, h);
      for (int x = x0; x < x1; ++x) {
        const uint8_t* srow = src + (int64_t)(fy ? h - 1 - x : x) * sp;
        uint8_t* d = dst + (int64_t)y0 * dp + (size_t)x * C;
        if (!fx) {
          const uint8_t* p = srow + (size_t)y0 * C;
          for (int y = y0; y < y1; ++y, p += C, d += dp)
            for (int c = 0; c < C; ++c) d[c] = p[c];
        } else {
          const uint8_t* p = srow + (size_t)(w - 1 - y0) * C;
          for (int y = y0; y < y1; ++y, p -= C, d += dp)
            for (int c = 0; c < C; ++c) d[c] = p[c];
        }
      }
    }
  }
}
}  // namespace

void cpu_orient(const uint8_t* src, int64_t src_pitch, int w, int h, int C, uint8_t* dst, int64_t dst_pitch, Orient op,
                int threads) {
  STRIPE_CHECK(C == 1 || C == 3, "orient: image must have 1 or 3 channels, got C = " << C);
  STRIPE_CHECK(src && dst && w >= 1 && h >= 1, "orient: empty image");
  const bool t = orient_t(op), fx = orient_fx(op), fy = orient_fy(op);
  const int W2 = t ? h : w, H2 = t ? w : h;
  STRIPE_CHECK(src_pitch >= (int64_t)w * C && dst_pitch >= (int64_t)W2 * C, "orient: pitch smaller than a row");
  parallel_rows(0, H2, 2 * (int64_t)W2 * C, std::max(1, threads), [&](int ya, int yb) {
    if (!t) {
      for (int y = ya; y < yb; ++y) {
        const uint8_t* s = src + (int64_t)(fy ? h - 1 - y : y) * src_pitch;
        if (C == 1) orient_row<1>(s, dst + (int64_t)y * dst_pitch, w, fx);
        else orient_row<3>(s, dst + (int64_t)y * dst_pitch, w, fx);
      }
    } else if (C == 1) {
      orient_transposed<1>(src, src_pitch, w, h, dst, dst_pitch, fx, fy, ya, yb);
    } else {
      orient_transposed<3>(src, src_pitch, w, h, dst, dst_pitch, fx, fy, ya, yb);
    }
  });
}

Image cpu_orient(const Image& in, Orient op, const CropRect& crop, int threads) {
  STRIPE_CHECK(in.C == 1 || in.C == 3, "orient: image must have 1 or 3 channels, got C = " << in.C);
  STRIPE_CHECK(in.W >= 1 && in.H >= 1 && in.W <= kOrientMaxSize && in.H <= kOrientMaxSize,
               "orient: size " << in.W << "x" << in.H << " outside 1.." << kOrientMaxSize);
  if (!crop.empty())
    check_crop(crop, orient_t(op) ? in.H : in.W, orient_t(op) ? in.W : in.H,
               std::to_string(crop.w) + "x" + std::to_string(crop.h) + "+" + std::to_string(crop.x0) + "+" +
                   std::to_string(crop.y0));
  const CropRect s = orient_source_window(op, in.W, in.H, crop);
  Image out(orient_t(op) ? s.h : s.w, orient_t(op) ? s.w : s.h, in.C, NoInit{});
  cpu_orient(in.row(s.y0) + (size_t)s.x0 * in.C, in.row_bytes(), s.w, s.h, in.C, out.data.data(), out.row_bytes(), op,
             threads);
  return out;
}

// ---- affine warp (stripe/warp.h) ----
namespace {
inline int64_t floor_div64(int64_t n, int64_t d) {  // d > 0
  const int64_t q = n / d;
  return n % d < 0 ? q - 1 : q;
}
inline int64_t ceil_div64(int64_t n, int64_t d) { return -floor_div64(-n, d); }

// the integers x of [*x0, *x1) with lo <= a * x + c < hi, intersected with what [*x0, *x1) held
void linear_span(int64_t a, int64_t c, int64_t lo, int64_t hi, int* x0, int* x1) {
  int64_t b0 = *x0, b1 = *x1;
  if (a == 0) {
    if (c < lo || c >= hi) b1 = b0;
  } else if (a > 0) {
    b0 = std::max(b0, ceil_div64(lo - c, a));
    b1 = std::min(b1, ceil_div64(hi - c, a));
  } else {
    b0 = std::max(b0, floor_div64(c - hi, -a) + 1);
    b1 = std::min(b1, floor_div64(c - lo, -a) + 1);
  }
  b0 = std::min<int64_t>(b0, *x1);  // (an empty span stays inside the old one)
  *x0 = (int)b0;
  *x1 = (int)std::max(b0, b1);
}

// output pixels [xa, xb) of row y; INSIDE: every tap lies inside the frame
template <int C, bool BIL, bool INSIDE>
void warp_span(const uint8_t* src, int64_t sp, int W, int H, uint8_t* drow, const WarpMap& m, int y, int xa, int xb) {
  const bool rep = m.border == WarpBorder::Replicate;
  const uint32_t fill = m.fill;
  auto tap = [&](int iy, int ix, int ch) -> uint32_t {
    if constexpr (!INSIDE) {
      if (rep) {
        iy = std::min(std::max(iy, 0), H - 1);
        ix = std::min(std::max(ix, 0), W - 1);
      } else if (ix < 0 || iy < 0 || ix >= W || iy >= H) {
        return fill;
      }
    }
    return src[(int64_t)iy * sp + (int64_t)ix * C + ch];
  };
  int64_t sx = warp_sx(m, xa, y), sy = warp_sy(m, xa, y);
  uint8_t* o = drow + (size_t)xa * C;
  for (int x = xa; x < xb; ++x, sx += m.A[0][0], sy += m.A[1][0], o += C) {
    if constexpr (BIL) {
      const int64_t X = (sx + (1 << 15)) >> 16, Y = (sy + (1 << 15)) >> 16;
      const int ix = (int)(X >> 8), iy = (int)(Y >> 8);
      const uint32_t fx = (uint32_t)(X & 255), fy = (uint32_t)(Y & 255);
      for (int ch = 0; ch < C; ++ch)
        o[ch] = (uint8_t)warp_bilinear(tap(iy, ix, ch), tap(iy, ix + 1, ch), tap(iy + 1, ix, ch),
                                       tap(iy + 1, ix + 1, ch), fx, fy);
    } else {
      const int ix = (int)((sx + (1 << 23)) >> 24), iy = (int)((sy + (1 << 23)) >> 24);
      for (int ch = 0; ch < C; ++ch) o[ch] = (uint8_t)tap(iy, ix, ch);
    }
  }
}

template <int C, bool BIL>
void warp_rows(const uint8_t* src, int64_t sp, int W, int H, uint8_t* dst, int64_t dp, const WarpMap& m, int ya, int yb) {
  // every tap inside the frame: lo <= sx < hix and lo <= sy < hiy (bilinear: ix >= 0 and ix + 1 <= W - 1)
  const int64_t lo = BIL ? -(int64_t(1) << 15) : -(int64_t(1) << 23);
  const int64_t hix = ((int64_t)(BIL ? W - 1 : W) << 24) + lo, hiy = ((int64_t)(BIL ? H - 1 : H) << 24) + lo;
  for (int y = ya; y < yb; ++y) {
    int x0 = 0, x1 = m.W2;
    linear_span(m.A[0][0], (int64_t)m.A[0][1] * y + m.B[0], lo, hix, &x0, &x1);
    linear_span(m.A[1][0], (int64_t)m.A[1][1] * y + m.B[1], lo, hiy, &x0, &x1);
    uint8_t* drow = dst + (int64_t)y * dp;
    if (x1 <= x0) {
      warp_span<C, BIL, false>(src, sp, W, H, drow, m, y, 0, m.W2);
      continue;
    }
    warp_span<C, BIL, false>(src, sp, W, H, drow, m, y, 0, x0);
    warp_span<C, BIL, true>(src, sp, W, H, drow, m, y, x0, x1);
    warp_span<C, BIL, false>(src, sp, W, H, drow, m, y, x1, m.W2);
  }
}
}  // namespace

void cpu_warp(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch,
              const WarpMap& m, int threads) {
  STRIPE_CHECK(C == 1 || C == 3, "warp: image must have 1 or 3 channels, got C = " << C);
  STRIPE_CHECK(src && dst, "warp: empty image");
  STRIPE_CHECK(W >= 1 && H >= 1 && W <= kWarpMaxSize && H <= kWarpMaxSize,
               "warp: source size " << W << "x" << H << " outside 1.." << kWarpMaxSize);
  STRIPE_CHECK(m.W2 >= 1 && m.H2 >= 1 && m.W2 <= kWarpMaxSize && m.H2 <= kWarpMaxSize,
               "warp: destination size " << m.W2 << "x" << m.H2 << " outside 1.." << kWarpMaxSize);
  STRIPE_CHECK(src_pitch >= (int64_t)W * C && dst_pitch >= (int64_t)m.W2 * C, "warp: pitch smaller than a row");
  const bool bil = m.mode == WarpMode::Bilinear;
  parallel_rows(0, m.H2, (bil ? 5 : 2) * (int64_t)m.W2 * C, std::max(1, threads), [&](int ya, int yb) {
    if (C == 1) {
      if (bil) warp_rows<1, true>(src, src_pitch, W, H, dst, dst_pitch, m, ya, yb);
      else warp_rows<1, false>(src, src_pitch, W, H, dst, dst_pitch, m, ya, yb);
    } else {
      if (bil) warp_rows<3, true>(src, src_pitch, W, H, dst, dst_pitch, m, ya, yb);
      else warp_rows<3, false>(src, src_pitch, W, H, dst, dst_pitch, m, ya, yb);
    }
  });
}

Image cpu_warp(const Image& in, const WarpMap& m, int threads) {
  STRIPE_CHECK(in.C == 1 || in.C == 3, "warp: image must have 1 or 3 channels, got C = " << in.C);
  STRIPE_CHECK(m.W2 >= 1 && m.H2 >= 1 && m.W2 <= kWarpMaxSize && m.H2 <= kWarpMaxSize,
               "warp: destination size " << m.W2 << "x" << m.H2 << " outside 1.." << kWarpMaxSize);
  Image out(m.W2, m.H2, in.C, NoInit{});
  cpu_warp(in.data.data(), in.row_bytes(), in.W, in.H, in.C, out.data.data(), out.row_bytes(), m, threads);
  return out;
}

// ---- mesh warp (stripe/remap.h) ----
namespace {
template <int C, bool BIL>
void remap_rows(const uint8_t* src, int64_t sp, int W, int H, uint8_t* dst, int64_t dp, const RemapMesh& m, int ya, int yb) {
  const int s = m.shift, gw = m.gw();
  const int64_t S = int64_t(1) << s;
  const bool rep = m.border == WarpBorder::Replicate;
  const uint32_t fill = m.fill;
  const int sh = BIL ? 4 + 2 * s : 12 + 2 * s;
  const int64_t rnd = int64_t(1) << (sh - 1);
  auto tap = [&](int64_t iy, int64_t ix, int ch) -> uint32_t {
    if (rep) {
      iy = std::min<int64_t>(std::max<int64_t>(iy, 0), H - 1);
      ix = std::min<int64_t>(std::max<int64_t>(ix, 0), W - 1);
    } else if (ix < 0 || iy < 0 || ix >= W || iy >= H) {
      return fill;
    }
    return src[iy * sp + ix * C + ch];
  };
  for (int y = ya; y < yb; ++y) {
    const int i = y >> s;
    const int64_t ty = y & (S - 1);
    const int32_t* n0 = m.nodes + (size_t)i * gw * 2;
    const int32_t* n1 = n0 + (size_t)gw * 2;
    uint8_t* o = dst + (int64_t)y * dp;
    for (int x0 = 0; x0 < m.W2; x0 += (int)S) {
      const int j = x0 >> s;
      // the cell's left and right edges at this row; P = S L + tx (R - L)
      const int64_t Lx = (S - ty) * n0[2 * j] + ty * n1[2 * j], Rx = (S - ty) * n0[2 * j + 2] + ty * n1[2 * j + 2];
      const int64_t Ly = (S - ty) * n0[2 * j + 1] + ty * n1[2 * j + 1], Ry = (S - ty) * n0[2 * j + 3] + ty * n1[2 * j + 3];
      int64_t Px = S * Lx + rnd, Py = S * Ly + rnd;
      const int64_t dx = Rx - Lx, dy = Ry - Ly;
      const int xe = std::min<int64_t>(x0 + S, m.W2);
      for (int x = x0; x < xe; ++x, Px += dx, Py += dy, o += C) {
        if constexpr (BIL) {
          const int64_t X = Px >> sh, Y = Py >> sh;
          const int64_t ix = X >> 8, iy = Y >> 8;
          const uint32_t fx = (uint32_t)(X & 255), fy = (uint32_t)(Y & 255);
          if (ix >= 0 && iy >= 0 && ix + 1 < W && iy + 1 < H) {  // every tap inside the frame
            const uint8_t* q = src + iy * sp + ix * C;
            for (int ch = 0; ch < C; ++ch) o[ch] = (uint8_t)warp_bilinear(q[ch], q[C + ch], q[sp + ch], q[sp + C + ch], fx, fy);
          } else {
            for (int ch = 0; ch < C; ++ch)
              o[ch] = (uint8_t)warp_bilinear(tap(iy, ix, ch), tap(iy, ix + 1, ch), tap(iy + 1, ix, ch),
                                             tap(iy + 1, ix + 1, ch), fx, fy);
          }
        } else {
          const int64_t ix = Px >> sh, iy = Py >> sh;
          for (int ch = 0; ch < C; ++ch) o[ch] = (uint8_t)tap(iy, ix, ch);
        }
      }
    }
  }
}
}  // namespace

void cpu_remap(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch,
               const RemapMesh& m, int threads) {
  STRIPE_CHECK(C == 1 || C == 3, "remap: image must have 1 or 3 channels, got C = " << C);
  STRIPE_CHECK(src && dst, "remap: empty image");
  STRIPE_CHECK(W >= 1 && H >= 1 && W <= kWarpMaxSize && H <= kWarpMaxSize,
               "remap: source size " << W << "x" << H << " outside 1.." << kWarpMaxSize);
  check_mesh(m, (int64_t)m.gh() * m.gw() * 2, true);
  STRIPE_CHECK(src_pitch >= (int64_t)W * C && dst_pitch >= (int64_t)m.W2 * C, "remap: pitch smaller than a row");
  const bool bil = m.mode == WarpMode::Bilinear;
  parallel_rows(0, m.H2, (bil ? 6 : 3) * (int64_t)m.W2 * C, std::max(1, threads), [&](int ya, int yb) {
    if (C == 1) {
      if (bil) remap_rows<1, true>(src, src_pitch, W, H, dst, dst_pitch, m, ya, yb);
      else remap_rows<1, false>(src, src_pitch, W, H, dst, dst_pitch, m, ya, yb);
    } else {
      if (bil) remap_rows<3, true>(src, src_pitch, W, H, dst, dst_pitch, m, ya, yb);
      else remap_rows<3, false>(src, src_pitch, W, H, dst, dst_pitch, m, ya, yb);
    }
  });
}

Image cpu_remap(const Image& in, const RemapMesh& m, int threads) {
  STRIPE_CHECK(in.C == 1 || in.C == 3, "remap: image must have 1 or 3 channels, got C = " << in.C);
  check_mesh(m, (int64_t)m.gh() * m.gw() * 2, true);
  Image out(m.W2, m.H2, in.C, NoInit{});
  cpu_remap(in.data.data(), in.row_bytes(), in.W, in.H, in.C, out.data.data(), out.row_bytes(), m, threads);
  return out;
}

// ---- connected components (stripe/components.h) ----
namespace {

// f(t) for t in [0, T) on T threads (the caller's among them); the first exception is rethrown after all joined.
template <class F>
void run_blocks(int T, F&& f) {
  if (T <= 1) {
    f(0);
    return;
  }
  std::vector<std::exception_ptr> err((size_t)T);
  auto guarded = [&f, &err](int t) {
    try {
      f(t);
    } catch (...) {
      err[(size_t)t] = std::current_exception();
    }
  };
  std::vector<std::thread> th;
  th.reserve((size_t)T - 1);
  try {
    for (int t = 1; t < T; ++t) th.emplace_back(guarded, t);
  } catch (...) {
    err[0] = std::current_exception();
  }
  if (!err[0]) guarded(0);
  for (auto& t : th) t.join();
  for (auto& e : err)
    if (e) std::rethrow_exception(e);
}

// The forest in the label plane: slot i (raster index y * W + x, at y * lp + x) holds 0 (background) or its
// parent's raster index + 1; a root holds its own.  Parents never have a larger index than their children.
struct Forest {
  int32_t* L;
  int64_t lp;
  int W;
  int32_t* at(int64_t i) const {
    const int64_t y = i / W;
    return L + y * lp + (i - y * W);
  }
  int64_t find(int64_t i) const {
    int64_t r = i;
    for (int64_t p; (p = *at(r) - 1) != r;) r = p;
    for (int64_t p; (p = *at(i) - 1) != r; i = p) *at(i) = (int32_t)(r + 1);  // compress
    return r;
  }
  void unite(int64_t a, int64_t b) const {
    a = find(a), b = find(b);
    if (a == b) return;
    *at(std::max(a, b)) = (int32_t)(std::min(a, b) + 1);
  }
  // links the run [xs, xe) of row y (head y * W + xs) with the runs of row y - 1 it touches
  void link_up(const uint8_t* prev, int y, int xs, int xe, int conn) const {
    const int a = conn == 8 ? std::max(xs - 1, 0) : xs, b = conn == 8 ? std::min(xe + 1, W) : xe;
    for (int x = a; x < b; ++x)
      if (prev[x] != 0 && (x == a || prev[x - 1] == 0)) unite((int64_t)y * W + xs, (int64_t)(y - 1) * W + x);
  }
};

inline int32_t ld(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
inline void st(int32_t* p, int32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

}  // namespace

int cpu_components(const uint8_t* src, int64_t sp, int W, int H, int conn, int32_t* labels, int64_t lp, int threads) {
  check_components(W, H, 1, conn);
  STRIPE_CHECK(src && labels, "components: empty image");
  STRIPE_CHECK(sp >= W && lp >= W, "components: pitch smaller than a row");
  const Forest F{labels, lp, W};
  const int T = std::max(1, std::min(threads, H));
  auto y_of = [&](int t) { return (int)((int64_t)H * t / T); };
  // 1. per block: the runs of every row, linked with the runs of the row above inside the block
  run_blocks(T, [&](int t) {
    for (int y = y_of(t); y < y_of(t + 1); ++y) {
      const uint8_t* s = src + (int64_t)y * sp;
      int32_t* l = labels + (int64_t)y * lp;
      for (int x = 0; x < W;) {
        if (s[x] == 0) {
          l[x++] = 0;
          continue;
        }
        const int xs = x;
        const int32_t head = (int32_t)((int64_t)y * W + xs + 1);
        while (x < W && s[x] != 0) l[x++] = head;
        if (y > y_of(t)) F.link_up(s - sp, y, xs, x, conn);
      }
    }
  });
  // 2. the seams between the blocks
  for (int t = 1; t < T; ++t) {
    const int y = y_of(t);
    const uint8_t* s = src + (int64_t)y * sp;
    for (int x = 0; x < W;) {
      if (s[x] == 0) {
        ++x;
        continue;
      }
      const int xs = x;
      while (x < W && s[x] != 0) ++x;
      F.link_up(s - sp, y, xs, x, conn);
    }
  }
  // 3. flatten (every slot takes its root; a block reads other blocks' slots while they are rewritten: any
  // value a slot ever holds is an ancestor, and roots do not change) and count the roots per block
  std::vector<int64_t> base((size_t)T + 1, 0);
  run_blocks(T, [&](int t) {
    int64_t roots = 0;
    for (int y = y_of(t); y < y_of(t + 1); ++y) {
      int32_t* l = labels + (int64_t)y * lp;
      for (int x = 0; x < W; ++x) {
        const int32_t v = ld(l + x);
        if (v == 0) continue;
        const int64_t self = (int64_t)y * W + x;
        int64_t r = v - 1;
        if (r == self) {
          ++roots;
          continue;
        }
        for (int64_t p; (p = ld(F.at(r)) - 1) != r;) r = p;
        st(l + x, (int32_t)(r + 1));
      }
    }
    base[(size_t)t + 1] = roots;
  });
  for (int t = 0; t < T; ++t) base[(size_t)t + 1] += base[(size_t)t];
  STRIPE_CHECK(base[(size_t)T] <= INT32_MAX, "components: too many components");
  // 4. the roots take minus their number, in raster order
  run_blocks(T, [&](int t) {
    int32_t n = (int32_t)base[(size_t)t];
    for (int y = y_of(t); y < y_of(t + 1); ++y) {
      int32_t* l = labels + (int64_t)y * lp;
      for (int x = 0; x < W; ++x)
        if (l[x] != 0 && l[x] - 1 == (int64_t)y * W + x) l[x] = -(++n);
    }
  });
  // 5. every pixel takes its root's number (a root's slot holds -n until its own block rewrites it to n)
  run_blocks(T, [&](int t) {
    for (int y = y_of(t); y < y_of(t + 1); ++y) {
      int32_t* l = labels + (int64_t)y * lp;
      for (int x = 0; x < W; ++x) {
        const int32_t v = ld(l + x);
        if (v == 0) continue;
        const int32_t n = v < 0 ? v : ld(F.at(v - 1));
        st(l + x, n < 0 ? -n : n);
      }
    }
  });
  return (int)base[(size_t)T];
}

std::vector<int64_t> cpu_component_stats(const int32_t* labels, int64_t lp, int W, int H, int N, int threads) {
  STRIPE_CHECK(labels && W >= 1 && H >= 1 && lp >= W && N >= 0, "components: bad label plane");
  const int T = std::max(1, std::min(threads, H));
  const size_t n = (size_t)(N + 1) * kStatCols;
  std::vector<std::vector<int64_t>> part((size_t)T);
  run_blocks(T, [&](int t) {
    std::vector<int64_t>& tb = part[(size_t)t];
    tb.assign(n, 0);
    for (int l = 0; l <= N; ++l) tb[(size_t)l * kStatCols + 1] = tb[(size_t)l * kStatCols + 2] = INT64_MAX;
    for (int y = (int)((int64_t)H * t / T); y < (int)((int64_t)H * (t + 1) / T); ++y) {
      const int32_t* r = labels + (int64_t)y * lp;
      for (int x = 0; x < W;) {  // per run of equal labels
        const int32_t l = r[x];
        STRIPE_CHECK(l >= 0 && l <= N, "components: label " << l << " outside 0.." << N);
        const int64_t xs = x;
        while (x < W && r[x] == l) ++x;
        const int64_t len = x - xs;
        int64_t* e = tb.data() + (size_t)l * kStatCols;
        e[0] += len;
        e[1] = std::min(e[1], xs), e[2] = std::min<int64_t>(e[2], y);
        e[3] = std::max<int64_t>(e[3], x), e[4] = std::max<int64_t>(e[4], y + 1);
        e[5] += len * xs + len * (len - 1) / 2, e[6] += len * y;
      }
    }
  });
  std::vector<int64_t> out = std::move(part[0]);
  for (int t = 1; t < T; ++t)
    for (int l = 0; l <= N; ++l) {
      int64_t* e = out.data() + (size_t)l * kStatCols;
      const int64_t* p = part[(size_t)t].data() + (size_t)l * kStatCols;
      e[0] += p[0], e[5] += p[5], e[6] += p[6];
      e[1] = std::min(e[1], p[1]), e[2] = std::min(e[2], p[2]);
      e[3] = std::max(e[3], p[3]), e[4] = std::max(e[4], p[4]);
    }
  for (int l = 0; l <= N; ++l) {
    int64_t* e = out.data() + (size_t)l * kStatCols;
    if (e[0] == 0) e[1] = e[2] = 0;
  }
  return out;
}

Image cpu_area_filter(const Image& img, int conn, int64_t amin, int64_t amax, int threads) {
  check_components(img.W, img.H, img.C, conn);
  check_area_bounds(amin, amax);
  const int W = img.W, H = img.H;
  std::vector<int32_t> labels((size_t)W * H);
  const int N = cpu_components(img.data.data(), W, W, H, conn, labels.data(), W, threads);
  const std::vector<int64_t> tb = cpu_component_stats(labels.data(), W, W, H, N, threads);
  Image out(W, H, 1, NoInit{});
  parallel_rows(0, H, 6 * (int64_t)W, std::max(1, threads), [&](int ya, int yb) {
    for (int64_t p = (int64_t)ya * W; p < (int64_t)yb * W; ++p) {
      const int32_t l = labels[(size_t)p];
      const int64_t a = tb[(size_t)l * kStatCols];
      out.data[(size_t)p] = l != 0 && a >= amin && a <= amax ? img.data[(size_t)p] : 0;
    }
  });
  return out;
}

// ---- distance transform (stripe/distance.h) ----
namespace {

constexpr int32_t kNoG = -1;  // g: the column has no site

// One row of the squared distance from its g values: the lower envelope of the parabolas
// (x - i)^2 + g(i)^2 over the columns i that have a site (Meijster's scan, integers only).
// s: the envelope's columns, t: where each takes over; both W entries.
void edt_row(const int32_t* g, int W, int32_t* out, int32_t* s, int32_t* t) {
  const auto F = [g](int64_t x, int64_t i) { return (x - i) * (x - i) + (int64_t)g[i] * g[i]; };
  int q = -1;
  for (int u = 0; u < W; ++u) {
    if (g[u] == kNoG) continue;
    while (q >= 0 && F(t[q], s[q]) > F(t[q], u)) --q;
    if (q < 0) {
      q = 0, s[0] = u, t[0] = 0;
    } else {
      // the first x at which u is no worse than s[q]: 1 + floor(num / den), num >= 0 after the loop above
      const int64_t i = s[q];
      const int64_t num = (int64_t)u * u - i * i + (int64_t)g[u] * g[u] - (int64_t)g[i] * g[i], den = 2 * (u - i);
      const int64_t w = 1 + (num >= 0 ? num / den : -((-num + den - 1) / den));
      if (w < W) ++q, s[q] = u, t[q] = (int32_t)std::max<int64_t>(w, 0);
    }
  }
  if (q < 0) {
    std::fill(out, out + W, kDistanceNone);
    return;
  }
  for (int u = W - 1; u >= 0; --u) {
    out[u] = (int32_t)F(u, s[q]);
    if (u == t[q] && q > 0) --q;
  }
}

}  // namespace

void cpu_distance(const uint8_t* src, int64_t sp, int W, int H, bool to_foreground, int32_t* out, int64_t op,
                  int threads) {
  check_distance(W, H, 1);
  STRIPE_CHECK(src && out, "distance: empty image");
  STRIPE_CHECK(sp >= W && op >= W, "distance: pitch smaller than a row");
  const int T = std::max(1, threads);
  // column pass: g into the output plane, column blocks of whole cache lines, rows walked down and up
  constexpr int kColBlock = 256;
  const int ncb = (int)div_up(W, kColBlock);
  const int TC = std::min(T, ncb);
  run_blocks(TC, [&](int tb) {
    for (int cb = (int)((int64_t)ncb * tb / TC); cb < (int)((int64_t)ncb * (tb + 1) / TC); ++cb) {
      const int xa = cb * kColBlock, xb = std::min(W, xa + kColBlock);
      for (int y = 0; y < H; ++y) {
        const uint8_t* r = src + (int64_t)y * sp;
        int32_t* o = out + (int64_t)y * op;
        const int32_t* up = y > 0 ? o - op : nullptr;
        for (int x = xa; x < xb; ++x)
          o[x] = (r[x] != 0) == to_foreground ? 0 : (up && up[x] != kNoG ? up[x] + 1 : kNoG);
      }
      for (int y = H - 2; y >= 0; --y) {
        int32_t* o = out + (int64_t)y * op;
        const int32_t* dn = o + op;
        for (int x = xa; x < xb; ++x)
          if (dn[x] != kNoG && (o[x] == kNoG || dn[x] + 1 < o[x])) o[x] = dn[x] + 1;
      }
    }
  });
  // row pass, in place through a copy of the row's g
  parallel_rows(0, H, 16 * (int64_t)W, T, [&](int ya, int yb) {
    std::vector<int32_t> g((size_t)W), s((size_t)W), t((size_t)W);
    for (int y = ya; y < yb; ++y) {
      int32_t* o = out + (int64_t)y * op;
      std::copy(o, o + W, g.begin());
      edt_row(g.data(), W, o, s.data(), t.data());
    }
  });
}

namespace {

template <class F>
Image distance_map(const Image& img, bool to_foreground, int threads, F&& f) {
  check_distance(img.W, img.H, img.C);
  const int W = img.W, H = img.H;
  std::vector<int32_t> d((size_t)W * H);
  cpu_distance(img.data.data(), W, W, H, to_foreground, d.data(), W, threads);
  Image out(W, H, 1, NoInit{});
  parallel_rows(0, H, 5 * (int64_t)W, std::max(1, threads), [&](int ya, int yb) {
    for (int64_t p = (int64_t)ya * W; p < (int64_t)yb * W; ++p) out.data[(size_t)p] = f(d[(size_t)p]);
  });
  return out;
}

}  // namespace

Image cpu_distance_u8(const Image& img, bool to_foreground, int threads) {
  return distance_map(img, to_foreground, threads, [](int32_t d2) { return distance_u8(d2); });
}

Image cpu_distance_mask(const Image& img, bool to_foreground, int32_t t, bool keep_above, int threads) {
  check_distance_mode((int)DistanceMode::MaskAbove, t);
  return distance_map(img, to_foreground, threads, [=](int32_t d2) { return distance_mask(d2, t, keep_above); });
}

Image cpu_disk_morph(const Image& img, DiskOp op, double radius, int threads) {
  check_distance(img.W, img.H, img.C);
  const int32_t t = check_radius(radius);
  switch (op) {
    case DiskOp::Erode: return cpu_distance_mask(img, false, t, true, threads);
    case DiskOp::Dilate: return cpu_distance_mask(img, true, t, false, threads);
    case DiskOp::Open: return cpu_distance_mask(cpu_distance_mask(img, false, t, true, threads), true, t, false, threads);
    case DiskOp::Close: return cpu_distance_mask(cpu_distance_mask(img, true, t, false, threads), false, t, true, threads);
  }
  fail("distance: unknown disc operation");
}

// ---- integral images (stripe/integral.h) ----
namespace {

// The wrapping u32 integral of a frame of We x He values given row by row: t is (He + 1) rows of pitch tp, row 0
// and column 0 zero.  Row blocks are scanned on their own (a running row sum plus the row above inside the
// block), then every block but the first takes the carry row: the last row of the block above, itself carried.
// u32 addition is associative modulo 2^32, so the table does not depend on the number of blocks.
template <class RowFn>
void sat_build(int We, int He, uint32_t* t, int64_t tp, int threads, RowFn&& row) {
  const int T = std::max(1, std::min(threads, He));
  std::fill(t, t + We + 1, 0u);
  const auto ya = [&](int b) { return (int)((int64_t)He * b / T); };
  run_blocks(T, [&](int b) {
    std::vector<uint32_t> v((size_t)We);
    for (int y = ya(b); y < ya(b + 1); ++y) {
      row(y, v.data());
      uint32_t* o = t + (int64_t)(y + 1) * tp;
      const uint32_t* up = o - tp;
      const bool first = y == ya(b);
      uint32_t run = 0;
      o[0] = 0;
      for (int x = 0; x < We; ++x) {
        run += v[(size_t)x];
        o[x + 1] = run + (first ? 0u : up[x + 1]);
      }
    }
  });
  if (T == 1) return;
  // block b's carry is the finished last row of block b - 1: finish those rows in order, then the rest at once
  for (int b = 1; b < T; ++b) {
    const uint32_t* c = t + (int64_t)ya(b) * tp;
    uint32_t* last = t + (int64_t)ya(b + 1) * tp;
    if (ya(b + 1) > ya(b))
      for (int x = 1; x <= We; ++x) last[x] += c[x];
  }
  run_blocks(T, [&](int b) {
    if (b == 0) return;
    const uint32_t* c = t + (int64_t)ya(b) * tp;
    for (int y = ya(b); y + 1 < ya(b + 1); ++y) {
      uint32_t* o = t + (int64_t)(y + 1) * tp;
      for (int x = 1; x <= We; ++x) o[x] += c[x];
    }
  });
}

}  // namespace

void cpu_integral(const uint8_t* src, int64_t sp, int W, int H, bool squared, int32_t* out, int64_t op, int threads) {
  check_integral(W, H, 1);
  STRIPE_CHECK(src && out, "integral: empty image");
  STRIPE_CHECK(sp >= W && op >= (int64_t)W + 1, "integral: pitch smaller than a row");
  sat_build(W, H, reinterpret_cast<uint32_t*>(out), op, threads, [&](int y, uint32_t* v) {
    const uint8_t* r = src + (int64_t)y * sp;
    for (int x = 0; x < W; ++x) v[x] = squared ? (uint32_t)r[x] * r[x] : (uint32_t)r[x];
  });
}

void cpu_window(const uint8_t* src, int64_t sp, int W, int H, const WindowSpec& spec, Border border, uint8_t* dst,
                int64_t dp, int threads) {
  check_integral(W, H, 1);
  check_window((int)spec.op, spec.K, border, spec.C, spec.kq);
  STRIPE_CHECK(src && dst, "integral: empty image");
  STRIPE_CHECK(sp >= W && dp >= W, "integral: pitch smaller than a row");
  const int K = spec.K, R = K / 2, We = W + 2 * R, He = H + 2 * R;
  const int64_t tp = (int64_t)We + 1;
  const bool sq = window_uses_squares(spec.op);
  std::vector<int> cx((size_t)We);
  for (int x = 0; x < We; ++x) cx[(size_t)x] = border_index(x - R, W, border);
  const auto ext_row = [&](int y, uint32_t* v, bool squared) {
    const int sy = border_index(y - R, H, border);
    if (sy < 0) {
      std::fill(v, v + We, 0u);
      return;
    }
    const uint8_t* r = src + (int64_t)sy * sp;
    for (int x = 0; x < We; ++x) {
      const uint32_t p = cx[(size_t)x] < 0 ? 0u : r[cx[(size_t)x]];
      v[x] = squared ? p * p : p;
    }
  };
  std::vector<uint32_t> ta((size_t)(tp * (He + 1))), tb(sq ? ta.size() : 0);
  sat_build(We, He, ta.data(), tp, threads, [&](int y, uint32_t* v) { ext_row(y, v, false); });
  if (sq) sat_build(We, He, tb.data(), tp, threads, [&](int y, uint32_t* v) { ext_row(y, v, true); });
  const uint32_t N = (uint32_t)K * (uint32_t)K;
  parallel_rows(0, H, 24 * (int64_t)W, std::max(1, threads), [&](int y0, int y1) {
    for (int y = y0; y < y1; ++y) {
      const uint32_t *a0 = ta.data() + (int64_t)y * tp, *a1 = a0 + (int64_t)K * tp;
      const uint32_t *b0 = sq ? tb.data() + (int64_t)y * tp : nullptr, *b1 = sq ? b0 + (int64_t)K * tp : nullptr;
      const uint8_t* r = src + (int64_t)y * sp;
      uint8_t* o = dst + (int64_t)y * dp;
      for (int x = 0; x < W; ++x) {
        const uint32_t A = a1[x + K] - a0[x + K] - a1[x] + a0[x];
        const uint32_t B = sq ? b1[x + K] - b0[x + K] - b1[x] + b0[x] : 0u;
        o[x] = window_rule((int)spec.op, r[x], A, B, N, spec.C, spec.kq);
      }
    }
  });
}

// ---- canny and hysteresis thresholding (stripe/canny.h) ----
namespace {

// magnitudes carry their sector in the top bits (a magnitude is below 2^21)
constexpr int kCannySectorShift = 24;
constexpr uint32_t kCannyMagMask = (1u << kCannySectorShift) - 1u;

}  // namespace

void cpu_canny_classes(const uint8_t* src, int64_t sp, int W, int H, int low, int high, CannyNorm norm, Border border,
                       uint8_t* dst, int64_t dp, int threads) {
  check_canny(W, H, 1, low, high, (int)norm, border);
  STRIPE_CHECK(src && dst, "canny: empty image");
  STRIPE_CHECK(sp >= W && dp >= W, "canny: pitch smaller than a row");
  const bool l2 = norm == CannyNorm::L2;
  const uint32_t lo = l2 ? (uint32_t)low * low : (uint32_t)low, hi = l2 ? (uint32_t)high * high : (uint32_t)high;
  std::vector<int> cx((size_t)W + 2);
  for (int x = 0; x < W + 2; ++x) cx[(size_t)x] = border_index(x - 1, W, border);
  const size_t We = (size_t)W + 2;
  parallel_rows(0, H, 16 * (int64_t)W, std::max(1, threads), [&](int y0, int y1) {
    const int n = y1 - y0;
    // the extended rows y0 - 2 .. y1 + 1 (those of magnitude rows outside the frame stay unused), then the
    // magnitude rows y0 - 1 .. y1 with a zero column on both sides; rows outside the frame are zero
    std::vector<uint8_t> P(We * (size_t)(n + 4));
    std::vector<uint32_t> M(We * (size_t)(n + 2), 0u);
    for (int r = 0; r < n + 4; ++r) {
      const int y = y0 - 2 + r;
      if (y < -1 || y > H) continue;
      const int sy = border_index(y, H, border);
      uint8_t* p = P.data() + We * (size_t)r;
      if (sy < 0) {
        std::fill(p, p + We, (uint8_t)0);
        continue;
      }
      const uint8_t* s = src + (int64_t)sy * sp;
      for (size_t x = 0; x < We; ++x) p[x] = cx[x] < 0 ? (uint8_t)0 : s[cx[x]];
    }
    for (int r = 0; r < n + 2; ++r) {
      const int y = y0 - 1 + r;
      if (y < 0 || y >= H) continue;
      const uint8_t *a = P.data() + We * (size_t)r, *b = a + We, *c = b + We;  // the extended rows y - 1, y, y + 1
      uint32_t* m = M.data() + We * (size_t)r + 1;
      for (int x = 0; x < W; ++x) {
        const int gx = (a[x + 2] + 2 * b[x + 2] + c[x + 2]) - (a[x] + 2 * b[x] + c[x]);
        const int gy = (c[x] + 2 * c[x + 1] + c[x + 2]) - (a[x] + 2 * a[x + 1] + a[x + 2]);
        m[x] = canny_magnitude(gx, gy, l2) | ((uint32_t)canny_sector(gx, gy) << kCannySectorShift);
      }
    }
    for (int y = y0; y < y1; ++y) {
      const uint32_t* m = M.data() + We * (size_t)(y - y0 + 1) + 1;
      uint8_t* o = dst + (int64_t)y * dp;
      for (int x = 0; x < W; ++x) {
        const int s = (int)(m[x] >> kCannySectorShift);
        const ptrdiff_t d = (ptrdiff_t)canny_dy(s) * (ptrdiff_t)We + canny_dx(s);
        o[x] = canny_class(m[x] & kCannyMagMask, m[x - d] & kCannyMagMask, m[x + d] & kCannyMagMask, s, lo, hi);
      }
    }
  });
}

void cpu_hysteresis(const uint8_t* cls, int64_t cp, int W, int H, int conn, uint8_t* dst, int64_t dp, int threads) {
  check_components(W, H, 1, conn);
  STRIPE_CHECK(cls && dst, "canny: empty image");
  STRIPE_CHECK(cp >= W && dp >= W, "canny: pitch smaller than a row");
  std::vector<int32_t> labels((size_t)W * H);
  const int N = cpu_components(cls, cp, W, H, conn, labels.data(), W, threads);
  std::vector<uint8_t> strong((size_t)N + 1, 0);  // per label: the component holds a class 2 pixel
  for (int y = 0; y < H; ++y) {
    const uint8_t* c = cls + (int64_t)y * cp;
    const int32_t* l = labels.data() + (size_t)y * W;
    for (int x = 0; x < W; ++x)
      if (c[x] >= 2) strong[(size_t)l[x]] = 1;
  }
  strong[0] = 0;
  parallel_rows(0, H, 6 * (int64_t)W, std::max(1, threads), [&](int ya, int yb) {
    for (int y = ya; y < yb; ++y) {
      const int32_t* l = labels.data() + (size_t)y * W;
      uint8_t* o = dst + (int64_t)y * dp;
      for (int x = 0; x < W; ++x) o[x] = strong[(size_t)l[x]] ? 255 : 0;
    }
  });
}

void cpu_canny(const uint8_t* src, int64_t sp, int W, int H, int low, int high, CannyNorm norm, Border border,
               uint8_t* dst, int64_t dp, int threads) {
  check_canny(W, H, 1, low, high, (int)norm, border);
  std::vector<uint8_t> cls((size_t)W * H);
  cpu_canny_classes(src, sp, W, H, low, high, norm, border, cls.data(), W, threads);
  cpu_hysteresis(cls.data(), W, W, H, 8, dst, dp, threads);
}

void cpu_hysteresis_threshold(const uint8_t* src, int64_t sp, int W, int H, int low, int high, int conn, uint8_t* dst,
                              int64_t dp, int threads) {
  check_hysteresis(W, H, 1, low, high, conn);
  STRIPE_CHECK(src && dst, "canny: empty image");
  STRIPE_CHECK(sp >= W && dp >= W, "canny: pitch smaller than a row");
  std::vector<uint8_t> cls((size_t)W * H);
  parallel_rows(0, H, 2 * (int64_t)W, std::max(1, threads), [&](int ya, int yb) {
    for (int y = ya; y < yb; ++y) {
      const uint8_t* s = src + (int64_t)y * sp;
      uint8_t* c = cls.data() + (size_t)y * W;
      for (int x = 0; x < W; ++x) c[x] = hysteresis_class(s[x], (uint32_t)low, (uint32_t)high);
    }
  });
  cpu_hysteresis(cls.data(), W, W, H, conn, dst, dp, threads);
}

}  // namespace stripe
