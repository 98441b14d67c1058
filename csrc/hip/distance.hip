// Exact squared Euclidean distance transform on the device (k_edt_*).  The rule
// is stripe/distance.h's; the int32 plane, the u8 form and the masks are
// bit-identical to the golden functions.
//
// d2(x, y) = min over x' of (x - x')^2 + g(x', y)^2, where g(x', y) is the
// vertical distance to the nearest site of column x'.  The passes of
// distance_device, all queued on the caller's stream, none waited for:
//
//   k_edt_bits   a lane per 4 columns and band of kEdtBand = 64 rows: the band's
//                site bits of each column as one u64 (bit r: row r of the band),
//                4 mask bytes per dword load where the view is aligned to 4,
//                single bytes otherwise and at a row's ragged end.  The polarity
//                is one xor here; no other pass knows it.
//   k_edt_carry  a lane per column walks the H / kEdtBand words down and up: for
//                every band the nearest site row above it and below it (u16,
//                kEdtNoG: none).
//   k_edt_band   a lane per 4 columns and band: g for its 64 rows from the word's
//                leading / trailing zero counts and the two carries, u16 with
//                kEdtNoG = 0xFFFF for a column without any site, 8 bytes a store.
//   k_edt_row    one workgroup per row, the row's g in LDS.  The leftmost
//                arg-min a(x) of (x - x')^2 + g(x')^2 does not decrease with x
//                (a Monge cost plus a column term; "none" counts as 2^31 - 1),
//                so the columns are solved level by level: x = 0 over the whole
//                row (a minimum of "none" there ends the row: it has no site),
//                x = W - 1 from a(0) on, then the odd multiples of h = P/2, P/4,
//                .. 1 over [a(x - h), a(min(x + h, W - 1))], cut to
//                |x - x'| <= g(x) where the column has a site (nothing farther
//                can win).  A level's ranges total
//                at most W + its queries, so a row costs O(W log W) whatever the
//                mask holds.  A lane solves a query whose range holds at most
//                kEdtLong candidates; longer ranges go to a list in LDS and are
//                scanned by a whole wave each with a shuffle min-reduction on
//                (cost, column) keys.  a(x) lives in LDS beside g as u16; a last
//                coalesced pass recomputes d2 from a(x) and stores int32 d2,
//                u8 floor(sqrt) or the u8 mask (template MODE), so the derived
//                forms never touch a 4 B / pixel plane.
//
// Every loop's trip count is bounded by W, H or a constant: bands by
// H / kEdtBand, levels by 2 + log2 P <= 17, a lane's scan by kEdtLong (by W if the
// list were ever full, which W + queries <= 1.5 * 32767 < kEdtList * kEdtLong
// rules out), a wave's by W / 64, the list by kEdtList.
//
// Arithmetic is u32: (x - x')^2 <= 2^30 plus at most 2^31 - 1; a minimum of
// 2^31 - 1 or more means the row (then the frame) has no site: kDistanceNone.
//
// Scratch per (device, stream, W, H), cached, released by
// distance_release_scratch: g (2 B / pixel), the site words (1 bit / pixel), two
// carries per band and column, and for open / close one u8 mask.
//
// Addressing as k_orient: 64-bit on pitched views, any source pitch >= W at any
// alignment, no byte outside a source row's W bytes read, nothing outside a
// destination row's W elements written.
#include <array>
#include <climits>
#include <list>
#include <mutex>

#include "dev_common.h"
#include "stripe/distance.h"
#include "stripe/kernels.h"

namespace stripe {
namespace dev {

constexpr uint32_t kEdtNoG = 0xFFFFu;
constexpr uint32_t kEdtNoneCost = 0x7FFFFFFFu;  // g^2 of a column without a site

struct EdtArgs {
  const uint8_t* src;
  int64_t sp;  // bytes
  uint16_t* g;
  unsigned long long* bits;  // nb x gp site words
  uint16_t* above;           // nb x gp: the nearest site row above the band / below it
  uint16_t* below;
  int64_t gp;  // elements of a g / bits / carry row: W rounded up to 4
  int W, H, nb;
  uint32_t inv;  // 0xF: the sites are the background pixels
};

// the site bits of pixels x .. x + 3 of a row (bit i: pixel x + i); x is a multiple of 4
template <bool AL>
__device__ __forceinline__ uint32_t site_bits4(const uint8_t* row, int x, int W, uint32_t inv) {
  uint32_t v = 0;
  if (AL && x + 4 <= W) {
    v = *reinterpret_cast<const uint32_t*>(row + x);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x + i < W) v |= (uint32_t)row[x + i] << (8 * i);
  }
  const uint32_t b = ((v & 0xFFu) != 0 ? 1u : 0u) | ((v & 0xFF00u) != 0 ? 2u : 0u) | ((v & 0xFF0000u) != 0 ? 4u : 0u) |
                     ((v & 0xFF000000u) != 0 ? 8u : 0u);
  return b ^ inv;
}

template <bool AL>
__global__ __launch_bounds__(kNT) void k_edt_bits(EdtArgs a) {
  const int x = 4 * (int)(blockIdx.x * kNT + threadIdx.x);
  if (x >= a.W) return;
  const int b = blockIdx.y, y0 = b * kEdtBand;
  const int rows = min(kEdtBand, a.H - y0);
  unsigned long long m[4] = {0, 0, 0, 0};
  const uint8_t* row = a.src + (int64_t)y0 * a.sp;
  for (int r = 0; r < rows; ++r, row += a.sp) {
    const uint32_t s = site_bits4<AL>(row, x, a.W, a.inv);
#pragma unroll
    for (int i = 0; i < 4; ++i) m[i] |= (unsigned long long)((s >> i) & 1u) << r;
  }
  unsigned long long* o = a.bits + (int64_t)b * a.gp + x;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = m[i];
}

__global__ __launch_bounds__(kNT) void k_edt_carry(EdtArgs a) {
  const int x = (int)(blockIdx.x * kNT + threadIdx.x);
  if (x >= a.gp) return;  // the padding columns too: k_edt_band reads whole groups of 4
  uint32_t c = kEdtNoG;
  for (int b = 0; b < a.nb; ++b) {
    const int64_t i = (int64_t)b * a.gp + x;
    a.above[i] = (uint16_t)c;
    const unsigned long long m = a.bits[i];
    if (m) c = (uint32_t)(b * kEdtBand + 63 - __builtin_clzll(m));
  }
  c = kEdtNoG;
  for (int b = a.nb - 1; b >= 0; --b) {
    const int64_t i = (int64_t)b * a.gp + x;
    a.below[i] = (uint16_t)c;
    const unsigned long long m = a.bits[i];
    if (m) c = (uint32_t)(b * kEdtBand + __builtin_ctzll(m));
  }
}

__global__ __launch_bounds__(kNT) void k_edt_band(EdtArgs a) {
  const int x = 4 * (int)(blockIdx.x * kNT + threadIdx.x);
  if (x >= a.W) return;
  const int b = blockIdx.y, y0 = b * kEdtBand;
  const int rows = min(kEdtBand, a.H - y0);
  const int64_t i0 = (int64_t)b * a.gp + x;
  unsigned long long m[4];
  uint32_t up[4], dn[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = a.bits[i0 + i], up[i] = a.above[i0 + i], dn[i] = a.below[i0 + i];
  uint16_t* o = a.g + (int64_t)y0 * a.gp + x;
  for (int r = 0; r < rows; ++r, o += a.gp) {
    const uint32_t y = (uint32_t)(y0 + r);
    uint32_t gv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned long long mu = m[i] & (~0ull >> (63 - r)), ml = m[i] >> r;
      const uint32_t da = mu ? (uint32_t)(r - (63 - __builtin_clzll(mu))) : (up[i] != kEdtNoG ? y - up[i] : kEdtNoG);
      const uint32_t db = ml ? (uint32_t)__builtin_ctzll(ml) : (dn[i] != kEdtNoG ? dn[i] - y : kEdtNoG);
      gv[i] = min(da, db);
    }
    *reinterpret_cast<uint2*>(o) = make_uint2(gv[0] | (gv[1] << 16), gv[2] | (gv[3] << 16));
  }
}

// ---- the row pass ----
template <int WMAX>
struct EdtRowLds {
  uint16_t g[WMAX];
  uint16_t arg[WMAX];
  uint16_t list[kEdtList];
  uint32_t nlong[kEdtCounters];
};
static_assert(sizeof(EdtRowLds<4096>) == (size_t)edt_row_lds_bytes(4096), "kernels.h states the row pass's LDS");
static_assert(sizeof(EdtRowLds<32768>) == (size_t)edt_row_lds_bytes(32768), "kernels.h states the row pass's LDS");

struct EdtRowArgs {
  const uint16_t* g;
  int64_t gp;
  void* dst;
  int64_t dp;  // elements of the destination's type
  int W, H;
  int P;      // the smallest power of two >= W
  int32_t t;  // masks: the threshold
  int above;  // masks: 255 where d2 > t, else where d2 <= t
};

__device__ __forceinline__ uint32_t edt_cost(const uint16_t* g, int x, int c) {
  const uint32_t gv = g[c], d = (uint32_t)(x > c ? x - c : c - x);
  return d * d + (gv == kEdtNoG ? kEdtNoneCost : gv * gv);
}

// The candidates of column x at step h (h = 0: the two end columns, solved first, x = 0 over the whole row and
// x = W - 1 from a(0) on): between its solved neighbours' arg-mins (a(W - 1) where x + h lies outside the row), and
// no farther from x than its own column's site.  0 <= lo, hi <= W - 1.
template <class L>
__device__ __forceinline__ void edt_range(const L& s, int x, int h, int W, int& lo, int& hi) {
  lo = h ? (int)s.arg[x - h] : (x ? (int)s.arg[0] : 0);
  hi = h ? (int)s.arg[x + h < W ? x + h : W - 1] : W - 1;
  const int gx = s.g[x];
  if (gx != (int)kEdtNoG) lo = max(lo, x - gx), hi = min(hi, x + gx);
}

// One level: the queries x = x0 + 2 h q, q < nq, but for the last column, which is solved before the levels.
// Ends with a barrier.
template <class L>
__device__ __forceinline__ void edt_level(L& s, int x0, int h, int nq, int lv, int W) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int q = tid; q < nq; q += kEdtRowThreads) {
    const int x = x0 + 2 * h * q;
    if (h && x == W - 1) continue;
    int lo, hi;
    edt_range(s, x, h, W, lo, hi);
    if (hi - lo >= kEdtLong) {
      const uint32_t i = atomicAdd(&s.nlong[lv], 1u);
      if (i < (uint32_t)kEdtList) {
        s.list[i] = (uint16_t)x;
        continue;
      }
    }
    uint32_t best = 0xFFFFFFFFu;
    int bi = lo;
    for (int c = lo; c <= hi; ++c) {
      const uint32_t v = edt_cost(s.g, x, c);
      if (v < best) best = v, bi = c;  // strict: the leftmost minimum
    }
    s.arg[x] = (uint16_t)bi;
  }
  __syncthreads();
  const int n = (int)min(s.nlong[lv], (uint32_t)kEdtList);
  for (int i = wave; i < n; i += kEdtRowThreads / 64) {
    const int x = s.list[i];
    int lo, hi;
    edt_range(s, x, h, W, lo, hi);
    uint32_t best = 0xFFFFFFFFu;
    int bi = lo;
#pragma unroll 4
    for (int c = lo + lane; c <= hi; c += 64) {
      const uint32_t v = edt_cost(s.g, x, c);
      if (v < best) best = v, bi = c;
    }
    unsigned long long key = ((unsigned long long)best << 16) | (unsigned long long)(uint32_t)bi;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long other = __shfl_xor(key, off);
      key = other < key ? other : key;
    }
    if (lane == 0) s.arg[x] = (uint16_t)(key & 0xFFFFu);
  }
  __syncthreads();
}

__device__ __forceinline__ uint32_t edt_isqrt255(uint32_t d2) {
  if (d2 >= 255u * 255u) return 255u;
  uint32_t r = (uint32_t)sqrtf((float)d2);
  r -= r * r > d2 ? 1u : 0u;
  r += (r + 1u) * (r + 1u) <= d2 ? 1u : 0u;
  return r;
}

// MODE 0: int32 d2, 1: u8 floor(sqrt), 2: u8 mask
template <int WMAX, int MODE>
__global__ __launch_bounds__(kEdtRowThreads) void k_edt_row(EdtRowArgs a) {
  __shared__ EdtRowLds<WMAX> s;
  const int tid = threadIdx.x, W = a.W;
  const int64_t y = blockIdx.x;
  {
    const uint2* gr = reinterpret_cast<const uint2*>(a.g + y * a.gp);
    uint2* gl = reinterpret_cast<uint2*>(s.g);
    for (int i = tid; i < (int)(a.gp >> 2); i += kEdtRowThreads) gl[i] = gr[i];
    if (tid < kEdtCounters) s.nlong[tid] = 0;
  }
  __syncthreads();
  edt_level(s, 0, 0, 1, 0, W);
  // a row without any site (then the frame has none): nothing to solve
  const bool none_row = edt_cost(s.g, 0, s.arg[0]) >= kEdtNoneCost;
  if (!none_row) {
    edt_level(s, W - 1, 0, W > 1 ? 1 : 0, 1, W);
    int lv = 2;
    for (int h = a.P >> 1; h >= 1; h >>= 1, ++lv) {
      const int nq = W > h ? (W - h - 1) / (2 * h) + 1 : 0;
      edt_level(s, h, h, nq, lv, W);
    }
  }
  for (int x = tid; x < W; x += kEdtRowThreads) {
    const uint32_t v = none_row ? kEdtNoneCost : edt_cost(s.g, x, s.arg[x]);
    const int32_t d2 = v >= kEdtNoneCost ? INT32_MAX : (int32_t)v;
    if (MODE == 0)
      static_cast<int32_t*>(a.dst)[y * a.dp + x] = d2;
    else if (MODE == 1)
      static_cast<uint8_t*>(a.dst)[y * a.dp + x] = (uint8_t)edt_isqrt255((uint32_t)d2);
    else
      static_cast<uint8_t*>(a.dst)[y * a.dp + x] = (d2 > a.t) == (a.above != 0) ? 255 : 0;
  }
}

}  // namespace dev

namespace {

constexpr size_t kAlign = 256;
size_t aligned(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

// Per device, stream, W and H: work queued on one stream runs in order, so two calls never use one buffer at a
// time.  The lock is held while a call enqueues, so that no buffer is freed between its lookup and its launches
// (hipFree waits for the device).
struct EdtScratch {
  std::array<int64_t, 4> key{};  // device, stream, W, H
  uint8_t* d = nullptr;          // g, site words, carries
  uint8_t* mask = nullptr;       // open / close: the first operation's result, on demand
};
constexpr size_t kMaxScratch = 4;
std::mutex g_edt_mu;
std::list<EdtScratch>& edt_cache() {
  static std::list<EdtScratch>* cache = new std::list<EdtScratch>;  // never destroyed before the runtime
  return *cache;
}

int64_t edt_gp(int W) { return div_up(W, 4) * 4; }
int edt_nb(int H) { return (int)div_up(H, kEdtBand); }

EdtScratch& edt_scratch(int W, int H, hipStream_t s, bool need_mask) {
  std::list<EdtScratch>& cache = edt_cache();
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  const std::array<int64_t, 4> key{dev, (int64_t) reinterpret_cast<intptr_t>(s), W, H};
  auto hit = cache.end();
  for (auto it = cache.begin(); it != cache.end(); ++it)
    if (it->key == key) hit = it;
  if (hit != cache.end()) {
    cache.splice(cache.begin(), cache, hit);
  } else {
    while (cache.size() >= kMaxScratch) {
      (void)hipFree(cache.back().d);
      (void)hipFree(cache.back().mask);
      cache.pop_back();
    }
    EdtScratch t;
    t.key = key;
    const size_t gp = (size_t)edt_gp(W), nb = (size_t)edt_nb(H);
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t.d),
                        aligned((size_t)H * gp * 2) + aligned(nb * gp * 8) + 2 * aligned(nb * gp * 2)));
    cache.push_front(t);
  }
  EdtScratch& e = cache.front();
  if (need_mask && !e.mask) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e.mask), (size_t)H * (size_t)edt_gp(W)));
  return e;
}

template <int WMAX>
void launch_row(const dev::EdtRowArgs& r, int mode, hipStream_t s) {
  const dim3 grid((unsigned)r.H), block(kEdtRowThreads);
  if (mode == (int)DistanceMode::Squared)
    dev::k_edt_row<WMAX, 0><<<grid, block, 0, s>>>(r);
  else if (mode == (int)DistanceMode::U8)
    dev::k_edt_row<WMAX, 1><<<grid, block, 0, s>>>(r);
  else
    dev::k_edt_row<WMAX, 2><<<grid, block, 0, s>>>(r);
  HIP_CHECK(hipGetLastError());
}

// the passes of one transform; the caller holds g_edt_mu
void enqueue_distance(const DistanceLaunch& L, EdtScratch& e, hipStream_t s) {
  const int W = L.W, H = L.H;
  const size_t gp = (size_t)edt_gp(W), nb = (size_t)edt_nb(H);
  dev::EdtArgs a{};
  a.src = L.src, a.sp = L.src_pitch;
  uint8_t* p = e.d;
  a.g = reinterpret_cast<uint16_t*>(p), p += aligned((size_t)H * gp * 2);
  a.bits = reinterpret_cast<unsigned long long*>(p), p += aligned(nb * gp * 8);
  a.above = reinterpret_cast<uint16_t*>(p), p += aligned(nb * gp * 2);
  a.below = reinterpret_cast<uint16_t*>(p);
  a.gp = (int64_t)gp;
  a.W = W, a.H = H, a.nb = (int)nb;
  a.inv = L.to_foreground ? 0u : 0xFu;
  const dim3 block(dev::kNT), bands((unsigned)div_up(W, 4 * dev::kNT), (unsigned)nb);
  const bool al = ((reinterpret_cast<uintptr_t>(L.src) | (uintptr_t)L.src_pitch) & 3) == 0;
  if (al)
    dev::k_edt_bits<true><<<bands, block, 0, s>>>(a);
  else
    dev::k_edt_bits<false><<<bands, block, 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
  dev::k_edt_carry<<<dim3((unsigned)div_up((int64_t)gp, dev::kNT)), block, 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
  dev::k_edt_band<<<bands, block, 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
  dev::EdtRowArgs r{};
  r.g = a.g, r.gp = a.gp;
  r.dst = L.dst, r.dp = L.dst_pitch;
  r.W = W, r.H = H;
  r.P = 1;
  while (r.P < W) r.P <<= 1;
  r.t = (int32_t)L.t;
  r.above = L.mode == (int)DistanceMode::MaskAbove;
  switch (edt_width_class(W)) {
    case 0: launch_row<kEdtWidths[0]>(r, L.mode, s); break;
    case 1: launch_row<kEdtWidths[1]>(r, L.mode, s); break;
    default: launch_row<kEdtWidths[2]>(r, L.mode, s); break;
  }
}

}  // namespace

void launch_distance_kernels(const DistanceLaunch& L, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_edt_mu);
  enqueue_distance(L, edt_scratch(L.W, L.H, s, false), s);
}

void launch_disk_morph_kernels(const DistanceLaunch& L, int op, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_edt_mu);
  const bool two = op == (int)DiskOp::Open || op == (int)DiskOp::Close;
  EdtScratch& e = edt_scratch(L.W, L.H, s, two);
  // erode: d2 to the background > t; dilate: d2 to the foreground <= t
  const auto step = [&](bool dilate, const uint8_t* src, int64_t sp, void* dst, int64_t dp) {
    DistanceLaunch M = L;
    M.src = src, M.src_pitch = sp, M.dst = dst, M.dst_pitch = dp;
    M.to_foreground = dilate;
    M.mode = (int)(dilate ? DistanceMode::MaskWithin : DistanceMode::MaskAbove);
    enqueue_distance(M, e, s);
  };
  const bool first_dilates = op == (int)DiskOp::Dilate || op == (int)DiskOp::Close;
  if (!two) {
    step(first_dilates, L.src, L.src_pitch, L.dst, L.dst_pitch);
    return;
  }
  const int64_t mp = edt_gp(L.W);
  step(first_dilates, L.src, L.src_pitch, e.mask, mp);
  step(!first_dilates, e.mask, mp, L.dst, L.dst_pitch);
}

void distance_release_scratch() {
  std::lock_guard<std::mutex> lk(g_edt_mu);
  for (EdtScratch& e : edt_cache()) {
    (void)hipFree(e.d);
    (void)hipFree(e.mask);
  }
  edt_cache().clear();
}

void distance_device(const uint8_t* src, int64_t src_pitch, int W, int H, bool to_foreground, int mode, int64_t t,
                     void* dst, int64_t dst_pitch, hipStream_t s) {
  DistanceLaunch L;
  L.src = src, L.src_pitch = src_pitch;
  L.W = W, L.H = H, L.to_foreground = to_foreground;
  L.mode = mode, L.t = t;
  L.dst = dst, L.dst_pitch = dst_pitch;
  launch_distance(L, s);
}

void disk_morph_device(const uint8_t* src, int64_t src_pitch, int W, int H, int op, int64_t t, uint8_t* dst,
                       int64_t dst_pitch, hipStream_t s) {
  DistanceLaunch L;
  L.src = src, L.src_pitch = src_pitch;
  L.W = W, L.H = H;
  L.mode = (int)DistanceMode::MaskAbove, L.t = t;
  L.dst = dst, L.dst_pitch = dst_pitch;
  launch_disk_morph(L, op, s);
}

}  // namespace stripe
