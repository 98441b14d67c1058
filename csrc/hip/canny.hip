// Canny edge detection and hysteresis thresholding on the device (k_canny_*).
// The rule is stripe/canny.h's; the class plane and the edge map are
// bit-identical to the golden functions.
//
//   k_canny_nms<L2>   one workgroup per tile of kCannyTileX x kCannyTileY pixels.
//                The source goes once into LDS with a 2-pixel apron, the border
//                applied at load time as an index map (border_index per byte;
//                a padded copy of the frame is never stored).  Then the
//                magnitudes of the tile plus a 1-pixel apron go to LDS, one u32
//                each with the sector in bits 24 and 25 (a magnitude is below
//                2^21), 0 for a position outside the frame.  After a barrier
//                every lane classifies kCannyPixels pixels in a row from its own
//                word and the two neighbours the sector names, and stores the
//                class bytes (one dword on an aligned plane, single bytes on an
//                unaligned one and at a ragged row end).
//   k_canny_classify  hysteresis_threshold's pointwise class map, a lane per
//                kCannyPixels pixels of a row.
//   (launch_ccl_forest of components.hip on the class plane: class != 0 is
//    foreground.  Afterwards every slot of the int32 plane holds 0 or its root's
//    raster index + 1.)
//   k_canny_mark      every class 2 pixel stores -(r) into the slot of its root
//                r - 1.  All writers of a slot store the same value, and a
//                reader takes |slot|, as k_ccl_resolve does, so neither the
//                order of the writers nor that of readers and writers matters.
//   k_canny_select    255 where the class is >= 1 and the root's slot is
//                negative, else 0.
//
// Every loop's trip count is a constant of the tile; the only data-dependent
// loops are the forest's, which are capped (components.hip).  A root index read
// from the plane is used as an address only when it lies in 1 .. W * H.
//
// Scratch per (device, stream, W, H), cached, released by
// canny_release_scratch: the class plane (H rows at a pitch of W rounded up to
// 4, so that its stores and loads are dwords at any W) and the forest plane
// (W * H int32, packed).  A call holds this cache's lock, and from the forest
// passes on the components' lock too, until its one host synchronisation (the
// read-back of the forest's error word).  Launch policy: default stores, no
// residency cap (none was measured; launch_policy.h has no entry for this family).
//
// Addressing as k_orient / k_sat: 64-bit on pitched views, any source pitch >= W
// at any alignment, no byte outside a source row's W bytes read, nothing outside
// a destination row's W bytes written.
#include <array>
#include <list>
#include <mutex>

#include "dev_common.h"
#include "stripe/canny.h"
#include "stripe/kernels.h"

namespace stripe {
namespace dev {

constexpr int kSectorShift = 24;
constexpr uint32_t kMagMask = (1u << kSectorShift) - 1u;

struct CannyArgs {
  const uint8_t* src;  // the frame (nms, classify)
  const uint8_t* cls;  // the class plane (mark, select)
  int32_t* lab;        // the forest plane, packed: W ints a row
  uint8_t* dst;
  int64_t sp, cp, dp;  // pitches in bytes
  int W, H, border;
  int ntx;             // workgroups per row of tiles / per row
  uint32_t lo, hi;     // what a magnitude (a pixel) is compared with
  uint32_t n;          // W * H
  int src_al, cls_al, dst_al;  // base and pitch are multiples of 4
};

// kCannyPixels = 4 bytes of a row from column x (a multiple of 4); columns >= W read as 0
__device__ __forceinline__ void load4(const uint8_t* row, int x, int W, bool al, uint32_t (&v)[4]) {
  if (al && x + 3 < W) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(row + x);
    v[0] = w & 0xFF, v[1] = (w >> 8) & 0xFF, v[2] = (w >> 16) & 0xFF, v[3] = w >> 24;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x + k < W ? (uint32_t)row[x + k] : 0u;
  }
}
__device__ __forceinline__ void store4(uint8_t* row, int x, int W, bool al, const uint32_t (&v)[4]) {
  if (al && x + 3 < W) {
    *reinterpret_cast<uint32_t*>(row + x) = pack4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x + k < W) row[x + k] = (uint8_t)v[k];
  }
}

template <bool L2>
__global__ __launch_bounds__(kNT) void k_canny_nms(CannyArgs a) {
  constexpr int TX = kCannyTileX, TY = kCannyTileY, SW = TX + 4, SH = TY + 4, MW = TX + 2, MH = TY + 2;
  static_assert(kCannyPixels == 4 && TX % 4 == 0 && (TX / 4) * TY % kNT == 0, "a lane classifies 4 pixels of a row");
  __shared__ uint8_t S[SW * SH];    // the source of the tile with a 2-pixel apron
  __shared__ uint32_t M[MW * MH];   // magnitude | sector << 24 of the tile with a 1-pixel apron
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % a.ntx, by = blockIdx.x / a.ntx;
  const int X0 = bx * TX, Y0 = by * TY;
  for (int i = tid; i < SW * SH; i += kNT) {
    const int ly = i / SW, lx = i - ly * SW;
    const int sy = border_index_dev(Y0 - 2 + ly, a.H, a.border), sx = border_index_dev(X0 - 2 + lx, a.W, a.border);
    S[i] = sy >= 0 && sx >= 0 ? a.src[(int64_t)sy * a.sp + sx] : (uint8_t)0;
  }
  __syncthreads();
  for (int i = tid; i < MW * MH; i += kNT) {
    const int my = i / MW, mx = i - my * MW;
    const int x = X0 - 1 + mx, y = Y0 - 1 + my;
    uint32_t v = 0;  // outside the frame: no gradient
    if (x >= 0 && y >= 0 && x < a.W && y < a.H) {
      const uint8_t* p = S + my * SW + mx;  // (x - 1, y - 1)
      const int p00 = p[0], p01 = p[1], p02 = p[2], p10 = p[SW], p12 = p[SW + 2], p20 = p[2 * SW], p21 = p[2 * SW + 1],
                p22 = p[2 * SW + 2];
      const int gx = (p02 + 2 * p12 + p22) - (p00 + 2 * p10 + p20), gy = (p20 + 2 * p21 + p22) - (p00 + 2 * p01 + p02);
      v = canny_magnitude(gx, gy, L2) | ((uint32_t)canny_sector(gx, gy) << kSectorShift);
    }
    M[i] = v;
  }
  __syncthreads();
  constexpr int LPR = TX / 4;  // lanes per tile row
#pragma unroll
  for (int it = 0; it < LPR * TY / kNT; ++it) {
    const int ly = it * (kNT / LPR) + tid / LPR, lx = (tid % LPR) * 4;
    const int x = X0 + lx, y = Y0 + ly;
    if (x >= a.W || y >= a.H) continue;
    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t* m = M + (ly + 1) * MW + lx + k + 1;
      const uint32_t w = *m;
      const int sec = (int)(w >> kSectorShift);
      const int d = canny_dy(sec) * MW + canny_dx(sec);
      // (a column >= W holds 0 and is not stored)
      c[k] = canny_class(w & kMagMask, *(m - d) & kMagMask, *(m + d) & kMagMask, sec, a.lo, a.hi);
    }
    store4(a.dst + (int64_t)y * a.dp, x, a.W, a.dst_al, c);
  }
}

__global__ __launch_bounds__(kNT) void k_canny_classify(CannyArgs a) {
  const int bx = blockIdx.x % a.ntx, y = blockIdx.x / a.ntx;
  const int x = (bx * kNT + (int)threadIdx.x) * 4;
  if (x >= a.W) return;
  uint32_t v[4];
  load4(a.src + (int64_t)y * a.sp, x, a.W, a.src_al, v);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = hysteresis_class(v[k], a.lo, a.hi);
  store4(a.dst + (int64_t)y * a.dp, x, a.W, a.dst_al, v);
}

// |slot| of pixel p of the packed forest plane: its root's raster index + 1 (0: background)
__device__ __forceinline__ uint32_t root_of(const CannyArgs& a, int64_t p) {
  const int32_t v = __hip_atomic_load(a.lab + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return (uint32_t)(v < 0 ? -v : v);
}

__global__ __launch_bounds__(kNT) void k_canny_mark(CannyArgs a) {
  const int bx = blockIdx.x % a.ntx, y = blockIdx.x / a.ntx;
  const int x = (bx * kNT + (int)threadIdx.x) * 4;
  if (x >= a.W) return;
  uint32_t c[4];
  load4(a.cls + (int64_t)y * a.cp, x, a.W, a.cls_al, c);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (c[k] < 2) continue;
    const uint32_t r = root_of(a, (int64_t)y * a.W + x + k);
    if (r >= 1 && r <= a.n) __hip_atomic_store(a.lab + (r - 1u), -(int32_t)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(kNT) void k_canny_select(CannyArgs a) {
  const int bx = blockIdx.x % a.ntx, y = blockIdx.x / a.ntx;
  const int x = (bx * kNT + (int)threadIdx.x) * 4;
  if (x >= a.W) return;
  uint32_t c[4];
  load4(a.cls + (int64_t)y * a.cp, x, a.W, a.cls_al, c);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t out = 0;
    if (c[k] >= 1) {
      const uint32_t r = root_of(a, (int64_t)y * a.W + x + k);
      if (r >= 1 && r <= a.n && a.lab[r - 1u] < 0) out = 255;
    }
    c[k] = out;
  }
  store4(a.dst + (int64_t)y * a.dp, x, a.W, a.dst_al, c);
}

}  // namespace dev

namespace {

// Per device, stream, W and H: the class plane and the forest plane.
struct CannyScratch {
  std::array<int64_t, 4> key{};
  uint8_t* cls = nullptr;
  int32_t* lab = nullptr;
};
constexpr size_t kMaxScratch = 4;
std::mutex g_canny_mu;
std::list<CannyScratch>& canny_cache() {
  static std::list<CannyScratch>* cache = new std::list<CannyScratch>;  // never destroyed before the runtime
  return *cache;
}

int64_t class_pitch(int W) { return align_up(W, 4); }

CannyScratch& canny_scratch(int W, int H, hipStream_t s) {
  std::list<CannyScratch>& cache = canny_cache();
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  const std::array<int64_t, 4> key{dev, (int64_t) reinterpret_cast<intptr_t>(s), W, H};
  for (auto it = cache.begin(); it != cache.end(); ++it)
    if (it->key == key) {
      cache.splice(cache.begin(), cache, it);
      return cache.front();
    }
  while (cache.size() >= kMaxScratch) {
    (void)hipFree(cache.back().cls);
    (void)hipFree(cache.back().lab);
    cache.pop_back();
  }
  CannyScratch t;
  t.key = key;
  HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t.cls), (size_t)class_pitch(W) * (size_t)H));
  if (hipMalloc(reinterpret_cast<void**>(&t.lab), (size_t)W * (size_t)H * sizeof(int32_t)) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(t.cls);
    fail("canny: no device memory for the forest plane of " + std::to_string(W) + "x" + std::to_string(H));
  }
  cache.push_front(t);
  return cache.front();
}

unsigned grid_of(int64_t n, const char* what) {
  STRIPE_CHECK(n >= 1 && n < (int64_t(1) << 31), "canny: too many workgroups (" << what << ")");
  return (unsigned)n;
}

bool aligned4(const void* p, int64_t pitch) { return ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)pitch) & 3) == 0; }

// k_canny_nms of L into dst
void enqueue_nms(const CannyLaunch& L, dev::CannyArgs a, uint8_t* dst, int64_t dp, hipStream_t s) {
  const bool l2 = L.norm == (int)CannyNorm::L2;
  a.lo = (uint32_t)(l2 ? L.low * L.low : L.low), a.hi = (uint32_t)(l2 ? L.high * L.high : L.high);
  a.dst = dst, a.dp = dp, a.dst_al = aligned4(dst, dp);
  const int64_t tx = div_up(L.W, kCannyTileX), ty = div_up(L.H, kCannyTileY);
  a.ntx = (int)tx;
  if (l2) dev::k_canny_nms<true><<<grid_of(tx * ty, "tiles"), dev::kNT, 0, s>>>(a);
  else dev::k_canny_nms<false><<<grid_of(tx * ty, "tiles"), dev::kNT, 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

void launch_canny_kernels(const CannyLaunch& L, hipStream_t s) {
  dev::CannyArgs a{};
  a.src = L.src, a.sp = L.src_pitch, a.src_al = aligned4(L.src, L.src_pitch);
  a.W = L.W, a.H = L.H, a.border = L.border;
  a.n = (uint32_t)((int64_t)L.W * L.H);
  if (L.stage == (int)CannyStage::Classes) {
    enqueue_nms(L, a, L.dst, L.dst_pitch, s);
    return;
  }
  std::lock_guard<std::mutex> lk(g_canny_mu);
  CannyScratch& e = canny_scratch(L.W, L.H, s);
  const int64_t cp = class_pitch(L.W);
  const int64_t segs = div_up(L.W, 4 * dev::kNT);
  const unsigned rows = grid_of(segs * L.H, "rows");
  if (L.stage == (int)CannyStage::Canny) {
    enqueue_nms(L, a, e.cls, cp, s);
  } else {
    dev::CannyArgs c = a;
    c.lo = (uint32_t)L.low, c.hi = (uint32_t)L.high;
    c.dst = e.cls, c.dp = cp, c.dst_al = 1;
    c.ntx = (int)segs;
    dev::k_canny_classify<<<rows, dev::kNT, 0, s>>>(c);
    HIP_CHECK(hipGetLastError());
  }
  ComponentsLaunch F;
  F.src = e.cls, F.src_pitch = cp;
  F.W = L.W, F.H = L.H, F.conn = L.stage == (int)CannyStage::Canny ? 8 : L.conn;
  F.labels = e.lab, F.labels_pitch = L.W;
  const CclForest f = launch_ccl_forest(F, s);
  a.cls = e.cls, a.cp = cp, a.cls_al = 1;
  a.lab = e.lab;
  a.dst = L.dst, a.dp = L.dst_pitch, a.dst_al = aligned4(L.dst, L.dst_pitch);
  a.ntx = (int)segs;
  dev::k_canny_mark<<<rows, dev::kNT, 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
  dev::k_canny_select<<<rows, dev::kNT, 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
  uint32_t back = 0;  // the forest's error word
  HIP_CHECK(hipMemcpyAsync(&back, f.err, sizeof(back), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  STRIPE_CHECK(back == 0, "canny: a union-find loop overran its step cap of " << f.cap
                              << " (a kernel bug; the edges are not valid)");
}

void canny_release_scratch() {
  std::lock_guard<std::mutex> lk(g_canny_mu);
  for (CannyScratch& e : canny_cache()) {
    (void)hipFree(e.cls);
    (void)hipFree(e.lab);
  }
  canny_cache().clear();
}

void canny_device(const uint8_t* src, int64_t src_pitch, int W, int H, int low, int high, int norm, int border,
                  uint8_t* dst, int64_t dst_pitch, hipStream_t s) {
  CannyLaunch L;
  L.src = src, L.src_pitch = src_pitch;
  L.W = W, L.H = H;
  L.stage = (int)CannyStage::Canny;
  L.low = low, L.high = high, L.norm = norm, L.border = border;
  L.dst = dst, L.dst_pitch = dst_pitch;
  launch_canny(L, s);
}

void canny_classes_device(const uint8_t* src, int64_t src_pitch, int W, int H, int low, int high, int norm, int border,
                          uint8_t* dst, int64_t dst_pitch, hipStream_t s) {
  CannyLaunch L;
  L.src = src, L.src_pitch = src_pitch;
  L.W = W, L.H = H;
  L.stage = (int)CannyStage::Classes;
  L.low = low, L.high = high, L.norm = norm, L.border = border;
  L.dst = dst, L.dst_pitch = dst_pitch;
  launch_canny(L, s);
}

void hysteresis_device(const uint8_t* src, int64_t src_pitch, int W, int H, int low, int high, int conn, uint8_t* dst,
                       int64_t dst_pitch, hipStream_t s) {
  CannyLaunch L;
  L.src = src, L.src_pitch = src_pitch;
  L.W = W, L.H = H;
  L.stage = (int)CannyStage::Hysteresis;
  L.low = low, L.high = high, L.conn = conn;
  L.dst = dst, L.dst_pitch = dst_pitch;
  launch_canny(L, s);
}

}  // namespace stripe
