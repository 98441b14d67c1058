// Resize of a whole frame: nearest, bilinear and area scaling (k_resize).
//
// The rule is stripe/resize.h's: the kernel consumes the integer tap tables of
// resize_taps() and is bit-identical to golden_resize.  Horizontal first (to
// 8.8 fixed point), then vertical.
//
// A workgroup owns a tile of `tile` output bytes (4 per thread, one dword
// store each) in a band of kResizeBand output rows.  It walks the source rows
// its band reads, in order.  Per source row:
//   * the byte span the tile's pixels read goes to LDS: a head of single
//     bytes up to the first 16-byte boundary of the row's address, whole
//     16-byte groups (every lane of a wave on a contiguous run), a tail of
//     single bytes.  Nothing outside the span is read, so nothing outside
//     [src, src + (H - 1) pitch + W C) is; base pointers and pitches need no
//     alignment (the LDS image keeps the row's own misalignment so that
//     16-byte global groups are 16-byte LDS groups);
//   * each thread reduces its four output bytes from LDS with its
//     loop-invariant x-taps: in registers when no pixel has more than two
//     (XS), from an LDS copy of the tile's weights otherwise.
// The vertical pass keeps the two most recent h' rows in registers (two u16
// per dword): a bilinear or nearest axis finds both rows of every output row
// between two source rows there, an area axis the one row adjacent cells
// share.  The source row index is uniform over the workgroup, so "need a new
// row?" is a scalar branch.  Everything is u16 x u16 -> u32 multiply-adds.
//
// Stores bypass the caches (nt) when source + destination exceed the Infinity
// Cache (policy::Family::Resize).
#include <array>
#include <list>
#include <mutex>
#include <vector>

#include "dev_common.h"
#include "stripe/kernels.h"
#include "stripe/resize.h"

namespace stripe {
namespace dev {

struct ResizeArgs {
  const uint8_t* src;
  uint8_t* dst;
  int64_t src_pitch, dst_pitch;
  const int32_t *fx, *ox, *fy, *oy;
  const uint16_t *wx, *wy;
  int E2;    // destination row bytes
  int H2;
  int tile;  // output bytes per workgroup, a multiple of 4
  int ntx;   // tiles per row
};

typedef uint32_t u32x4r __attribute__((ext_vector_type(4)));
typedef uint32_t u32_unaligned __attribute__((aligned(1)));

template <int C, bool XS, int SRCB, int WN, bool NT>
__global__ __launch_bounds__(kNT) void k_resize(ResizeArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t srow[SRCB];
  __shared__ uint16_t wl[WN > 0 ? WN : 1];
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % a.ntx, by = blockIdx.x / a.ntx;
  // the tile's output bytes [ob0, obe) and the source bytes [x0, x1) they read
  // (first and first + count are non-decreasing: resize_taps checks it)
  const int ob0 = bx * a.tile;
  const int obe = min(ob0 + a.tile, a.E2);
  const int px0 = ob0 / C, px1 = (obe - 1) / C;
  const int x0 = a.fx[px0] * C;
  const int n = (a.fx[px1] + a.ox[px1 + 1] - a.ox[px1]) * C - x0;
  const int wbase = a.ox[px0];

  // this thread's four output bytes and their x-taps
  const int ob = ob0 + 4 * tid;
  const bool active = ob < obe;
  int li[4];        // LDS index of the first tap (before the row's misalignment)
  int cnt[4];       // taps (!XS)
  int wo[4];        // first weight in wl (!XS)
  uint32_t w01[4];  // XS: w0 | w1 << 16
  int l1[4];        // XS: LDS index of the second tap
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int b = min(ob + j, obe - 1);  // bytes past the tile repeat its last one (not stored)
    const int px = b / C, ch = b - px * C;
    const int f = a.fx[px], o = a.ox[px], c = a.ox[px + 1] - o;
    li[j] = active ? f * C + ch - x0 : 0;
    if constexpr (XS) {
      const uint32_t w0 = a.wx[o], w1 = c > 1 ? a.wx[o + 1] : 0u;
      w01[j] = active ? (w0 | (w1 << 16)) : 0u;
      l1[j] = c > 1 ? li[j] + C : li[j];
    } else {
      cnt[j] = active ? c : 0;
      wo[j] = o - wbase;
    }
  }
  if constexpr (!XS) {
    const int nw = a.ox[px1 + 1] - wbase;  // <= WN (resize_tile_plan)
    for (int i = tid; i < nw; i += kNT) wl[i] = a.wx[wbase + i];
  }

  // h' of source row sy for this thread's bytes: (0 | 1 << 16), (2 | 3 << 16)
  auto hrow = [&](int sy, uint32_t& ha, uint32_t& hb) {
    __syncthreads();  // the previous row's reads are done
    const uint8_t* rp = a.src + (int64_t)sy * a.src_pitch + x0;
    const int mis = (int)((uintptr_t)rp & 15);
    const int head = min(n, (16 - mis) & 15);
    if (tid < head) srow[mis + tid] = rp[tid];
    const int nbody = (n - head) >> 4;  // whole 16-byte groups, aligned in memory and in LDS
    for (int g = tid; g < nbody; g += kNT)
      *reinterpret_cast<u32x4r*>(srow + mis + head + 16 * g) =
          *reinterpret_cast<const u32x4r*>(rp + head + 16 * (int64_t)g);
    const int t0 = head + 16 * nbody;
    if (tid < n - t0) srow[mis + t0 + tid] = rp[t0 + tid];
    __syncthreads();
    uint32_t h[4];
    const uint8_t* sp = srow + mis;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t s;
      if constexpr (XS) {
        s = (w01[j] & 0xFFFFu) * sp[li[j]] + (w01[j] >> 16) * sp[l1[j]];
      } else {
        s = 0;
        const uint8_t* p = sp + li[j];
        const uint16_t* w = wl + wo[j];
        for (int u = 0; u < cnt[j]; ++u) s += (uint32_t)w[u] * p[u * C];
      }
      h[j] = (s + 64u) >> 7;
    }
    ha = h[0] | (h[1] << 16);
    hb = h[2] | (h[3] << 16);
  };

  const int oy0 = by * kResizeBand, oy1 = min(oy0 + kResizeBand, a.H2);
  int r0 = -1, r1 = -1, mru = 1;  // the cached rows and which was used last
  uint32_t c0a = 0, c0b = 0, c1a = 0, c1b = 0;
  for (int oy = oy0; oy < oy1; ++oy) {
    const int f = a.fy[oy], wo_y = a.oy[oy], ny = a.oy[oy + 1] - wo_y;
    uint32_t acc[4] = {0, 0, 0, 0};
    for (int v = 0; v < ny; ++v) {
      const int sy = f + v;
      const uint32_t w = a.wy[wo_y + v];
      uint32_t ha, hb;
      if (sy == r0) {
        ha = c0a, hb = c0b, mru = 0;
      } else if (sy == r1) {
        ha = c1a, hb = c1b, mru = 1;
      } else {
        hrow(sy, ha, hb);
        if (mru == 0) c1a = ha, c1b = hb, r1 = sy, mru = 1;
        else c0a = ha, c0b = hb, r0 = sy, mru = 0;
      }
      acc[0] += w * (ha & 0xFFFFu);
      acc[1] += w * (ha >> 16);
      acc[2] += w * (hb & 0xFFFFu);
      acc[3] += w * (hb >> 16);
    }
    if (!active) continue;
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (acc[j] + (1u << 22)) >> 23;
    uint8_t* dp = a.dst + (int64_t)oy * a.dst_pitch + ob;
    if (ob + 4 <= obe) {
      const uint32_t v4 = pack4(o[0], o[1], o[2], o[3]);
      if constexpr (NT) __builtin_nontemporal_store(v4, reinterpret_cast<u32_unaligned*>(dp));
      else *reinterpret_cast<u32_unaligned*>(dp) = v4;
    } else {  // the row's last 1..3 bytes
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (ob + j < obe) dp[j] = (uint8_t)o[j];
    }
  }
}

}  // namespace dev

void resize_tile_plan(const ResizeTaps& tx, int C, ResizeLaunch* L) {
  const int E2 = tx.n_out * C;
  const bool xs = tx.max_count <= 2;
  L->max_count_x = tx.max_count;
  for (int tile = kResizeTile; tile >= 4; tile >>= 1) {
    int span = 0, nw = 0;
    for (int ob0 = 0; ob0 < E2; ob0 += tile) {
      const int px0 = ob0 / C, px1 = (std::min(ob0 + tile, E2) - 1) / C;
      span = std::max(span, (tx.first[(size_t)px1] + tx.count(px1) - tx.first[(size_t)px0]) * C);
      nw = std::max(nw, tx.offset[(size_t)px1 + 1] - tx.offset[(size_t)px0]);
    }
    for (int cls = xs ? 0 : 2; cls < (xs ? 2 : 4); ++cls) {
      if (span + 15 <= kResizeClasses[cls].src_bytes && (xs || nw <= kResizeClasses[cls].w_entries)) {
        L->tile = tile;
        L->cls = cls;
        L->max_span = span;
        L->max_weights = nw;
        return;
      }
    }
  }
  fail("resize: no tile fits the kernel's LDS");  // a 4-byte tile reads at most 2 * 33 * 3 bytes
}

namespace {
template <int C, int CLS, bool NT>
void launch_cls(const dev::ResizeArgs& a, unsigned grid, hipStream_t s) {
  constexpr bool XS = kResizeClasses[CLS].w_entries == 0;
  dev::k_resize<C, XS, kResizeClasses[CLS].src_bytes, kResizeClasses[CLS].w_entries, NT><<<grid, dev::kNT, 0, s>>>(a);
}
template <int C, bool NT>
void launch_c(int cls, const dev::ResizeArgs& a, unsigned grid, hipStream_t s) {
  switch (cls) {
    case 0: launch_cls<C, 0, NT>(a, grid, s); break;
    case 1: launch_cls<C, 1, NT>(a, grid, s); break;
    case 2: launch_cls<C, 2, NT>(a, grid, s); break;
    default: launch_cls<C, 3, NT>(a, grid, s); break;
  }
}
}  // namespace

void launch_resize_kernel(const ResizeLaunch& L, hipStream_t s) {
  dev::ResizeArgs a{};
  a.src = L.src;
  a.dst = L.dst;
  a.src_pitch = L.src_pitch;
  a.dst_pitch = L.dst_pitch;
  a.fx = L.fx, a.ox = L.ox, a.fy = L.fy, a.oy = L.oy;
  a.wx = L.wx, a.wy = L.wy;
  a.E2 = L.W2 * L.C;
  a.H2 = L.H2;
  a.tile = L.tile;
  a.ntx = (int)div_up(a.E2, L.tile);
  const int64_t nwg = (int64_t)a.ntx * div_up(L.H2, kResizeBand);
  STRIPE_CHECK(nwg < (int64_t(1) << 31), "resize: too many workgroups");
  policy::PolicyIn pin{policy::Family::Resize};
  pin.cin = pin.cout = pin.cmid = L.C;
  pin.W = L.W, pin.rows = L.H, pin.W2 = L.W2, pin.rows2 = L.H2;
  const bool nt = policy::stream_policy(pin).nt_stores;
  if (L.C == 1) {
    if (nt) launch_c<1, true>(L.cls, a, (unsigned)nwg, s);
    else launch_c<1, false>(L.cls, a, (unsigned)nwg, s);
  } else {
    if (nt) launch_c<3, true>(L.cls, a, (unsigned)nwg, s);
    else launch_c<3, false>(L.cls, a, (unsigned)nwg, s);
  }
  HIP_CHECK(hipGetLastError());
}

namespace {
// The device copy of one (W, W2, H, H2, mode) pair's tap tables, with the tile
// plan of its x tables.  Built and uploaded once (a synchronous copy: the
// host vector is pageable), then shared by every later call, so a stream of
// equal frames launches without touching the host tables again.  The least
// recently used entry is freed (hipFree waits for the device) beyond kMaxTables.
struct DevTables {
  std::array<int, 7> key{};  // device, W, W2, H, H2, mode, C
  void* d = nullptr;
  ResizeLaunch L;  // table pointers and tile plan; the views are filled per call
};
constexpr size_t kMaxTables = 16;

ResizeLaunch device_tables(int W, int W2, int H, int H2, ResizeMode mode, int C) {
  static std::mutex mu;
  static std::list<DevTables> cache;  // most recently used first; never destroyed before the runtime
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  const std::array<int, 7> key{dev, W, W2, H, H2, (int)mode, C};
  std::lock_guard<std::mutex> lk(mu);
  for (auto it = cache.begin(); it != cache.end(); ++it)
    if (it->key == key) {
      cache.splice(cache.begin(), cache, it);
      return cache.front().L;
    }
  const ResizeTaps tx = resize_taps(W, W2, mode), ty = resize_taps(H, H2, mode);
  // one buffer: [fx | ox | fy | oy] int32, then [wx | wy] u16
  const size_t ni = 2 * (size_t)W2 + 1 + 2 * (size_t)H2 + 1;
  std::vector<int32_t> host(ni + (tx.w.size() + ty.w.size() + 1) / 2);
  int32_t* p = host.data();
  p = std::copy(tx.first.begin(), tx.first.end(), p);
  p = std::copy(tx.offset.begin(), tx.offset.end(), p);
  p = std::copy(ty.first.begin(), ty.first.end(), p);
  p = std::copy(ty.offset.begin(), ty.offset.end(), p);
  uint16_t* hw = reinterpret_cast<uint16_t*>(p);
  std::copy(tx.w.begin(), tx.w.end(), hw);
  std::copy(ty.w.begin(), ty.w.end(), hw + tx.w.size());
  DevTables t;
  t.key = key;
  resize_tile_plan(tx, C, &t.L);
  while (cache.size() >= kMaxTables) {
    (void)hipFree(cache.back().d);
    cache.pop_back();
  }
  HIP_CHECK(hipMalloc(&t.d, host.size() * sizeof(int32_t)));
  if (hipError_t e = hipMemcpy(t.d, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice); e != hipSuccess) {
    (void)hipFree(t.d);
    HIP_CHECK(e);
  }
  const int32_t* di = static_cast<const int32_t*>(t.d);
  t.L.fx = di;
  t.L.ox = t.L.fx + W2;
  t.L.fy = t.L.ox + W2 + 1;
  t.L.oy = t.L.fy + H2;
  t.L.wx = reinterpret_cast<const uint16_t*>(di + ni);
  t.L.wy = t.L.wx + tx.w.size();
  cache.push_front(t);
  return cache.front().L;
}
}  // namespace

void resize_device(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch, int W2,
                   int H2, ResizeMode mode, hipStream_t s) {
  STRIPE_CHECK(C == 1 || C == 3, "resize: image must have 1 or 3 channels, got C = " << C);
  ResizeLaunch L = device_tables(W, W2, H, H2, mode, C);
  L.src = src, L.src_pitch = src_pitch, L.W = W, L.H = H, L.C = C;
  L.dst = dst, L.dst_pitch = dst_pitch, L.W2 = W2, L.H2 = H2;
  launch_resize(L, s);
}

}  // namespace stripe
