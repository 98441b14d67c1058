// Affine warp of a whole frame (k_warp): rotation by any angle and warpAffine.
// The rule is stripe/warp.h's; the kernel is bit-identical to golden_warp.
//
// A workgroup owns a destination tile of kWarpTile x kWarpTile pixels.  A lane
// computes four neighbouring pixels of a destination row (16 lanes a row, 16
// rows a step, four steps) and stores them as one (gray) or three (RGB)
// dwords, so a row of the tile is stored contiguously.  Two instances:
//
//   * staged.  The map is affine, so the source coordinates of the tile's
//     pixels lie between the minimum and the maximum over its four corners,
//     which the workgroup evaluates exactly (int64, scalar).  The box of taps
//     that follows from them (+ 1 for bilinear's second tap) is clamped to the
//     frame and staged in LDS: every row of the box in 16-byte groups from its
//     own first byte (whatever its alignment in memory; four dword stores in
//     LDS, whose row pitch is an odd number of dwords), and the last n mod 16
//     bytes a byte a lane, so nothing outside the box's bytes is read and no
//     alignment of pointers or pitches is assumed.  All of a lane's loads are
//     issued before its first store waits.
//     After one barrier every lane gathers its pixels' taps from LDS.
//     Coordinates are kept relative to the box's first pixel, where they fit
//     32 bits.  A tile whose box lies inside the frame (nearly all of them)
//     gathers without border tests; elsewhere a tap outside the frame is
//     resolved at gather time: the fill byte, or the clamped pixel, which the
//     clamped box holds.  A tile whose box misses the frame under `constant`
//     stores the fill byte without loading.
//   * direct.  Any map whose box can exceed kWarpBox pixels a side (the host
//     decides from A alone: warp_plan_staged) loads every tap from global
//     memory, a byte at a time, with the map evaluated in int64 per pixel.
//
// Stores bypass the caches (nt) when source + destination exceed the Infinity
// Cache (policy::Family::Warp).
#include "dev_common.h"
#include "stripe/kernels.h"
#include "stripe/warp.h"

namespace stripe {
namespace dev {

struct WarpArgs {
  const uint8_t* src;
  uint8_t* dst;
  int64_t sp, dp;  // pitches
  int64_t B0, B1;
  int A00, A01, A10, A11;
  int W, H;    // source, pixels
  int W2, H2;  // destination, pixels
  int ntx;     // tiles per destination row
  uint32_t fill;
};

typedef uint32_t u32x4w __attribute__((ext_vector_type(4)));
typedef u32x4w u32x4w_unaligned __attribute__((aligned(1)));
typedef uint32_t u32w_unaligned __attribute__((aligned(1)));
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) uint8_t lds_u8;

__device__ __forceinline__ int64_t min0(int64_t v) { return v < 0 ? v : 0; }
__device__ __forceinline__ int64_t max0(int64_t v) { return v > 0 ? v : 0; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int C, bool BIL, bool REP, bool STAGED, bool NT>
__global__ __launch_bounds__(kNT) void k_warp(WarpArgs a) {
  constexpr int T = kWarpTile;
  constexpr int RND = BIL ? 1 << 15 : 1 << 23;  // added before the shift to the Q8 position / the index
  constexpr int RB = warp_row_bytes(C);
  uint8_t* lb = nullptr;
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % a.ntx, by = blockIdx.x / a.ntx;
  const int X0 = bx * T, Y0 = by * T;
  const int nx = min(T, a.W2 - X0), ny = min(T, a.H2 - Y0);
  // source coordinates of the tile's first pixel
  const int64_t sx0 = (int64_t)a.A00 * X0 + (int64_t)a.A01 * Y0 + a.B0;
  const int64_t sy0 = (int64_t)a.A10 * X0 + (int64_t)a.A11 * Y0 + a.B1;

  int bx0 = 0, by0 = 0, cx0 = 0, cy0 = 0;
  uint32_t relx0 = 0, rely0 = 0;
  bool inside = false;  // every tap of the tile lies inside the frame
  if constexpr (STAGED) {
    __shared__ uint32_t box[kWarpBox * RB / 4];
    lb = reinterpret_cast<uint8_t*>(box);
    // the box: the extremes of an affine map over a rectangle are at its corners
    const int64_t exx = (int64_t)a.A00 * (nx - 1), exy = (int64_t)a.A01 * (ny - 1);
    const int64_t eyx = (int64_t)a.A10 * (nx - 1), eyy = (int64_t)a.A11 * (ny - 1);
    bx0 = (int)((sx0 + min0(exx) + min0(exy) + RND) >> 24);
    by0 = (int)((sy0 + min0(eyx) + min0(eyy) + RND) >> 24);
    const int bx1 = (int)((sx0 + max0(exx) + max0(exy) + RND) >> 24) + (BIL ? 1 : 0);
    const int by1 = (int)((sy0 + max0(eyx) + max0(eyy) + RND) >> 24) + (BIL ? 1 : 0);
    relx0 = (uint32_t)(sx0 - ((int64_t)bx0 << 24)) + (uint32_t)RND;
    rely0 = (uint32_t)(sy0 - ((int64_t)by0 << 24)) + (uint32_t)RND;
    const bool miss = bx1 < 0 || by1 < 0 || bx0 >= a.W || by0 >= a.H;
    inside = bx0 >= 0 && by0 >= 0 && bx1 < a.W && by1 < a.H;
    cx0 = clampi(bx0, 0, a.W - 1), cy0 = clampi(by0, 0, a.H - 1);
    const int ncols = min(clampi(bx1, 0, a.W - 1) - cx0 + 1, kWarpBox);
    const int nrows = min(clampi(by1, 0, a.H - 1) - cy0 + 1, kWarpBox);
    if (REP || !miss) {
      const uint8_t* s0 = a.src + (int64_t)cy0 * a.sp + (int64_t)cx0 * C;
      const int n = ncols * C;             // bytes of a staged row, <= RB
      const int nb = n >> 4, nt = n & 15;  // whole 16-byte groups, bytes behind them
      // Every load of a batch is issued before the first store waits for one: the tail bytes of all rows
      // (16 lanes a row), then the groups, a batch of kGB per lane at a time.
      constexpr int kTB = (kWarpBox * 16 + kNT - 1) / kNT, kGB = 6;
      uint32_t tv[kTB];
      int to[kTB];
#pragma unroll
      for (int u = 0; u < kTB; ++u) {
        const int it = tid + u * kNT, i = it >> 4, k = 16 * nb + (it & 15);
        to[u] = i < nrows && k < n ? i * RB + k : -1;
        tv[u] = to[u] >= 0 ? (uint32_t)s0[(int64_t)i * a.sp + k] : 0u;
      }
      // a row's groups take 8, 16 or 32 lanes, whichever holds them
      const int sh = nb <= 8 ? 3 : nb <= 16 ? 4 : 5;
      for (int base = tid; base < (nrows << sh); base += kGB * kNT) {
        u32x4w gv[kGB];
        int go[kGB];
#pragma unroll
        for (int u = 0; u < kGB; ++u) {
          const int it = base + u * kNT, i = it >> sh, g = it & ((1 << sh) - 1);
          go[u] = i < nrows && g < nb ? i * RB + 16 * g : -1;
          if (go[u] >= 0) gv[u] = *reinterpret_cast<const u32x4w_unaligned*>(s0 + (int64_t)i * a.sp + 16 * g);
        }
#pragma unroll
        for (int u = 0; u < kGB; ++u)
          if (go[u] >= 0) {
            // dword stores: a row's pitch is an odd number of dwords, so a group is only dword-aligned in LDS
            // (volatile: merged into one 16-byte store they would be replayed at every misaligned group)
            volatile lds_u32* lp = (volatile lds_u32*)(lb + go[u]);
            lp[0] = gv[u].x, lp[1] = gv[u].y, lp[2] = gv[u].z, lp[3] = gv[u].w;
          }
      }
#pragma unroll
      for (int u = 0; u < kTB; ++u)
        if (to[u] >= 0) lb[to[u]] = (uint8_t)tv[u];
    }
    __syncthreads();
  }

  const int x4 = 4 * (tid & 15);
  if (x4 >= nx) return;
  const bool whole = x4 + 4 <= nx;
  // The box is bounded from the tile's own nx x ny pixels: a lane whose four pixels straddle the tile's
  // last column also computes pixels beyond it (they are not stored), whose coordinates can leave the
  // box.  Every LDS offset is therefore clamped to the last one a tap of the box can have (an unsigned
  // minimum: an offset below the box wraps to a large one).
  constexpr uint32_t kLastTap = BIL ? kWarpBox * RB - RB - 2 * C : kWarpBox * RB - C;
  for (int yy = tid >> 4; yy < ny; yy += kNT / 16) {
    uint32_t ob[4 * C];
    if (STAGED && inside) {
      // every tap of the tile is inside the frame (and the box starts at its own first tap): no border tests
      uint32_t rx = relx0 + (uint32_t)a.A00 * (uint32_t)x4 + (uint32_t)a.A01 * (uint32_t)yy;
      uint32_t ry = rely0 + (uint32_t)a.A10 * (uint32_t)x4 + (uint32_t)a.A11 * (uint32_t)yy;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j > 0) rx += (uint32_t)a.A00, ry += (uint32_t)a.A10;
        // (volatile: byte reads stay byte reads; a merged 2-byte read at an odd address is replayed)
        const volatile lds_u8* q = (const volatile lds_u8*)(lb + min((ry >> 24) * RB + (rx >> 24) * C, kLastTap));
        const uint32_t fx = (rx >> 16) & 255u, fy = (ry >> 16) & 255u;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          if constexpr (BIL) ob[j * C + ch] = warp_bilinear(q[ch], q[C + ch], q[RB + ch], q[RB + C + ch], fx, fy);
          else ob[j * C + ch] = q[ch];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int dx = x4 + j;
        int ix, iy;
        uint32_t fx = 0, fy = 0;
        if constexpr (STAGED) {
          // relative to the box's first pixel every coordinate of the tile fits 32 bits
          const int rx = (int)(relx0 + (uint32_t)a.A00 * (uint32_t)dx + (uint32_t)a.A01 * (uint32_t)yy);
          const int ry = (int)(rely0 + (uint32_t)a.A10 * (uint32_t)dx + (uint32_t)a.A11 * (uint32_t)yy);
          ix = bx0 + (rx >> 24), iy = by0 + (ry >> 24);
          if constexpr (BIL) fx = (uint32_t)(rx >> 16) & 255u, fy = (uint32_t)(ry >> 16) & 255u;
        } else {
          const int64_t sx = sx0 + (int64_t)a.A00 * dx + (int64_t)a.A01 * yy + RND;
          const int64_t sy = sy0 + (int64_t)a.A10 * dx + (int64_t)a.A11 * yy + RND;
          ix = (int)(sx >> 24), iy = (int)(sy >> 24);
          if constexpr (BIL) fx = (uint32_t)(sx >> 16) & 255u, fy = (uint32_t)(sy >> 16) & 255u;
        }
        // the taps: (iy + ty, ix + tx); `ok`: inside the frame (replicate: clamped into it)
        constexpr int NTAP = BIL ? 2 : 1;
        int colx[NTAP], rowy[NTAP];
        bool okx[NTAP], oky[NTAP];
#pragma unroll
        for (int t = 0; t < NTAP; ++t) {
          int gx = ix + t, gy = iy + t;
          if constexpr (REP) {
            gx = clampi(gx, 0, a.W - 1), gy = clampi(gy, 0, a.H - 1);
            okx[t] = oky[t] = true;
          } else {
            okx[t] = (unsigned)gx < (unsigned)a.W, oky[t] = (unsigned)gy < (unsigned)a.H;
          }
          colx[t] = gx, rowy[t] = gy;
        }
        uint32_t p[NTAP][NTAP][C];
#pragma unroll
        for (int ty = 0; ty < NTAP; ++ty)
#pragma unroll
          for (int tx = 0; tx < NTAP; ++tx) {
            const bool ok = okx[tx] && oky[ty];
            const uint8_t* q = STAGED ? lb + min((uint32_t)((rowy[ty] - cy0) * RB + (colx[tx] - cx0) * C),
                                                 (uint32_t)(kWarpBox * RB - C))
                                      : a.src + (int64_t)rowy[ty] * a.sp + (int64_t)colx[tx] * C;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) p[ty][tx][ch] = ok ? (uint32_t)q[ch] : a.fill;
          }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          if constexpr (BIL) ob[j * C + ch] = warp_bilinear(p[0][0][ch], p[0][1][ch], p[1][0][ch], p[1][1][ch], fx, fy);
          else ob[j * C + ch] = p[0][0][ch];
        }
      }
    }
    uint8_t* dp = a.dst + (int64_t)(Y0 + yy) * a.dp + (int64_t)(X0 + x4) * C;
    if (whole) {
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const uint32_t v4 = pack4(ob[4 * k], ob[4 * k + 1], ob[4 * k + 2], ob[4 * k + 3]);
        if constexpr (NT) __builtin_nontemporal_store(v4, reinterpret_cast<u32w_unaligned*>(dp + 4 * k));
        else *reinterpret_cast<u32w_unaligned*>(dp + 4 * k) = v4;
      }
    } else {  // the row's last 1..3 pixels
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (x4 + j < nx) {
#pragma unroll
          for (int ch = 0; ch < C; ++ch) dp[j * C + ch] = (uint8_t)ob[j * C + ch];
        }
    }
  }
}

}  // namespace dev

namespace {
template <int C, bool BIL, bool REP>
void launch_inst(bool staged, bool nt, const dev::WarpArgs& a, unsigned grid, hipStream_t s) {
  if (staged) {
    if (nt) dev::k_warp<C, BIL, REP, true, true><<<grid, dev::kNT, 0, s>>>(a);
    else dev::k_warp<C, BIL, REP, true, false><<<grid, dev::kNT, 0, s>>>(a);
  } else {
    if (nt) dev::k_warp<C, BIL, REP, false, true><<<grid, dev::kNT, 0, s>>>(a);
    else dev::k_warp<C, BIL, REP, false, false><<<grid, dev::kNT, 0, s>>>(a);
  }
}
template <int C>
void launch_c(bool bil, bool rep, bool staged, bool nt, const dev::WarpArgs& a, unsigned grid, hipStream_t s) {
  if (bil) {
    if (rep) launch_inst<C, true, true>(staged, nt, a, grid, s);
    else launch_inst<C, true, false>(staged, nt, a, grid, s);
  } else {
    if (rep) launch_inst<C, false, true>(staged, nt, a, grid, s);
    else launch_inst<C, false, false>(staged, nt, a, grid, s);
  }
}
}  // namespace

void launch_warp_kernel(const WarpLaunch& L, hipStream_t s) {
  const WarpMap& m = L.map;
  dev::WarpArgs a{};
  a.src = L.src;
  a.dst = L.dst;
  a.sp = L.src_pitch;
  a.dp = L.dst_pitch;
  a.B0 = m.B[0], a.B1 = m.B[1];
  a.A00 = m.A[0][0], a.A01 = m.A[0][1], a.A10 = m.A[1][0], a.A11 = m.A[1][1];
  a.W = L.W, a.H = L.H;
  a.W2 = m.W2, a.H2 = m.H2;
  a.fill = m.fill;
  a.ntx = (int)div_up(m.W2, kWarpTile);
  const int64_t nwg = a.ntx * div_up(m.H2, kWarpTile);
  STRIPE_CHECK(nwg < (int64_t(1) << 31), "warp: too many workgroups");
  policy::PolicyIn pin{policy::Family::Warp};
  pin.cin = pin.cout = pin.cmid = L.C;
  pin.W = L.W, pin.rows = L.H;
  pin.W2 = m.W2, pin.rows2 = m.H2;
  const bool nt = policy::stream_policy(pin).nt_stores;
  const bool bil = m.mode == WarpMode::Bilinear, rep = m.border == WarpBorder::Replicate;
  const bool staged = warp_plan_staged(m);
  if (L.C == 1) launch_c<1>(bil, rep, staged, nt, a, (unsigned)nwg, s);
  else launch_c<3>(bil, rep, staged, nt, a, (unsigned)nwg, s);
  HIP_CHECK(hipGetLastError());
}

void warp_device(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch,
                 const WarpMap& map, hipStream_t s) {
  WarpLaunch L;
  L.src = src;
  L.src_pitch = src_pitch;
  L.W = W, L.H = H, L.C = C;
  L.dst = dst;
  L.dst_pitch = dst_pitch;
  L.map = map;
  launch_warp(L, s);
}

}  // namespace stripe
