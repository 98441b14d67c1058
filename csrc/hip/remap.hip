// Mesh warp of a whole frame (k_remap): perspective warps, lens undistortion and
// remap.  The rule is stripe/remap.h's; the kernel is bit-identical to
// golden_remap.
//
// The shape is k_warp's: a workgroup owns a destination tile of kWarpTile x
// kWarpTile pixels, a lane computes four neighbouring pixels of a destination
// row (16 lanes a row, 16 rows a step, four steps) and stores them as one (gray)
// or three (RGB) dwords.  The mesh lives on the device and the host never reads
// it, so every decision that depends on the nodes is taken per tile, by the
// workgroup (a uniform branch, no synchronisation between workgroups):
//
//   * spacing >= 4.  The tile's nodes (at most 17 x 17) go to LDS; a lane's four
//     pixels then share one cell.  A bilinear patch lies in the hull of its
//     nodes, so the minimum and maximum over the nodes (a wave reduction, then
//     four values a wave through LDS) bound the tile's source box without any
//     corner algebra.
//       - The box misses the frame under `constant`: the fill byte is stored,
//         nothing is loaded.
//       - The box has at most kWarpBox pixels a side: it is clamped to the frame
//         and staged in LDS with k_warp's loads (16-byte groups from each row's
//         own first byte, single bytes at its end, all issued before the first
//         store waits; the same odd-dword row pitch) and gathered with
//         coordinates relative to the box's first pixel, where P itself fits 32
//         bits (92 * 4096 * 4096 < 2^31).  A tile whose box lies inside the
//         frame gathers without border tests.
//       - Otherwise this tile alone gathers from global memory, in int64.
//   * spacing 1 and 2.  A scan for the box would read 65 x 65 nodes a tile, so
//     every tile takes the direct path, with its nodes read from global memory
//     per pixel; at spacing 1 (nothing is interpolated) a lane whose four
//     pixels are all stored reads their four nodes as one 32-byte load.
//
// Every node index is clamped to the mesh, every LDS offset to the box and
// every global tap clamped to or tested against the frame, so a mesh of any
// content reads nothing outside the frame.  The staging and the store are
// copies of k_warp's (csrc/hip/warp.hip stays as it is: its registers and
// times are pinned).
//
// Stores bypass the caches (nt) when source + destination + mesh exceed the
// Infinity Cache (policy::Family::Remap).
#include <climits>

#include "dev_common.h"
#include "stripe/kernels.h"
#include "stripe/remap.h"

namespace stripe {
namespace dev {

struct RemapArgs {
  const uint8_t* src;
  uint8_t* dst;
  const int32_t* mesh;
  int64_t sp, dp;  // pitches
  int W, H;        // source, pixels
  int W2, H2;      // destination, pixels
  int ntx;         // tiles per destination row
  int gw, gh;      // nodes per mesh row, mesh rows
  int s;           // log2 of the spacing
  uint32_t fill;
};

typedef uint32_t u32x4r __attribute__((ext_vector_type(4)));
typedef u32x4r u32x4r_unaligned __attribute__((aligned(1)));
typedef uint32_t u32r_unaligned __attribute__((aligned(1)));
typedef int32_t i32x4r __attribute__((ext_vector_type(4)));
typedef i32x4r i32x4r_a4 __attribute__((aligned(4)));
typedef __attribute__((address_space(3))) uint32_t rlds_u32;
typedef __attribute__((address_space(3))) uint8_t rlds_u8;

__device__ __forceinline__ int rclampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// The taps of one pixel at (ix, iy) with the border rule, from the staged box (LDS: `base` is the box, whose
// first pixel is (ox, oy) of the frame) or from global memory (`base` is the frame).
template <int C, bool BIL, bool REP, bool LDS>
__device__ __forceinline__ void remap_sample(const uint8_t* base, int64_t pitch, int ox, int oy, int W, int H, int ix,
                                             int iy, uint32_t fx, uint32_t fy, uint32_t fill, uint32_t* ob) {
  constexpr int NTAP = BIL ? 2 : 1;
  constexpr int RB = warp_row_bytes(C);
  int colx[NTAP], rowy[NTAP];
  bool okx[NTAP], oky[NTAP];
#pragma unroll
  for (int t = 0; t < NTAP; ++t) {
    int gx = ix + t, gy = iy + t;
    if constexpr (REP) {
      okx[t] = oky[t] = true;
    } else {
      okx[t] = (unsigned)gx < (unsigned)W, oky[t] = (unsigned)gy < (unsigned)H;
    }
    // (clamped under `constant` too: the address of a tap that is not used stays inside the frame)
    colx[t] = rclampi(gx, 0, W - 1), rowy[t] = rclampi(gy, 0, H - 1);
  }
  uint32_t p[NTAP][NTAP][C];
#pragma unroll
  for (int ty = 0; ty < NTAP; ++ty)
#pragma unroll
    for (int tx = 0; tx < NTAP; ++tx) {
      const bool ok = okx[tx] && oky[ty];
      const uint8_t* q;
      if constexpr (LDS)
        q = base + min((uint32_t)((rowy[ty] - oy) * RB + (colx[tx] - ox) * C), (uint32_t)(kWarpBox * RB - C));
      else
        q = base + (int64_t)rowy[ty] * pitch + (int64_t)colx[tx] * C;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const uint32_t v = q[ch];
        p[ty][tx][ch] = ok ? v : fill;
      }
    }
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    if constexpr (BIL) ob[ch] = warp_bilinear(p[0][0][ch], p[0][1][ch], p[1][0][ch], p[1][1][ch], fx, fy);
    else ob[ch] = p[0][0][ch];
  }
}

// LN: the spacing is at least kRemapLdsSpacing (nodes in LDS); the host knows the spacing
template <int C, bool BIL, bool REP, bool LN, bool NT>
__global__ __launch_bounds__(kNT) void k_remap(RemapArgs a) {
  constexpr int T = kWarpTile;
  constexpr int RB = warp_row_bytes(C);
  constexpr int NN = kRemapNodes;
  __shared__ uint32_t box[LN ? kWarpBox * RB / 4 : 1];
  __shared__ int32_t nodes[LN ? NN * NN * 2 : 1];
  __shared__ int32_t red[LN ? kRemapReduceBytes / 4 : 1];
  uint8_t* lb = reinterpret_cast<uint8_t*>(box);
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % a.ntx, by = blockIdx.x / a.ntx;
  const int X0 = bx * T, Y0 = by * T;
  const int nx = min(T, a.W2 - X0), ny = min(T, a.H2 - Y0);
  const int s = a.s, S = 1 << s;
  const int SH = (BIL ? 4 : 12) + 2 * s;  // from P to the Q8 position / the index

  bool staged = false, inside = false, fill_only = false;
  int bx0 = 0, by0 = 0, cx0 = 0, cy0 = 0;
  if constexpr (LN) {
    // the tile's nodes: rows i0 .. i0 + nni - 1, columns j0 .. j0 + nnj - 1 (all of them exist)
    const int i0 = Y0 >> s, j0 = X0 >> s;
    const int nni = ((ny - 1) >> s) + 2, nnj = ((nx - 1) >> s) + 2;
    int mnx = INT_MAX, mny = INT_MAX, mxx = INT_MIN, mxy = INT_MIN;
    for (int k = tid; k < nni * nnj; k += kNT) {
      const int r = k / nnj, c = k - r * nnj;
      const int gi = min(i0 + r, a.gh - 1), gj = min(j0 + c, a.gw - 1);
      const int32_t* np = a.mesh + ((int64_t)gi * a.gw + gj) * 2;
      const int vx = np[0], vy = np[1];
      nodes[(r * NN + c) * 2] = vx, nodes[(r * NN + c) * 2 + 1] = vy;
      mnx = min(mnx, vx), mxx = max(mxx, vx), mny = min(mny, vy), mxy = max(mxy, vy);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mnx = min(mnx, __shfl_xor(mnx, off)), mxx = max(mxx, __shfl_xor(mxx, off));
      mny = min(mny, __shfl_xor(mny, off)), mxy = max(mxy, __shfl_xor(mxy, off));
    }
    if ((tid & 63) == 0) {
      int32_t* r = red + (tid >> 6) * 4;
      r[0] = mnx, r[1] = mxx, r[2] = mny, r[3] = mxy;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kNT / 64; ++w) {
      mnx = min(mnx, red[4 * w]), mxx = max(mxx, red[4 * w + 1]);
      mny = min(mny, red[4 * w + 2]), mxy = max(mxy, red[4 * w + 3]);
    }
    // the same in every lane: scalars
    mnx = __builtin_amdgcn_readfirstlane(mnx), mxx = __builtin_amdgcn_readfirstlane(mxx);
    mny = __builtin_amdgcn_readfirstlane(mny), mxy = __builtin_amdgcn_readfirstlane(mxy);
    // the index is monotone in P, and (S^2 v + rnd) >> shift is (v + RN) >> 12 at a node
    constexpr int RN = BIL ? 8 : 2048;
    bx0 = (int)(((int64_t)mnx + RN) >> 12), by0 = (int)(((int64_t)mny + RN) >> 12);
    const int bx1 = (int)(((int64_t)mxx + RN) >> 12) + (BIL ? 1 : 0);
    const int by1 = (int)(((int64_t)mxy + RN) >> 12) + (BIL ? 1 : 0);
    const bool miss = bx1 < 0 || by1 < 0 || bx0 >= a.W || by0 >= a.H;
    fill_only = !REP && miss;
    staged = !fill_only && bx1 - bx0 < kWarpBox && by1 - by0 < kWarpBox;
    inside = bx0 >= 0 && by0 >= 0 && bx1 < a.W && by1 < a.H;
    if (staged) {
      cx0 = rclampi(bx0, 0, a.W - 1), cy0 = rclampi(by0, 0, a.H - 1);
      const int ncols = min(rclampi(bx1, 0, a.W - 1) - cx0 + 1, kWarpBox);
      const int nrows = min(rclampi(by1, 0, a.H - 1) - cy0 + 1, kWarpBox);
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
        u32x4r gv[kGB];
        int go[kGB];
#pragma unroll
        for (int u = 0; u < kGB; ++u) {
          const int it = base + u * kNT, i = it >> sh, g = it & ((1 << sh) - 1);
          go[u] = i < nrows && g < nb ? i * RB + 16 * g : -1;
          if (go[u] >= 0) gv[u] = *reinterpret_cast<const u32x4r_unaligned*>(s0 + (int64_t)i * a.sp + 16 * g);
        }
#pragma unroll
        for (int u = 0; u < kGB; ++u)
          if (go[u] >= 0) {
            // dword stores: a row's pitch is an odd number of dwords (volatile: see k_warp)
            volatile rlds_u32* lp = (volatile rlds_u32*)(lb + go[u]);
            lp[0] = gv[u].x, lp[1] = gv[u].y, lp[2] = gv[u].z, lp[3] = gv[u].w;
          }
      }
#pragma unroll
      for (int u = 0; u < kTB; ++u)
        if (to[u] >= 0) lb[to[u]] = (uint8_t)tv[u];
      __syncthreads();
    }
  }

  const int x4 = 4 * (tid & 15);
  if (x4 >= nx) return;
  const bool whole = x4 + 4 <= nx;
  // A lane whose four pixels straddle the tile's last column also computes pixels beyond it (they are not
  // stored) as the extension of their cell's patch, whose coordinates can leave the box: every LDS offset is
  // clamped to the last one a tap of the box can have (an unsigned minimum), every global tap to the frame.
  constexpr uint32_t kLastTap = BIL ? kWarpBox * RB - RB - 2 * C : kWarpBox * RB - C;
  for (int yy = tid >> 4; yy < ny; yy += kNT / 16) {
    uint32_t ob[4 * C];
    if (fill_only) {
#pragma unroll
      for (int k = 0; k < 4 * C; ++k) ob[k] = a.fill;
    } else if constexpr (LN) {
      // the lane's four pixels lie in one cell
      const int ty = yy & (S - 1), tx0 = x4 & (S - 1);
      const int32_t* n0 = nodes + ((yy >> s) * NN + (x4 >> s)) * 2;
      const int32_t* n1 = n0 + NN * 2;
      if (staged) {
        // relative to the box's first pixel P fits 32 bits (unsigned: the pixels beyond the tile may wrap)
        const uint32_t ox = (uint32_t)bx0 << 12, oy = (uint32_t)by0 << 12, wy0 = (uint32_t)(S - ty), wy1 = (uint32_t)ty;
        const uint32_t Lx = wy0 * ((uint32_t)n0[0] - ox) + wy1 * ((uint32_t)n1[0] - ox);
        const uint32_t Rx = wy0 * ((uint32_t)n0[2] - ox) + wy1 * ((uint32_t)n1[2] - ox);
        const uint32_t Ly = wy0 * ((uint32_t)n0[1] - oy) + wy1 * ((uint32_t)n1[1] - oy);
        const uint32_t Ry = wy0 * ((uint32_t)n0[3] - oy) + wy1 * ((uint32_t)n1[3] - oy);
        const uint32_t dX = Rx - Lx, dY = Ry - Ly;
        uint32_t Px = (uint32_t)S * Lx + (uint32_t)tx0 * dX + (1u << (SH - 1));
        uint32_t Py = (uint32_t)S * Ly + (uint32_t)tx0 * dY + (1u << (SH - 1));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j > 0) Px += dX, Py += dY;
          const int qx = (int)Px >> SH, qy = (int)Py >> SH;  // the Q8 position / the index, relative
          const int rx = BIL ? qx >> 8 : qx, ry = BIL ? qy >> 8 : qy;
          const uint32_t fx = (uint32_t)qx & 255u, fy = (uint32_t)qy & 255u;
          if (inside) {
            // every tap of the tile is inside the frame and the box starts at its own first tap
            const volatile rlds_u8* q = (const volatile rlds_u8*)(lb + min((uint32_t)(ry * RB + rx * C), kLastTap));
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
              if constexpr (BIL) ob[j * C + ch] = warp_bilinear(q[ch], q[C + ch], q[RB + ch], q[RB + C + ch], fx, fy);
              else ob[j * C + ch] = q[ch];
            }
          } else {
            remap_sample<C, BIL, REP, true>(lb, 0, cx0, cy0, a.W, a.H, bx0 + rx, by0 + ry, fx, fy, a.fill, ob + j * C);
          }
        }
      } else {
        const int64_t wy0 = S - ty, wy1 = ty;
        const int64_t Lx = wy0 * n0[0] + wy1 * n1[0], Rx = wy0 * n0[2] + wy1 * n1[2];
        const int64_t Ly = wy0 * n0[1] + wy1 * n1[1], Ry = wy0 * n0[3] + wy1 * n1[3];
        const int64_t dX = Rx - Lx, dY = Ry - Ly;
        int64_t Px = S * Lx + tx0 * dX + (int64_t(1) << (SH - 1)), Py = S * Ly + tx0 * dY + (int64_t(1) << (SH - 1));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j > 0) Px += dX, Py += dY;
          const int qx = (int)(Px >> SH), qy = (int)(Py >> SH);
          remap_sample<C, BIL, REP, false>(a.src, a.sp, 0, 0, a.W, a.H, BIL ? qx >> 8 : qx, BIL ? qy >> 8 : qy,
                                           (uint32_t)qx & 255u, (uint32_t)qy & 255u, a.fill, ob + j * C);
        }
      }
    } else {
      const int y = Y0 + yy, i = y >> s, i1 = min(i + 1, a.gh - 1);
      const int64_t ty = y & (S - 1);
      i32x4r v0, v1;
      const bool row_load = s == 0 && whole;  // nothing is interpolated: the four pixels' own nodes, 32 bytes
      if (row_load) {
        const int32_t* np = a.mesh + ((int64_t)i * a.gw + (X0 + x4)) * 2;
        v0 = *reinterpret_cast<const i32x4r_a4*>(np), v1 = *reinterpret_cast<const i32x4r_a4*>(np + 4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int64_t Px, Py;
        if (row_load) {
          Px = j == 0 ? v0.x : j == 1 ? v0.z : j == 2 ? v1.x : v1.z;
          Py = j == 0 ? v0.y : j == 1 ? v0.w : j == 2 ? v1.y : v1.w;
        } else {
          const int x = min(X0 + x4 + j, a.W2 - 1), jn = x >> s, jn1 = min(jn + 1, a.gw - 1);
          const int64_t tx = x & (S - 1);
          const int32_t* m00 = a.mesh + ((int64_t)i * a.gw + jn) * 2;
          const int32_t* m01 = a.mesh + ((int64_t)i * a.gw + jn1) * 2;
          const int32_t* m10 = a.mesh + ((int64_t)i1 * a.gw + jn) * 2;
          const int32_t* m11 = a.mesh + ((int64_t)i1 * a.gw + jn1) * 2;
          const int64_t w00 = (S - tx) * (S - ty), w01 = tx * (S - ty), w10 = (S - tx) * ty, w11 = tx * ty;
          Px = w00 * m00[0] + w01 * m01[0] + w10 * m10[0] + w11 * m11[0];
          Py = w00 * m00[1] + w01 * m01[1] + w10 * m10[1] + w11 * m11[1];
        }
        const int qx = (int)((Px + (int64_t(1) << (SH - 1))) >> SH), qy = (int)((Py + (int64_t(1) << (SH - 1))) >> SH);
        remap_sample<C, BIL, REP, false>(a.src, a.sp, 0, 0, a.W, a.H, BIL ? qx >> 8 : qx, BIL ? qy >> 8 : qy,
                                         (uint32_t)qx & 255u, (uint32_t)qy & 255u, a.fill, ob + j * C);
      }
    }
    // from pixel-major to the bytes of the row
    uint8_t* dp = a.dst + (int64_t)(Y0 + yy) * a.dp + (int64_t)(X0 + x4) * C;
    if (whole) {
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const uint32_t v4 = pack4(ob[4 * k], ob[4 * k + 1], ob[4 * k + 2], ob[4 * k + 3]);
        if constexpr (NT) __builtin_nontemporal_store(v4, reinterpret_cast<u32r_unaligned*>(dp + 4 * k));
        else *reinterpret_cast<u32r_unaligned*>(dp + 4 * k) = v4;
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
void launch_inst(bool ln, bool nt, const dev::RemapArgs& a, unsigned grid, hipStream_t s) {
  if (ln) {
    if (nt) dev::k_remap<C, BIL, REP, true, true><<<grid, dev::kNT, 0, s>>>(a);
    else dev::k_remap<C, BIL, REP, true, false><<<grid, dev::kNT, 0, s>>>(a);
  } else {
    if (nt) dev::k_remap<C, BIL, REP, false, true><<<grid, dev::kNT, 0, s>>>(a);
    else dev::k_remap<C, BIL, REP, false, false><<<grid, dev::kNT, 0, s>>>(a);
  }
}
template <int C>
void launch_c(bool bil, bool rep, bool ln, bool nt, const dev::RemapArgs& a, unsigned grid, hipStream_t s) {
  if (bil) {
    if (rep) launch_inst<C, true, true>(ln, nt, a, grid, s);
    else launch_inst<C, true, false>(ln, nt, a, grid, s);
  } else {
    if (rep) launch_inst<C, false, true>(ln, nt, a, grid, s);
    else launch_inst<C, false, false>(ln, nt, a, grid, s);
  }
}
}  // namespace

void launch_remap_kernel(const RemapLaunch& L, hipStream_t s) {
  const RemapMesh& m = L.mesh;
  dev::RemapArgs a{};
  a.src = L.src;
  a.dst = L.dst;
  a.mesh = m.nodes;
  a.sp = L.src_pitch;
  a.dp = L.dst_pitch;
  a.W = L.W, a.H = L.H;
  a.W2 = m.W2, a.H2 = m.H2;
  a.gw = m.gw(), a.gh = m.gh();
  a.s = m.shift;
  a.fill = m.fill;
  a.ntx = (int)div_up(m.W2, kWarpTile);
  const int64_t nwg = a.ntx * div_up(m.H2, kWarpTile);
  STRIPE_CHECK(nwg < (int64_t(1) << 31), "remap: too many workgroups");
  policy::PolicyIn pin{policy::Family::Remap};
  pin.cin = pin.cout = pin.cmid = L.C;
  pin.W = L.W, pin.rows = L.H;
  pin.W2 = m.W2, pin.rows2 = m.H2;
  pin.mesh_bytes = L.mesh_count * 4;
  const bool nt = policy::stream_policy(pin).nt_stores;
  const bool bil = m.mode == WarpMode::Bilinear, rep = m.border == WarpBorder::Replicate;
  const bool ln = (1 << m.shift) >= kRemapLdsSpacing;
  if (L.C == 1) launch_c<1>(bil, rep, ln, nt, a, (unsigned)nwg, s);
  else launch_c<3>(bil, rep, ln, nt, a, (unsigned)nwg, s);
  HIP_CHECK(hipGetLastError());
}

void remap_device(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch,
                  const RemapMesh& mesh, int64_t mesh_count, hipStream_t s) {
  RemapLaunch L;
  L.src = src;
  L.src_pitch = src_pitch;
  L.W = W, L.H = H, L.C = C;
  L.dst = dst;
  L.dst_pitch = dst_pitch;
  L.mesh = mesh;
  L.mesh_count = mesh_count;
  launch_remap(L, s);
}

}  // namespace stripe
