// Device helpers shared by the stripe kernels (gfx950, wave64).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch_policy.h"
#include "stripe/common.h"
#include "stripe/kernels.h"

namespace stripe {
namespace dev {

constexpr int kNT = 256;  // threads per workgroup (4 waves)

// Kernel argument block (by value, scalar registers).
struct KArgs {
  const uint8_t* in;
  uint8_t* out;
  const uint8_t* luts;      // [pre | post | epi] 256 B each
  const uint8_t* zero_row;  // origin of a zero row (Constant y-border)
  int64_t in_pitch, out_pitch;
  int W;          // pixels
  int E;          // output row bytes (W * cmid for stencils, W * cout for pointwise)
  int rows;       // local rows
  int row0, Hg;   // border geometry
  int border;     // Border enum
  int ry0, ry1, ry2, ry3;  // output row ranges [ry0,ry1) U [ry2,ry3)
  int band;       // rows per wave task
  int nb0;        // bands covering range 0
  int ntx;        // wave tiles per row (stencil kernels)
  int nbands;     // bands over both ranges
  int out_px;     // x-margin pixels to maintain on the output
  int out_border; // border mode encoded in those margins
  int has_pre, has_post, has_epi;
  // post LUT as an affine map clamp((post_a * v + post_b) >> post_k, 0, 255)
  // (exact for every v, found by the host; 0: use the table)
  int post_aff, post_a, post_b, post_k;
  int gmode;      // 0 bt601, 1 ref
  uint32_t gmul[3];
  int gshift[3];
  int cin;        // pointwise: input channels
  int nxcd;       // > 1: XCD-aware workgroup remap over this many L2 domains
  // buffer-descriptor view (stencil kernels): offsets of the origins in the
  // allocations; every hot-loop load/store is a raw buffer op whose range check
  // masks inactive lanes (no divergent branches around memory ops, so hipcc's
  // vmcnt bookkeeping stays exact and prefetched rows stay in flight)
  const uint8_t* in_base;
  uint8_t* out_base;
  uint32_t in_bytes, in_org, in_zero;
  uint32_t out_bytes, out_org;
  // colour matrix pass (k_colormix): q row-major, then qb (Q12, filters.h)
  int cm[12];
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}

constexpr uint32_t kOOB = 0x80000000u;  // lane offset bias that fails the range check

// Cache-policy (aux) bits of the stencil hot-loop buffer ops (gfx950: 1 = sc0,
// 2 = nt, 16 = sc1).  Loads keep the default policy: halo rows are re-read by
// the neighbouring band (nt loads measured 12-15 % slower on a 16K RGB frame).
// Stores use nt when a pass streams more than the 256 MiB Infinity Cache
// (launch_policy.h decides; the launcher picks the kernel instance).
constexpr int kLoadAux = 0;
constexpr int kNtAux = 2;

__device__ __forceinline__ int border_index_dev(int i, int n, int b) {
  if (i >= 0 && i < n) return i;
  if (b == (int)Border::Constant) return -1;
  if (b == (int)Border::Replicate) return i < 0 ? 0 : n - 1;
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  int j = i % period;
  if (j < 0) j += period;
  return j < n ? j : period - j;
}

// Byte offset (in the input allocation) of local row y's origin, global-edge
// border applied (scalar; no memory access).
__device__ __forceinline__ uint32_t in_row_off(const KArgs& a, int y) {
  int g = a.row0 + y;
  if (g < 0 || g >= a.Hg) {
    const int m = border_index_dev(g, a.Hg, a.border);
    if (m < 0) return a.in_zero;
    g = m;
  }
  return a.in_org + (uint32_t)((int64_t)(g - a.row0) * a.in_pitch);
}

// True when input rows [y0, y1] of this wave's band need no border remap: the
// hot loop then computes row offsets without the remap's scalar branch tree
// (three scalar branches and the remap per row otherwise).
__device__ __forceinline__ bool rows_inside(const KArgs& a, int y0, int y1) {
  return a.row0 + y0 >= 0 && a.row0 + y1 < a.Hg;
}

// Offset of the input row feeding step y + ahead of a band ending at ye (rows
// past the band re-read its last input row).  `inner` (wave-uniform): the
// band's rows need no border remap (rows_inside) -> straight-line scalar math,
// no branch tree; the remap stays for the edge bands.
__device__ __forceinline__ uint32_t ahead_row_off(const KArgs& a, bool inner, int y, int ahead, int ye, int R,
                                                  uint32_t last_row) {
  if (inner) return a.in_org + (uint32_t)(min(y + ahead, ye - 1) + R) * (uint32_t)a.in_pitch;
  return y + ahead < ye ? in_row_off(a, y + ahead + R) : last_row;
}

// Bijective XCD-aware remap of the workgroup index: the hardware hands
// consecutive workgroups to the XCDs round-robin (blockIdx % 8 shares an L2),
// so logical workgroup ranges are made contiguous per XCD: vertically /
// horizontally adjacent tiles (which share halo rows / window bytes) then meet
// in one L2 (cdna_hip_programming.md T1).
__device__ __forceinline__ int xcd_remap(int bid, int nwg, int nxcd) {
  if (nxcd <= 1 || nwg < nxcd) return bid;
  const int q = nwg / nxcd, r = nwg % nxcd;
  const int x = bid % nxcd, slot = bid / nxcd;
  return x * q + min(x, r) + slot;
}

// Row range of workgroup row `by`.
__device__ __forceinline__ void band_range(const KArgs& a, int by, int& ys, int& ye) {
  if (by < a.nb0) {
    ys = a.ry0 + by * a.band;
    ye = min(ys + a.band, a.ry1);
  } else {
    ys = a.ry2 + (by - a.nb0) * a.band;
    ye = min(ys + a.band, a.ry3);
  }
}

// Orders this wave's LDS writes before its later LDS reads of other lanes' data
// (LDS ops of one wave execute in order; this only stops compiler reordering).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return a | (b << 8) | (c << 16) | (d << 24);
}

// Gray of one pixel (semantic R, G, B).
__device__ __forceinline__ uint32_t gray_dev(const KArgs& a, uint32_t r, uint32_t g, uint32_t b) {
  if (a.gmode == 1)
    return ((r * a.gmul[0]) >> a.gshift[0]) + ((g * a.gmul[1]) >> a.gshift[1]) +
           ((b * a.gmul[2]) >> a.gshift[2]);
  return (r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14;
}

// 16 RGB pixels (48 bytes) -> 16 gray bytes (4 dwords).
__device__ __forceinline__ void gray16(const KArgs& a, const uint32_t (&rgb)[12], uint32_t (&o)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int p = q * 4 + e;
      const int b0 = 3 * p;
      const uint32_t r = (rgb[b0 >> 2] >> ((b0 & 3) * 8)) & 0xFF;
      const uint32_t g = (rgb[(b0 + 1) >> 2] >> (((b0 + 1) & 3) * 8)) & 0xFF;
      const uint32_t bl = (rgb[(b0 + 2) >> 2] >> (((b0 + 2) & 3) * 8)) & 0xFF;
      v[e] = gray_dev(a, r, g, bl);
    }
    o[q] = pack4(v[0], v[1], v[2], v[3]);
  }
}

__device__ __forceinline__ void lut16(const uint8_t* lut, uint32_t (&o)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t w = o[q];
    o[q] = pack4(lut[w & 0xFF], lut[(w >> 8) & 0xFF], lut[(w >> 16) & 0xFF], lut[w >> 24]);
  }
}

// ---- host side ----
// The part of the argument block every launch fills the same way: geometry,
// border, the buffer-descriptor view (checked) and the output row ranges.
// n0 / n1: rows of the two ranges; tiles: wave tiles per row.
struct TileLaunch {
  int n0, n1, tiles;
};
// The allocation-view check as one launcher words it.
struct ViewCheck {
  const char* channels;    // cmid not 1 or 3 (nullptr: the caller has checked)
  const char* need_view;   // in_base / out_base missing
  const char* too_big;     // a view of 2 GiB or more
  int64_t out_slack = 0;   // bytes the output view must stay below 2 GiB by
};
// view == nullptr (pointwise passes: plain pointers, E = W * cout, one launch
// per row range): only the pointers, pitches, W and E are filled.
// Defined in stencil.hip.
TileLaunch fill_tile_args(const Pass& p, const PassLaunch& L, KArgs& a, const ViewCheck* view);

// What policy::stream_policy asks about a launch of `rows` output rows.
inline policy::PolicyIn policy_in(policy::Family f, const Pass& p, const PassLaunch& L, int rows) {
  policy::PolicyIn in{f};
  in.cin = p.cin;
  in.cout = p.cout;
  in.cmid = p.cmid;
  in.W = L.W;
  in.rows = rows;
  in.nt = L.nt;
  in.wgs = L.wgs;
  in.gray_prologue = p.pro.gray;
  in.lut_stage = p.pro.has_pre || p.pro.has_post;
  return in;
}

}  // namespace dev
}  // namespace stripe
