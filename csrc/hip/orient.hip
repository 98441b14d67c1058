// Orientation and crop of a whole frame: the eight orientations of the
// rectangle (k_orient).  The rule is stripe/orient.h's; the kernel is
// bit-identical to golden_orient.
//
// The launcher gets the source window (a crop is only a view of the source)
// and the three bits T, FX, FY.  Two code shapes:
//
//   * T = 0 without FX (`none`, `flipv`): rows are copied.  A workgroup owns
//     kOrientCopyRows rows of a 4 KiB column of the frame; a lane moves 16
//     bytes per row, stored at the destination row's own 16-byte boundaries
//     (single bytes up to the first and after the last of them), loaded from
//     wherever that puts it in the source row.  FY only picks the source row.
//   * every other orientation goes through a tile in LDS.  The workgroup
//     stages orient_tile_rows(T) source rows of orient_seg_px(C, T) pixels
//     (64 rows of 256 gray / 128 RGB pixels for FX, whole 128-byte lines on
//     both sides; 128 rows of 128 / 64 pixels for the transposing ops): per row
//     single bytes up to the first 16-byte boundary of the row's own address,
//     whole 16-byte groups, single bytes at the end, so nothing outside the
//     window's rows is read and no alignment of pointers or pitches is
//     assumed.  The LDS image of a row keeps the address's phase within a
//     dword (4 dword writes per group).  Then every lane assembles
//     destination dwords, contiguous along destination rows, from four byte
//     reads; it keeps its dword columns down the tile, so the four addresses
//     are computed once and a row step adds one term to them.  For the
//     transposing ops the four bytes of a gray dword come from
//     four source rows, and neighbouring lanes are four rows apart, so the
//     image pads one dword behind every four rows (group pitch odd): the 32
//     lanes of a half wave then read 32 different banks (gray; RGB keeps
//     2-way conflicts where a dword straddles pixels, see
//     profiles/orient/README.md).  The flips are reflections of the tile's
//     coordinates, FX within a row included; they cost index arithmetic only.
//
// Stores bypass the caches (nt) when source + destination exceed the Infinity
// Cache (policy::Family::Orient).
#include "dev_common.h"
#include "stripe/kernels.h"
#include "stripe/orient.h"

namespace stripe {
namespace dev {

struct OrientArgs {
  const uint8_t* src;  // the source window
  uint8_t* dst;
  int64_t sp, dp;  // pitches
  int w, h;        // source window, pixels
  int W2, H2;      // destination, pixels
  int fx, fy;
  int ntx;         // tiles per destination row
};

typedef uint32_t u32x4o __attribute__((ext_vector_type(4)));
typedef u32x4o u32x4o_unaligned __attribute__((aligned(1)));
typedef uint32_t u32o_unaligned __attribute__((aligned(1)));

template <int C, bool T, bool FX, bool NT>
__global__ __launch_bounds__(kNT) void k_orient(OrientArgs a) {
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % a.ntx, by = blockIdx.x / a.ntx;
  const bool fy = a.fy != 0;
  if constexpr (!T && !FX) {
    // ---- row copies ----
    const int E = a.W2 * C;
    const int gi = bx * kNT + tid;
    u32x4o v[kOrientCopyRows];
    bool full[kOrientCopyRows];
    int off[kOrientCopyRows];
#pragma unroll
    for (int r = 0; r < kOrientCopyRows; ++r) {
      const int y = by * kOrientCopyRows + r;
      full[r] = false;
      off[r] = 0;
      if (y >= a.H2) continue;
      const uint8_t* sr = a.src + (int64_t)(fy ? a.h - 1 - y : y) * a.sp;
      uint8_t* dr = a.dst + (int64_t)y * a.dp;
      const int head = min(E, (16 - (int)((uintptr_t)dr & 15)) & 15);
      const int nbody = (E - head) >> 4;
      off[r] = head + 16 * gi;
      full[r] = gi < nbody;
      if (full[r]) v[r] = *reinterpret_cast<const u32x4o_unaligned*>(sr + off[r]);
      const int t0 = head + 16 * nbody;
      if (gi < head) dr[gi] = sr[gi];
      if (gi < E - t0) dr[t0 + gi] = sr[t0 + gi];
    }
#pragma unroll
    for (int r = 0; r < kOrientCopyRows; ++r) {
      if (!full[r]) continue;
      u32x4o* dp = reinterpret_cast<u32x4o*>(a.dst + (int64_t)(by * kOrientCopyRows + r) * a.dp + off[r]);
      if constexpr (NT) __builtin_nontemporal_store(v[r], dp);
      else *dp = v[r];
    }
  } else {
    // ---- a tile through LDS ----
    constexpr int NR = orient_tile_rows(T), SEG = orient_seg_px(C, T);
    constexpr int RL = orient_row_dwords(C, T), PQ = orient_group_dwords(C, T);
    constexpr int TWd = T ? NR : SEG, THd = T ? SEG : NR;  // the destination tile, pixels
    constexpr int G = SEG * C / 16;                        // most whole 16-byte groups of a row
    __shared__ uint32_t tile[NR / 4 * PQ];
    uint8_t* lb = reinterpret_cast<uint8_t*>(tile);
    const bool fx = T ? a.fx != 0 : FX;
    const int X0 = bx * TWd, Y0 = by * THd;
    const int x1 = min(X0 + TWd, a.W2), y1 = min(Y0 + THd, a.H2);
    const int nx = x1 - X0, ny = y1 - Y0;
    // the source rows and columns the tile maps from
    const int nrows = T ? nx : ny, ncols = T ? ny : nx;
    const int Rlo = T ? (fy ? a.h - x1 : X0) : (fy ? a.h - y1 : Y0);
    const int Clo = T ? (fx ? a.w - y1 : Y0) : (fx ? a.w - x1 : X0);
    const uint8_t* s0 = a.src + (int64_t)Rlo * a.sp + (int64_t)Clo * C;
    const int n = ncols * C;  // bytes of a staged row, <= SEG * C
    auto rowoff = [](int i) { return ((i >> 2) * PQ + (i & 3) * RL) * 4; };

    for (int it = tid; it < nrows * (G + 2); it += kNT) {
      const int i = it / (G + 2), sl = it - i * (G + 2);
      const uint8_t* rp = s0 + (int64_t)i * a.sp;
      const int mis = (int)((uintptr_t)rp & 15);
      const int head = min(n, (16 - mis) & 15);
      const int nbody = (n - head) >> 4;
      uint8_t* lr = lb + rowoff(i) + (mis & 3);
      if (sl == 0) {
        for (int k = 0; k < head; ++k) lr[k] = rp[k];
      } else if (sl == G + 1) {
        for (int k = head + 16 * nbody; k < n; ++k) lr[k] = rp[k];
      } else if (sl - 1 < nbody) {
        const int o = head + 16 * (sl - 1);  // 16-byte aligned in memory, dword aligned in LDS
        const u32x4o q = *reinterpret_cast<const u32x4o*>(rp + o);
        uint32_t* lp = reinterpret_cast<uint32_t*>(lr + o);
        lp[0] = q.x, lp[1] = q.y, lp[2] = q.z, lp[3] = q.w;
      }
    }
    __syncthreads();

    // A lane keeps its dword columns for the whole tile, so where its four
    // bytes sit in a staged row (T = 0) or which staged rows they come from
    // (T = 1) is computed once; a step down the destination rows adds one
    // term to the four LDS addresses.
    constexpr int DW = TWd * C / 4;                 // dwords of a full tile row
    constexpr int RPI = DW >= 64 ? 1 : 64 / DW;     // destination rows a wave covers per step
    constexpr int NCOL = (DW + 63) / 64;            // dword columns of a lane
    const int nb = nx * C;                          // bytes of this tile's rows
    const int sp4 = (int)(a.sp & 3), b4 = (int)((uintptr_t)s0 & 3);
    const int lane = tid & 63, wv = tid >> 6;
    const int rsub = RPI > 1 ? lane / DW : 0, col0 = RPI > 1 ? lane % DW : lane;
    int base[NCOL][4];
    bool valid[NCOL], whole[NCOL];
#pragma unroll
    for (int k = 0; k < NCOL; ++k) {
      const int bb = 4 * (col0 + 64 * k);
      valid[k] = col0 + 64 * k < DW && bb < nb;
      whole[k] = bb + 4 <= nb;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = valid[k] ? min(bb + j, nb - 1) : 0;  // bytes past the row repeat its last one (not stored)
        const int xl = b / C, ch = b - xl * C;
        if constexpr (T) {
          const int i = fy ? nrows - 1 - xl : xl;
          base[k][j] = rowoff(i) + ((b4 + i * sp4) & 3) + ch;
        } else {
          base[k][j] = (fx ? ncols - 1 - xl : xl) * C + ch;
        }
      }
    }
    for (int yy = wv * RPI + rsub; yy < ny; yy += (kNT / 64) * RPI) {
      int var;
      if constexpr (T) {
        var = (fx ? ncols - 1 - yy : yy) * C;
      } else {
        const int i = fy ? nrows - 1 - yy : yy;
        var = rowoff(i) + ((b4 + i * sp4) & 3);
      }
      uint8_t* drow = a.dst + (int64_t)(Y0 + yy) * a.dp + (int64_t)X0 * C;
#pragma unroll
      for (int k = 0; k < NCOL; ++k) {
        if (!valid[k]) continue;
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = lb[base[k][j] + var];
        const int bb = 4 * (col0 + 64 * k);
        uint8_t* dp = drow + bb;
        if (whole[k]) {
          const uint32_t v4 = pack4(o[0], o[1], o[2], o[3]);
          if constexpr (NT) __builtin_nontemporal_store(v4, reinterpret_cast<u32o_unaligned*>(dp));
          else *reinterpret_cast<u32o_unaligned*>(dp) = v4;
        } else {  // the row's last 1..3 bytes
#pragma unroll
          for (int j = 0; j < 3; ++j)
            if (bb + j < nb) dp[j] = (uint8_t)o[j];
        }
      }
    }
  }
}

}  // namespace dev

namespace {
template <int C, bool T, bool FX>
void launch_nt(bool nt, const dev::OrientArgs& a, unsigned grid, hipStream_t s) {
  if (nt) dev::k_orient<C, T, FX, true><<<grid, dev::kNT, 0, s>>>(a);
  else dev::k_orient<C, T, FX, false><<<grid, dev::kNT, 0, s>>>(a);
}
template <int C>
void launch_c(bool t, bool fx, bool nt, const dev::OrientArgs& a, unsigned grid, hipStream_t s) {
  if (t) launch_nt<C, true, false>(nt, a, grid, s);  // FX and FY are reflections of the tile
  else if (fx) launch_nt<C, false, true>(nt, a, grid, s);
  else launch_nt<C, false, false>(nt, a, grid, s);
}
}  // namespace

void launch_orient_kernel(const OrientLaunch& L, hipStream_t s) {
  const bool t = orient_t(L.op), fx = orient_fx(L.op);
  dev::OrientArgs a{};
  a.src = L.src;
  a.dst = L.dst;
  a.sp = L.src_pitch;
  a.dp = L.dst_pitch;
  a.w = L.w, a.h = L.h;
  a.W2 = t ? L.h : L.w;
  a.H2 = t ? L.w : L.h;
  a.fx = fx, a.fy = orient_fy(L.op);
  int64_t nty;
  if (!t && !fx) {
    a.ntx = (int)div_up(((int64_t)a.W2 * L.C >> 4) + 1, dev::kNT);
    nty = div_up(a.H2, kOrientCopyRows);
  } else {
    a.ntx = (int)div_up(a.W2, t ? orient_tile_rows(true) : orient_seg_px(L.C, false));
    nty = div_up(a.H2, t ? orient_seg_px(L.C, true) : orient_tile_rows(false));
  }
  const int64_t nwg = a.ntx * nty;
  STRIPE_CHECK(nwg < (int64_t(1) << 31), "orient: too many workgroups");
  policy::PolicyIn pin{policy::Family::Orient};
  pin.cin = pin.cout = pin.cmid = L.C;
  pin.W = L.w, pin.rows = L.h;
  const bool nt = policy::stream_policy(pin).nt_stores;
  if (L.C == 1) launch_c<1>(t, fx, nt, a, (unsigned)nwg, s);
  else launch_c<3>(t, fx, nt, a, (unsigned)nwg, s);
  HIP_CHECK(hipGetLastError());
}

void orient_device(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch,
                   Orient op, const CropRect& crop, hipStream_t s) {
  STRIPE_CHECK(C == 1 || C == 3, "orient: image must have 1 or 3 channels, got C = " << C);
  STRIPE_CHECK(W >= 1 && W <= kOrientMaxSize && H >= 1 && H <= kOrientMaxSize,
               "orient: size " << W << "x" << H << " outside 1.." << kOrientMaxSize);
  STRIPE_CHECK(src, "orient: null source");
  if (!crop.empty())
    check_crop(crop, orient_t(op) ? H : W, orient_t(op) ? W : H,
               std::to_string(crop.w) + "x" + std::to_string(crop.h) + "+" + std::to_string(crop.x0) + "+" +
                   std::to_string(crop.y0));
  const CropRect sw = orient_source_window(op, W, H, crop);
  OrientLaunch L;
  L.src = src + (int64_t)sw.y0 * src_pitch + (int64_t)sw.x0 * C;
  L.src_pitch = src_pitch;
  L.w = sw.w, L.h = sw.h, L.C = C;
  L.dst = dst;
  L.dst_pitch = dst_pitch;
  L.op = op;
  launch_orient(L, s);
}

}  // namespace stripe
