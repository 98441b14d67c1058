// Bilateral filter kernels (k_bilateral: bilateral3/5) and their launch
// template; instantiated in stencil_inst_f.hip.
#pragma once

// k_bilateral is the register-ring row walk (ring_task, stencil_kernels.h) with
// BilateralRow as its row operation, as k_rank is with RankRow: bands, the two
// output ranges, @skip, the prologues, the epilogue LUT, the expand epilogue,
// margins, nt stores and re-based launches need nothing special.
//
// The rule is filters.h's: per tap w = ws(dy,dx) r[|p - c|], D = sum w,
// N = sum w p, out = (N + (D >> 1)) / D.  Per output pair and tap:
//   * the signed difference of the two pixels, biased: 256 + p - c per u16
//     field in one 32-bit add (256 - c is formed once per output pair);
//   * two byte reads of the range table, which the kernel keeps in LDS behind
//     the three LUTs, mirrored so that the biased difference indexes it:
//     rng[256 + d] = r[|d|] (the pass's constant block is [pre | post | epi |
//     range]; 512 bytes in LDS).  Besides saving the packed max / min / sub of
//     an absolute difference, the signed form keeps the compiler from
//     recognising |p - c| of one step as |c' - p'| of the next and holding
//     looked-up weights in registers across the unrolled rows;
//   * w = r ws as one packed u16 multiply by the tap (<= 36 * 255), D
//     accumulated packed (<= 65280 per field), N per pixel in 32 bits
//     (bilateral_tap);
//   * the centre tap needs no lookup: r[0] = 255.
// The quotient is exact: n = N + (D >> 1) < 2^24 and D < 2^16 are exact in
// f32, v_rcp_f32 is good to 1 ulp, so trunc(n * rcp(D)) is off by at most one
// (the relative error 2^-22 times a quotient <= 255 is far below 1), and one
// integer step from the remainder n - q D puts it right.  No divide loop.

#include "stencil_kernels.h"

namespace stripe {
namespace dev {

// One tap of one output pair: with w = r * ws per u16 field (r: the two range
// weights, ws: the tap in both halves, v: the two window pixels)
//   d += w per field,  n0 += w.lo * v.lo,  n1 += w.hi * v.hi  (32-bit sums).
// One asm block: v_mad_u32_u16 with op_sel reads the fields where they lie.  As
// plain C++ the compiler (a) extracts every ring field once and keeps the
// zero-extended copies live across the row's 8 output pairs, (b) reassociates
// the sum of weights into a tree at the row's end and keeps every tap's w live
// until then: both spill; and the row walk's unrolled loop grows past the
// size the compiler still unrolls, which puts the ring into scratch.
__device__ __forceinline__ void bilateral_tap(uint32_t& d, uint32_t& n0, uint32_t& n1, uint32_t r, uint32_t ws,
                                              uint32_t v) {
  uint32_t w;
  asm("v_pk_mul_lo_u16 %3, %4, %5\n\t"
      "v_pk_mad_u16 %0, %4, %5, %0\n\t"
      "v_mad_u32_u16 %1, %3, %6, %1\n\t"
      "v_mad_u32_u16 %2, %3, %6, %2 op_sel:[1,1,0,0]"
      : "+v"(d), "+v"(n0), "+v"(n1), "=&v"(w)
      : "v"(r), "s"(ws), "v"(v));
}

// floor(n / d) for n < 2^24, 0 < d < 2^16 and a quotient below 2^8 (see above)
__device__ __forceinline__ uint32_t div_small_exact(uint32_t n, uint32_t d) {
  uint32_t q = (uint32_t)((float)n * __builtin_amdgcn_rcpf((float)d));
  const int rem = (int)(n - q * d);
  q += rem >= (int)d ? 1u : 0u;
  q -= rem < 0 ? 1u : 0u;
  return q;
}

// Row operation of the bilateral filters: the lane's 8 output pairs of one row
// from the K extended ring rows; ring[(o + dy) % K] holds window row dy.
template <int C, class F>
struct BilateralRow {
  static constexpr int NX = RingDims<C, F>::NX, NE = RingDims<C, F>::NE;
  const uint8_t* rng;  // the mirrored range table in LDS: rng[256 + d] = r[|d|], -255 <= d <= 255
  __device__ __forceinline__ void operator()(const uint32_t (&ring)[F::K][NE], int o, uint32_t (&h)[8]) const {
    constexpr int K = F::K, R = F::R;
    constexpr uint32_t kCentre = 255u * (uint32_t)F::w(R, R);  // ws(centre) r[0]
    const uint32_t(&cr)[NE] = ring[(o + R) % K];
    uint32_t D[8], N0[8], N1[8];  // D: packed u16 fields
#pragma unroll
    for (int pp = 0; pp < 8; ++pp) {
      const uint32_t c = cr[NX + pp];
      D[pp] = kCentre * 0x00010001u;
      N0[pp] = kCentre * (c & 0xFFFFu);
      N1[pp] = kCentre * (c >> 16);
    }
    // window row by window row: the row's odd-shifted pair views (one
    // v_alignbyte each, shared by neighbouring output pairs) live for that row
    // only.  The fences keep one output pair's K taps (2 K table reads) in
    // flight at a time: left alone, the scheduler hoists the reads of the
    // whole row of 8 pairs (up to 384 live results) and spills.
#pragma unroll
    for (int dy = 0; dy < K; ++dy) {
      const uint32_t(&row)[NE] = ring[(o + dy) % K];
#pragma unroll
      for (int pp = 0; pp < 8; ++pp) {
        uint32_t cb = 0x01000100u - cr[NX + pp];  // 256 - c per field
        asm("" : "+v"(cb));                        // (kept as one operand: v + cb is one add per tap)
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
          if (dy == R && dx == R) continue;
          const uint32_t v = pair_at(row, 2 * NX + 2 * pp + (dx - R) * C);
          const uint32_t d = v + cb;  // 256 + p - c per field, in [1, 511]: no carry
          const uint32_t r = (uint32_t)rng[d & 0xFFFFu] | ((uint32_t)rng[d >> 16] << 16);
          bilateral_tap(D[pp], N0[pp], N1[pp], r, (uint32_t)F::w(dy, dx) * 0x00010001u, v);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int pp = 0; pp < 8; ++pp) {
      const uint32_t D0 = D[pp] & 0xFFFFu, D1 = D[pp] >> 16;
      h[pp] = div_small_exact(N0[pp] + (D0 >> 1), D0) | (div_small_exact(N1[pp] + (D1 >> 1), D1) << 16);
    }
  }
};

// Waves per SIMD from the compiler's register report (build/kernel_resources.json):
// K = 5 takes 147-200 VGPRs (2 waves, some instances 3), K = 3 95-128, and with a
// gray prologue (36 raw dwords in flight) 134-136: 3 waves rather than a spill.
template <int C, class F, int PRO, bool SKIP, int SAUX, bool EXP = false>
__global__ __launch_bounds__(kNT, (F::K >= 5 ? 2 : is_gray(PRO) ? 3 : 4)) void k_bilateral(KArgs a) {
  static_assert(F::BILATERAL != 0, "k_bilateral runs bilateral filters");
  __shared__ uint8_t luts[768 + 512];  // [pre | post | epi | range, mirrored]
  __shared__ __attribute__((aligned(16))) uint4 xbuf[EXP ? kWaves : 1][EXP ? 3 * kW : 1];
  if (PRO != PRO_NONE || a.has_epi) load_luts(a, luts);
  for (int i = threadIdx.x; i < 512; i += (int)blockDim.x)  // rng[256 + d] = r[|d|]; entry 0 is never read
    luts[768 + i] = a.luts[768 + (i < 256 ? 256 - i : i - 256) % 256];
  __syncthreads();
  const WaveTask t = wave_task(a);
  if (t.valid)
    ring_task<C, F, PRO, SKIP, SAUX, EXP>(a, t, luts, xbuf[EXP ? t.wave : 0], BilateralRow<C, F>{luts + 768});
}

// Launch geometry and occupancy cap start as for the rank family.
template <int C, class F, int PRO, bool EXP>
void launch_bilateral(bool skip, const KArgs& a, const BandLaunch& B) {
  const KernelFn fns[4] = {k_bilateral<C, F, PRO, false, 0, EXP>, k_bilateral<C, F, PRO, false, kNtAux, EXP>,
                           k_bilateral<C, F, PRO, true, 0, EXP>, k_bilateral<C, F, PRO, true, kNtAux, EXP>};
  launch_bands(fns[2 * skip + B.nt], a, B, F::R, band_cap(B, policy::Family::Bilateral, is_gray(PRO)));
}

}  // namespace dev
}  // namespace stripe
