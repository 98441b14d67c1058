// Rank filter kernels (k_rank: median3/5, erode3/5, dilate3/5) and their launch
// template; instantiated in stencil_inst_e.hip.
#pragma once

// k_rank is the register-ring row walk of k_direct as a device function (ring_task,
// stencil_kernels.h: wave tile, K-row ring of prologue-applied rows as packed
// u16 pairs extended by the neighbour lanes' edge dwords, K rows in flight,
// @skip merge, epilogue, stores and margins) with RankRow as its row operation,
// so bands, the two output ranges and re-based launches need nothing special.
//
// The arithmetic is packed u16 min / max (v_pk_min_u16 / v_pk_max_u16: one
// VALU instruction per two pixels) on the pairs the ring already holds:
//   erode / dilate  one vertical min / max over the K ring rows on the NE
//                   extended dwords, then per output pair a horizontal
//                   min / max over the K shifted pair views;
//   median          the K ring rows are sorted per column once per output row
//                   (ranknet::ColSort on the NE extended dwords: neighbouring
//                   outputs share the sorted columns), then per output pair
//                   the selection network ranknet::Select runs over the K*K
//                   views (sorted column dx, element r).  The networks are
//                   compile-time tables (rank_net.h), unrolled through an
//                   index sequence so every wire is a register.
// A window's order statistics do not depend on the order of its rows, so the
// ring is read as it lies (no slot rotation per unrolled step).

#include <utility>

#include "stencil_kernels.h"
#include "stripe/rank_net.h"

namespace stripe {
namespace dev {

__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b) {
  return as_u32(__builtin_elementwise_min(as_u16x2(a), as_u16x2(b)));
}
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
  return as_u32(__builtin_elementwise_max(as_u16x2(a), as_u16x2(b)));
}

// Step I of a compare-exchange network on the wires w (packed u16 pairs).
template <class Net, int I, int NW>
__device__ __forceinline__ void net_step(uint32_t (&w)[NW]) {
  constexpr ranknet::Step s = Net::at(I);
  static_assert(s.i >= 0 && s.i < s.j && s.j < NW, "network wire out of range");
  const uint32_t a = w[s.i], b = w[s.j];
  if constexpr (s.mode != ranknet::kMax) w[s.i] = pk_min_u16(a, b);
  if constexpr (s.mode != ranknet::kMin) w[s.j] = pk_max_u16(a, b);
}
template <class Net, int NW, size_t... I>
__device__ __forceinline__ void run_net(uint32_t (&w)[NW], std::index_sequence<I...>) {
  (net_step<Net, (int)I>(w), ...);
}
template <class Net, int NW>
__device__ __forceinline__ void run_net(uint32_t (&w)[NW]) {
  run_net<Net>(w, std::make_index_sequence<Net::N>{});
}

// Row operation of the rank filters: the lane's 8 output pairs of one row from
// the K extended ring rows (the unrolled step o is not needed, see above).
template <int C, class F>
struct RankRow {
  static constexpr int NX = RingDims<C, F>::NX, NE = RingDims<C, F>::NE;
  __device__ __forceinline__ void operator()(const uint32_t (&ring)[F::K][NE], int, uint32_t (&h)[8]) const {
    constexpr int K = F::K, R = F::R;
    // u16 index of the window's view dx for output pair pp (as k_direct's taps)
    auto view = [](int pp, int dx) __attribute__((always_inline)) { return 2 * NX + 2 * pp + (dx - R) * C; };
    if constexpr (F::RANK == sdef::kRankMedian) {
      uint32_t s[K][NE];  // s[r]: element r (ascending) of every column
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        uint32_t col[K];
#pragma unroll
        for (int r = 0; r < K; ++r) col[r] = ring[r][e];
        run_net<ranknet::ColSort<K>>(col);
#pragma unroll
        for (int r = 0; r < K; ++r) s[r][e] = col[r];
      }
#pragma unroll
      for (int pp = 0; pp < 8; ++pp) {  // one output pair at a time: K*K live wires
        uint32_t w[K * K];
#pragma unroll
        for (int dx = 0; dx < K; ++dx)
#pragma unroll
          for (int r = 0; r < K; ++r) w[dx * K + r] = pair_at(s[r], view(pp, dx));
        run_net<ranknet::Select<K>>(w);
        h[pp] = w[ranknet::Select<K>::kOut];
      }
    } else {
      constexpr bool kMin = F::RANK == sdef::kRankMin;
      uint32_t v[NE];
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        uint32_t m = ring[0][e];
#pragma unroll
        for (int r = 1; r < K; ++r) m = kMin ? pk_min_u16(m, ring[r][e]) : pk_max_u16(m, ring[r][e]);
        v[e] = m;
      }
#pragma unroll
      for (int pp = 0; pp < 8; ++pp) {
        uint32_t m = pair_at(v, view(pp, 0));
#pragma unroll
        for (int dx = 1; dx < K; ++dx)
          m = kMin ? pk_min_u16(m, pair_at(v, view(pp, dx))) : pk_max_u16(m, pair_at(v, view(pp, dx)));
        h[pp] = m;
      }
    }
  }
};

// K = 5: the sorted columns (K * NE dwords) live beside the ring and the K raw
// rows in flight; 2 waves per SIMD (256 VGPRs) rather than a scratch spill.
template <int C, class F, int PRO, bool SKIP, int SAUX, bool EXP = false>
__global__ __launch_bounds__(kNT, (F::K >= 5 ? 2 : 4)) void k_rank(KArgs a) {
  static_assert(F::RANK != 0, "k_rank runs rank filters");
  __shared__ uint8_t luts[768];
  __shared__ __attribute__((aligned(16))) uint4 xbuf[EXP ? kWaves : 1][EXP ? 3 * kW : 1];
  if (PRO != PRO_NONE || a.has_epi) {
    load_luts(a, luts);
    __syncthreads();
  }
  const WaveTask t = wave_task(a);
  if (t.valid) ring_task<C, F, PRO, SKIP, SAUX, EXP>(a, t, luts, xbuf[EXP ? t.wave : 0], RankRow<C, F>{});
}

// Launch geometry and occupancy cap as for the direct family (plan_bands,
// kNtWgsDirect on HBM-streaming launches without a gray prologue).
template <int C, class F, int PRO, bool EXP>
void launch_rank(bool skip, const KArgs& a, const BandLaunch& B) {
  const KernelFn fns[4] = {k_rank<C, F, PRO, false, 0, EXP>, k_rank<C, F, PRO, false, kNtAux, EXP>,
                           k_rank<C, F, PRO, true, 0, EXP>, k_rank<C, F, PRO, true, kNtAux, EXP>};
  launch_bands(fns[2 * skip + B.nt], a, B, F::R, band_cap(B, policy::Family::Rank, is_gray(PRO)));
}

}  // namespace dev
}  // namespace stripe
