// Rank filter kernels (k_rank: median3/5, erode3/5, dilate3/5) and their launch
// template; instantiated in stencil_inst_e.hip.
#pragma once

// Same wave tile as k_direct (stencil_kernels.h): one wave = 64 lanes x 16
// bytes, 62 output chunks and a halo chunk each side, a K-row register ring of
// prologue-applied rows as packed u16 pairs, extended by the neighbour lanes'
// edge dwords (DPP wave shifts), the y loop unrolled K times with the next K
// raw rows in flight, raw buffer loads / stores with kOOB lane masking, no
// workgroup barrier and no LDS in the row loop.  It reads WaveTask / KArgs the
// same way, so bands, the two output ranges and re-based launches need nothing
// special.
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

// The lane's 8 output pairs of one row from the K extended ring rows.
template <int C, class F, int NX, int NE>
__device__ __forceinline__ void rank_row(const uint32_t (&ring)[F::K][NE], uint32_t (&h)[8]) {
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

// K = 5: the sorted columns (K * NE dwords) live beside the ring and the K raw
// rows in flight; 2 waves per SIMD (256 VGPRs) rather than a scratch spill.
template <int C, class F, int PRO, bool SKIP, int SAUX, bool EXP = false>
__global__ __launch_bounds__(kNT, (F::K >= 5 ? 2 : 4)) void k_rank(KArgs a) {
  static_assert(!EXP || C == 1, "expand epilogue needs a 1-channel stencil");
  static_assert(F::RANK != 0, "k_rank runs rank filters");
  constexpr int R = F::R, K = F::K;
  constexpr int NX = (R * C + 1) / 2;  // neighbour dwords per side
  constexpr int NE = 8 + 2 * NX;       // extended row dwords
  constexpr int CIN = is_gray(PRO) ? 3 : 1;
  __shared__ uint8_t luts[768];
  if (PRO != PRO_NONE || a.has_epi) {
    load_luts<PRO>(a, luts);
    __syncthreads();
  }
  const WaveTask t = wave_task(a);
  if (!t.valid) return;
  const int lane = t.lane;
  const int ys = t.ys, ye = t.ye;
  const int cb = tile_base<C>(a, t.xt, kOutChunks * 16) - 16 + lane * 16;
  const uint32_t lane_in = cb < a.E + 16 ? (uint32_t)(cb * CIN) : kOOB;
  const OutLanes lout = out_lanes<EXP>(a, lane, cb - 16 * lane);
  const __amdgpu_buffer_rsrc_t rin = make_rsrc(a.in_base, a.in_bytes);
  const __amdgpu_buffer_rsrc_t rout = make_rsrc(a.out_base, a.out_bytes);
  const uint32_t last_row = in_row_off(a, ye - 1 + R);
  __shared__ __attribute__((aligned(16))) uint4 xbuf[EXP ? kWaves : 1][EXP ? 3 * kW : 1];
  uint4* xb = xbuf[EXP ? t.wave : 0];

  uint32_t keep[SKIP ? 4 : 1];
  if constexpr (SKIP) skip_cols<C>(a, cb, R, keep);
  uint32_t ring[K][NE];  // slot of input row r: (r - (ys - R)) mod K
  auto push = [&](const RawChunk<PRO>& raw, uint32_t (&slot)[NE]) __attribute__((always_inline)) {
    uint32_t u[8];
    cook_pairs<PRO>(a, raw, luts, u);
    extend_row<NX>(u, slot);
  };
#pragma unroll
  for (int i = 0; i < K - 1; ++i) {  // rows ys-R .. ys+R-1
    RawChunk<PRO> r;
    load_raw<PRO>(rin, in_row_off(a, ys - R + i), lane_in, r);
    push(r, ring[i]);
  }
  RawChunk<PRO> nx[K];  // row y + o + R for the step o of the current round
#pragma unroll
  for (int o = 0; o < K; ++o) load_raw<PRO>(rin, ys + o < ye ? in_row_off(a, ys + o + R) : last_row, lane_in, nx[o]);

  const bool inner = rows_inside(a, ys - R, ye - 1 + R);
  for (int y = ys; y < ye; y += K) {
#pragma unroll
    for (int o = 0; o < K; ++o) {
      const int yy = y + o;
      push(nx[o], ring[(o + K - 1) % K]);
      load_raw<PRO>(rin, ahead_row_off(a, inner, yy, K, ye, R, last_row), lane_in, nx[o]);
      uint32_t h[8];
      rank_row<C, F, NX, NE>(ring, h);
      uint32_t o4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) o4[q] = __builtin_amdgcn_perm(h[2 * q + 1], h[2 * q], 0x06040200u);
      if constexpr (SKIP) {
        uint32_t center[4];
        const uint32_t(&cr)[NE] = ring[(o + R) % K];
#pragma unroll
        for (int q = 0; q < 4; ++q) center[q] = __builtin_amdgcn_perm(cr[NX + 2 * q + 1], cr[NX + 2 * q], 0x06040200u);
        apply_skip(a, a.row0 + yy, R, keep, center, o4);
      }
      if (a.has_epi) lut16(luts + 512, o4);
      store_out<EXP, SAUX>(o4, rout, yy < ye, a.out_org + (uint32_t)((int64_t)yy * a.out_pitch), lout, xb, lane);
    }
  }
  band_margins<C, EXP ? 3 : C>(a, t);
}

// Launch geometry and occupancy cap as for the direct family (plan_bands,
// kNtWgsDirect on HBM-streaming launches without a gray prologue).
template <int C, class F, int PRO, bool EXP>
void launch_rank(bool skip, bool nt, int wgs, KArgs a, int tiles, int n0, int n1, int band, hipStream_t s) {
  using K = void (*)(KArgs);
  const K fns[4] = {k_rank<C, F, PRO, false, 0, EXP>, k_rank<C, F, PRO, false, kNtAux, EXP>,
                    k_rank<C, F, PRO, true, 0, EXP>, k_rank<C, F, PRO, true, kNtAux, EXP>};
  const K fn = fns[2 * skip + nt];
  dim3 grid;
  plan_bands(a, grid, tiles, n0, n1, band, F::R, resident_slots((const void*)fn));
  fn<<<grid, kNT, nt_lds_reserve((const void*)fn, stencil_cap(nt, wgs, is_gray(PRO) ? 0 : kNtWgsDirect)), s>>>(a);
}

}  // namespace dev
}  // namespace stripe
