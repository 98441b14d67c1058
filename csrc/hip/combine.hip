// Two-input pointwise pass: out = post(op(X, H)) per byte, X the current image
// and H the held one (filters.h: add, sub, rsub, absdiff, min, max, lincomb,
// above; blend and the unsharp / gradient / top-hat sugar compile to these).
//
// Memory moves as in k_pointwise_flat: each row is a flat byte stream of
// 16-byte groups, kFlatU groups per lane kNT apart, so every load and store
// instruction of a wave covers 1 KiB contiguously and nt stores write whole
// lines.  Both inputs' loads are issued before any arithmetic.  Rows are
// addressed by plain 64-bit pointers (no buffer descriptors, so no 2 GiB
// chunking); launch_pass has checked that whole groups of [0, W * C) lie
// inside all three allocations.  Margins are not processed: in a branched plan
// every stencil fills its own input's margins (Pass::fill_in).
//
// The byte ops work on bytes widened to packed u16 halves (v_pk_add_u16 /
// v_pk_sub_u16 with clamp, v_pk_min / v_pk_max); lincomb forms the i16 pair
// (X, H) of each byte by v_perm, one v_dot2 with (qa, qb) from scalar registers
// accumulates on qc + 2048, and v_ashr_pk_u8_i32 shifts, saturates and packs two
// sums at a time (the arithmetic of k_colormix).  Instances without a post
// table take neither the LDS fill nor its barrier.
#include <algorithm>
#include <cstdlib>

#include "dev_common.h"
#include "stripe/image.h"
#include "stripe/kernels.h"

namespace stripe {
namespace dev {

constexpr int kCombineU = 4;  // 16-byte groups per lane (k_pointwise_flat's kFlatU)

struct CombineArgs {
  const uint8_t* x;     // origin of the current image's stripe
  const uint8_t* h;     // origin of the held image's stripe (pitch in_pitch)
  uint8_t* out;
  const uint8_t* post;  // 256-entry table (LUT instances)
  int64_t in_pitch, out_pitch;
  int ry0;              // first output row of the launch
  int ngroups;          // 16-byte groups per row
  uint32_t qab;         // lincomb: qa | qb << 16 (i16 each)
  int q0;               // lincomb: qc + 2048
  int d;                // above: offset
};

typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 as_u16x2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t as_u32(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }

// One packed pair of widened bytes (values 0..255 in each u16 half).
template <int OP>
__device__ __forceinline__ uint32_t combine_pair(uint32_t x, uint32_t h, int d) {
  const u16x2 X = as_u16x2(x), H = as_u16x2(h);
  const u16x2 k255 = {255, 255};
  if constexpr (OP == (int)CombineKind::Add) {
    return as_u32(__builtin_elementwise_min((u16x2)(X + H), k255));
  } else if constexpr (OP == (int)CombineKind::Sub) {
    return as_u32(__builtin_elementwise_sub_sat(H, X));
  } else if constexpr (OP == (int)CombineKind::RSub) {
    return as_u32(__builtin_elementwise_sub_sat(X, H));
  } else if constexpr (OP == (int)CombineKind::AbsDiff) {
    return as_u32((u16x2)(__builtin_elementwise_max(X, H) - __builtin_elementwise_min(X, H)));
  } else if constexpr (OP == (int)CombineKind::Min) {
    return as_u32(__builtin_elementwise_min(X, H));
  } else if constexpr (OP == (int)CombineKind::Max) {
    return as_u32(__builtin_elementwise_max(X, H));
  } else {
    // Above: H - X + d > 0 ? 255 : 0, both halves at once in one dword.  With
    // A = H + max(d, 0) and B = X + max(-d, 0) (each <= 510), the half
    // 0x8000 + A - B - 1 has bit 15 set exactly when A > B; no half borrows
    // from its neighbour (every half stays within 0x8000 +- 511).
    const uint32_t A = h + (uint32_t)(d > 0 ? d : 0) * 0x00010001u;
    const uint32_t B = x + (uint32_t)(d < 0 ? -d : 0) * 0x00010001u;
    const uint32_t gt = (((A | 0x80008000u) - B - 0x00010001u) >> 15) & 0x00010001u;
    return gt * 255u;
  }
}

// One dword of X and of H -> one output dword.
template <int OP>
__device__ __forceinline__ uint32_t combine_dword(uint32_t x, uint32_t h, const CombineArgs& a) {
  if constexpr (OP == (int)CombineKind::LinComb) {
    int acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      // v_perm selectors: bytes 0..3 of x, 4..7 of h, 0x0c = zero -> i16 pair (X_b, H_b)
      const uint32_t xh = __builtin_amdgcn_perm(h, x, 0x0c000c00u | (uint32_t)b | ((uint32_t)(4 + b) << 16));
      acc[b] = __builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, xh), __builtin_bit_cast(i16x2, a.qab), a.q0, false);
    }
    // floor shift and clamp to u8, two sums per instruction (gfx950 v_ashr_pk_u8_i32)
    const uint32_t lo = __builtin_amdgcn_ashr_pk_u8_i32(acc[0], acc[1], 12);
    const uint32_t hi = __builtin_amdgcn_ashr_pk_u8_i32(acc[2], acc[3], 12);
    return lo | (hi << 16);
  } else {
    const uint32_t m = 0x00FF00FFu;
    const uint32_t even = combine_pair<OP>(x & m, h & m, a.d);                // bytes 0, 2
    const uint32_t odd = combine_pair<OP>((x >> 8) & m, (h >> 8) & m, a.d);  // bytes 1, 3
    return even | (odd << 8);
  }
}

template <int OP, bool NT, bool LUT>
__global__ __launch_bounds__(kNT) void k_combine(CombineArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lut[LUT ? 256 : 4];
  if constexpr (LUT) {
    if (threadIdx.x < 64) reinterpret_cast<uint32_t*>(lut)[threadIdx.x] = reinterpret_cast<const uint32_t*>(a.post)[threadIdx.x];
  }
  const int y = a.ry0 + blockIdx.y;
  const uint8_t* xrow = a.x + (int64_t)y * a.in_pitch;
  const uint8_t* hrow = a.h + (int64_t)y * a.in_pitch;
  uint8_t* drow = a.out + (int64_t)y * a.out_pitch;
  u32x4v vx[kCombineU], vh[kCombineU];
#pragma unroll
  for (int u = 0; u < kCombineU; ++u) {
    const int g = (blockIdx.x * kCombineU + u) * kNT + threadIdx.x;
    if (g < a.ngroups) {
      vx[u] = *reinterpret_cast<const u32x4v*>(xrow + (int64_t)g * 16);
      vh[u] = *reinterpret_cast<const u32x4v*>(hrow + (int64_t)g * 16);
    }
  }
  if constexpr (LUT) __syncthreads();
#pragma unroll
  for (int u = 0; u < kCombineU; ++u) {
    const int g = (blockIdx.x * kCombineU + u) * kNT + threadIdx.x;
    if (g >= a.ngroups) break;
    uint32_t t[4] = {combine_dword<OP>(vx[u].x, vh[u].x, a), combine_dword<OP>(vx[u].y, vh[u].y, a),
                     combine_dword<OP>(vx[u].z, vh[u].z, a), combine_dword<OP>(vx[u].w, vh[u].w, a)};
    if constexpr (LUT) lut16(lut, t);
    // The row's last group may reach up to 15 bytes past W * C into the right
    // margin, and they are stored unmasked (k_pointwise_flat zeroes them under a
    // constant border).  That is correct only because a combine pass exists in
    // branched plans alone, where no consumer trusts its input's margins: every
    // stencil refills them first (Pass::fill_in, chain.cpp).
    const u32x4v o = {t[0], t[1], t[2], t[3]};
    if constexpr (NT) __builtin_nontemporal_store(o, reinterpret_cast<u32x4v*>(drow + (int64_t)g * 16));
    else *reinterpret_cast<u32x4v*>(drow + (int64_t)g * 16) = o;
  }
}

using CombineFn = void (*)(CombineArgs);

template <int OP>
CombineFn combine_instance(bool nt, bool lut) {
  if (nt) return lut ? k_combine<OP, true, true> : k_combine<OP, true, false>;
  return lut ? k_combine<OP, false, true> : k_combine<OP, false, false>;
}

CombineFn combine_kernel(CombineKind k, bool nt, bool lut) {
  switch (k) {
    case CombineKind::Add: return combine_instance<(int)CombineKind::Add>(nt, lut);
    case CombineKind::Sub: return combine_instance<(int)CombineKind::Sub>(nt, lut);
    case CombineKind::RSub: return combine_instance<(int)CombineKind::RSub>(nt, lut);
    case CombineKind::AbsDiff: return combine_instance<(int)CombineKind::AbsDiff>(nt, lut);
    case CombineKind::Min: return combine_instance<(int)CombineKind::Min>(nt, lut);
    case CombineKind::Max: return combine_instance<(int)CombineKind::Max>(nt, lut);
    case CombineKind::LinComb: return combine_instance<(int)CombineKind::LinComb>(nt, lut);
    case CombineKind::Above: return combine_instance<(int)CombineKind::Above>(nt, lut);
    default: break;
  }
  fail("combine: unknown op");
}

}  // namespace dev

void launch_combine(const Pass& p, const PassConsts& pc, const PassLaunch& L, hipStream_t s) {
  using policy::Family;
  STRIPE_CHECK(p.kind == PassKind::Combine && p.cin == p.cout && L.in2 != nullptr, "not a combine launch");
  STRIPE_CHECK((int64_t)L.W * p.cin < (int64_t(1) << 31) - 16, "combine: row of " << L.W << " pixels too wide");
  STRIPE_CHECK(std::abs(p.cq[0]) <= 32767 && std::abs(p.cq[1]) <= 32767, "combine: coefficient outside i16");
  dev::CombineArgs a{};
  a.x = L.in;
  a.h = L.in2;
  a.out = L.out;
  a.post = pc.luts + 256;  // [pre | post | epi]
  a.in_pitch = L.in_pitch;
  a.out_pitch = L.out_pitch;
  a.ngroups = (int)div_up((int64_t)L.W * p.cin, 16);
  a.qab = ((uint32_t)p.cq[0] & 0xFFFFu) | ((uint32_t)p.cq[1] << 16);
  a.q0 = p.cq[2] + 2048;
  a.d = p.cd;
  const policy::RowRanges rr = policy::row_ranges(L.ry, L.nrange);
  const policy::StreamPolicy sp = policy::stream_policy(dev::policy_in(Family::Combine, p, L, rr.rows()));
  const dev::CombineFn fn = dev::combine_kernel(p.comb, sp.nt_stores, p.pro.has_post);
  // the cap as an LDS reservation of the kernel that runs (0: no cap)
  const size_t reserve = nt_lds_reserve((const void*)fn, sp.cap_applied ? sp.cap : 0);
  for (int r = 0; r < L.nrange; ++r) {
    const int y0 = L.ry[2 * r], y1 = L.ry[2 * r + 1];
    if (y1 <= y0) continue;
    a.ry0 = y0;
    const dim3 grid((unsigned)div_up(a.ngroups, dev::kNT * dev::kCombineU), (unsigned)(y1 - y0));
    fn<<<grid, dev::kNT, reserve, s>>>(a);
    HIP_CHECK(hipGetLastError());
  }
}

}  // namespace stripe
