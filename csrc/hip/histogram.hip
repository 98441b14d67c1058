// Histogram of a stripe's own rows: 256 counts per channel, exact.
//
// The first pass of the project that reduces over an image (the statistic ops
// equalize / autocontrast / threshold:otsu build their table from it).  It is
// read-only and moves memory as k_pointwise_flat does: a row is a flat byte
// stream of 16-byte groups, one group per lane, so every load instruction of a
// wave covers 1 KiB contiguously; a wave takes kHistU such instructions per
// step (4 KiB in flight).  The grid is persistent (sized from the CU count)
// and the waves stride over the (row, 4 KiB span) tasks.
//
// Every wave counts into a private 256 x C u32 table in LDS (3 KiB for RGB)
// with non-returning LDS atomic adds; the workgroup's tables are summed once
// and the non-zero sums go to the 256 x C u32 device table with integer global
// atomics.  Integer adds only: the counts are exact and independent of arrival
// order.  In RGB, byte j of group g is channel (g + j) % 3 (16 % 3 == 1).
// Bytes of a row beyond W * C (the right margin, pitch padding) are masked; a
// lane whose group lies wholly outside issues no load.
#include <map>
#include <mutex>

#include "dev_common.h"
#include "stripe/kernels.h"

namespace stripe {
namespace dev {

constexpr int kHistU = 4;           // 16-byte groups per lane and step
constexpr int kHistWaves = kNT / 64;

template <int C>
__global__ __launch_bounds__(kNT) void k_hist(const uint8_t* in, int64_t pitch, int E, int tpr, int ntasks,
                                              uint32_t* bins) {
  constexpr int NB = 256 * C;
  __shared__ uint32_t tab[kHistWaves * NB];
  for (int i = threadIdx.x; i < kHistWaves * NB; i += kNT) tab[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t* t = tab + wave * NB;
  const int ng = (E + 15) >> 4;  // 16-byte groups that hold row bytes
  typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
  for (int task = blockIdx.x * kHistWaves + wave; task < ntasks; task += gridDim.x * kHistWaves) {
    const int y = task / tpr;
    const int g0 = (task - y * tpr) * (64 * kHistU) + lane;
    const uint8_t* row = in + (int64_t)y * pitch;
    u32x4v v[kHistU];
#pragma unroll
    for (int u = 0; u < kHistU; ++u) {
      const int g = g0 + 64 * u;
      v[u] = u32x4v{0, 0, 0, 0};
      if (g < ng) v[u] = *reinterpret_cast<const u32x4v*>(row + (int64_t)g * 16);
    }
#pragma unroll
    for (int u = 0; u < kHistU; ++u) {
      const int g = g0 + 64 * u;
      if (g >= ng) break;
      const int nvalid = min(16, E - g * 16);  // < 16 only in a row's last group
      // table of the channel of byte j: (g + j) % 3 in RGB
      uint32_t* tc[3] = {t, t, t};
      if constexpr (C == 3) {
        const int c0 = g % 3;
        tc[0] = t + 256 * c0;
        tc[1] = t + 256 * (c0 == 2 ? 0 : c0 + 1);
        tc[2] = t + 256 * (c0 == 0 ? 2 : c0 - 1);
      }
      const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        if (j < nvalid)
          (void)__hip_atomic_fetch_add(tc[j % 3] + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NB; i += kNT) {
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kHistWaves; ++k) s += tab[k * NB + i];
    if (s) (void)__hip_atomic_fetch_add(bins + i, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace dev

namespace {
int cu_count() {
  static std::mutex mu;
  static std::map<int, int> cache;
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(dev);
  if (it != cache.end()) return it->second;
  int cus = 0;
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  cache[dev] = std::max(1, cus);
  return cache[dev];
}
}  // namespace

void launch_hist_kernel(const HistLaunch& L, hipStream_t s) {
  if (L.rows <= 0) return;
  const int E = L.W * L.C;
  const int ng = (int)div_up(E, 16);
  const int tpr = (int)div_up(ng, 64 * dev::kHistU);  // wave tasks per row
  const int64_t ntasks = (int64_t)L.rows * tpr;
  STRIPE_CHECK(ntasks < (int64_t(1) << 31), "histogram: too many wave tasks");
  // persistent grid: at most 8 workgroups (32 waves, 8 x 12 KiB of LDS) per CU,
  // and at least kMinSteps steps per wave, so that a workgroup's flush (up to
  // 768 global atomics on the same 768 words as every other workgroup's) is
  // spread over 128 KiB of input or more.  Measured (profiles/histogram/):
  // 16384^2 RGB 0.296 ms at 2 per CU, 0.210 at 8; 4096^2 RGB 0.048 at 2, 0.068 at 8
  constexpr int kMinSteps = 8;
  const unsigned grid = (unsigned)std::min<int64_t>(div_up(ntasks, dev::kHistWaves * kMinSteps), (int64_t)cu_count() * 8);
  if (L.C == 1) dev::k_hist<1><<<grid, dev::kNT, 0, s>>>(L.in, L.pitch, E, tpr, (int)ntasks, L.bins);
  else dev::k_hist<3><<<grid, dev::kNT, 0, s>>>(L.in, L.pitch, E, tpr, (int)ntasks, L.bins);
  HIP_CHECK(hipGetLastError());
}

}  // namespace stripe
