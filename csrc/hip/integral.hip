// Integral images on the device (k_sat_*).  The rule is stripe/integral.h's; the
// tables and every window operation are bit-identical to the golden functions.
//
// The table is that of the frame extended by R = K / 2 on every side with the
// border, (He + 1) x (We + 1) wrapping u32 with We = W + 2R, He = H + 2R, row 0
// and column 0 zero (R = 0: the public integral, written straight into the
// caller's int32 plane).  The extension is an index map applied at load time
// (border_index per lane for its column, per row for the wave); a padded copy of
// the image is never stored.  Reduce, carry, scan, all queued on the caller's
// stream, none waited for, no workgroup ever waiting for another:
//
//   k_sat_reduce<MODE>  a wave owns a tile of kSatTile x kSatTile = 64 x 64
//                pixels of the extended frame, a lane one column; a workgroup is
//                kSatWaves = 4 such tiles side by side.  It walks the rows and
//                writes the tile's column totals (one per lane), its row totals
//                (a DPP wave reduction per row, stored by the last lane) and its
//                total.  MODE 0: sums, 1: squares, 2: both from one read.
//   k_sat_carry<NTAB>   three kinds of workgroup over those aggregates: a lane
//                per column walks the tile rows down (the sum of the column above
//                each tile), a lane per row walks the tile columns across (the sum
//                of the row left of each tile), and one workgroup turns the tile
//                totals into the sum above and left of each tile (down, a
//                barrier, across; through a temporary so that no pass is in
//                place and the loads of a walk are independent).
//   k_sat_scan<MODE>    the same tiles and the same reads of the source: a lane
//                keeps the running sum of its column, a DPP wave scan per row turns
//                those into the tile-local table row, and the row is stored as
//                64 consecutive dwords after adding the wave scan of the column
//                carries, the running sum of the row carries and the corner.
//                No LDS: a wave's tile needs nothing from its neighbours once
//                the carries are 64 columns fine (4 B per 64 pixels each way).
//   k_sat_window<OP>    a lane per 4 pixels of a row: the source bytes and per
//                table two rows at two x offsets, 16 bytes each (the offsets
//                x and x + K: one aligned, one at any dword), then window_rule
//                and one dword store (single bytes on unaligned views and at a
//                ragged row end).  The division by N is the plain u32 division.
//
// Traffic per pixel and table: 1 B + 1 B of source, 4 B of table and 3 * 4 / 64 B
// of aggregates written and read twice.
//
// Every loop's trip count is bounded by W, H, K or a constant: a tile's rows by
// kSatTile, the carry walks by the tile counts (He / 64 + 1, We / 64 + 1; the
// corner workgroup's strides by those over kNT), the window kernel has no loop
// but the 4 pixels of a lane.
//
// Arithmetic is wrapping u32 in the tables and aggregates; window sums are
// exact because the K limits keep them below 2^32 (stripe/integral.h).
//
// Scratch per (device, stream, We, He, tables), cached, released by
// integral_release_scratch: the aggregates, and for the window operations the
// tables.  Launch policy: default stores, no residency cap (none was measured
// to pay; launch_policy.h has no entry for this family).
//
// Addressing as k_orient / k_edt: 64-bit on pitched views, any source pitch >= W
// at any alignment, no byte outside a source row's W bytes read, nothing outside
// a destination row's elements written.
#include <array>
#include <list>
#include <mutex>

#include "dev_common.h"
#include "stripe/integral.h"
#include "stripe/kernels.h"

namespace stripe {
namespace dev {

struct SatArgs {
  const uint8_t* src;
  int64_t sp;  // bytes
  int W, H, R, border;
  int We, He;    // the extended frame
  int ntx, nty;  // wave tiles across and down
  // per table: column totals nty x We, row totals ntx x He, tile totals nty x ntx, and their carries
  uint32_t* col[2];
  uint32_t* row[2];
  uint32_t* tile[2];
  uint32_t* colx[2];
  uint32_t* rowx[2];
  uint32_t* tmp[2];
  uint32_t* corner[2];
  uint32_t* tab[2];
  int64_t tp;  // elements of a table row
};

template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
  // lanes without a source lane, and the rows ROWS masks out, add 0
  return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xF, false);
}

// Inclusive sum over the 64 lanes of a wave; every lane must be active.
__device__ __forceinline__ uint32_t wave_scan(uint32_t v) {
  v = dpp_add<0x111, 0xF>(v);  // row_shr:1 .. 8: the scan of each row of 16 lanes
  v = dpp_add<0x112, 0xF>(v);
  v = dpp_add<0x114, 0xF>(v);
  v = dpp_add<0x118, 0xF>(v);
  v = dpp_add<0x142, 0xA>(v);  // row_bcast:15 into rows 1 and 3
  v = dpp_add<0x143, 0xC>(v);  // row_bcast:31 into rows 2 and 3
  return v;
}

constexpr int sat_tables(int mode) { return mode == 2 ? 2 : 1; }
template <int MODE>
__device__ __forceinline__ uint32_t sat_value(uint32_t p, int t) {
  return MODE == 0 || (MODE == 2 && t == 0) ? p : p * p;
}

// the byte of extended row y (uniform) in this lane's column: sx < 0 for a column that is zero
__device__ __forceinline__ uint32_t sat_load(const SatArgs& a, int y, int sx) {
  const int sy = border_index_dev(y - a.R, a.H, a.border);
  return sy >= 0 && sx >= 0 ? (uint32_t)a.src[(int64_t)sy * a.sp + sx] : 0u;
}

template <int MODE>
__global__ __launch_bounds__(kSatWaves * 64) void k_sat_reduce(SatArgs a) {
  constexpr int NT = sat_tables(MODE);
  const int lane = threadIdx.x & 63, tx = (int)blockIdx.x * kSatWaves + (int)(threadIdx.x >> 6), ty = blockIdx.y;
  if (tx >= a.ntx) return;  // the whole wave
  const int x = tx * kSatTile + lane, y0 = ty * kSatTile;
  const int rows = min(kSatTile, a.He - y0);
  const int sx = x < a.We ? border_index_dev(x - a.R, a.W, a.border) : -1;
  uint32_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = 0;
  // a constant trip count (the loads of several rows then go out together); rows past the frame count as zero
#pragma unroll 4
  for (int r = 0; r < kSatTile; ++r) {
    const bool in = r < rows;
    const uint32_t p = in ? sat_load(a, y0 + r, sx) : 0u;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint32_t v = sat_value<MODE>(p, t);
      acc[t] += v;
      const uint32_t s = wave_scan(v);
      if (in && lane == 63) a.row[t][(int64_t)tx * a.He + y0 + r] = s;
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const uint32_t s = wave_scan(acc[t]);
    if (x < a.We) a.col[t][(int64_t)ty * a.We + x] = acc[t];
    if (lane == 63) a.tile[t][(int64_t)ty * a.ntx + tx] = s;
  }
}

// out[i * stride] for i < n: the sum of in[j * stride] over j < i
__device__ __forceinline__ void sat_walk(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n,
                                         int64_t stride) {
  uint32_t run = 0;
#pragma unroll 8
  for (int i = 0; i < n; ++i) {
    const uint32_t v = in[i * stride];
    out[i * stride] = run;
    run += v;
  }
}

template <int NTAB>
__global__ __launch_bounds__(kNT) void k_sat_carry(SatArgs a, int nbc, int nbr) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b < nbc) {
    const int x = b * kNT + tid;
    if (x < a.We)
      for (int t = 0; t < NTAB; ++t) sat_walk(a.col[t] + x, a.colx[t] + x, a.nty, a.We);
  } else if (b < nbc + nbr) {
    const int y = (b - nbc) * kNT + tid;
    if (y < a.He)
      for (int t = 0; t < NTAB; ++t) sat_walk(a.row[t] + y, a.rowx[t] + y, a.ntx, a.He);
  } else {
    for (int t = 0; t < NTAB; ++t)
      for (int u = tid; u < a.ntx; u += kNT) sat_walk(a.tile[t] + u, a.tmp[t] + u, a.nty, a.ntx);
    __syncthreads();  // this workgroup's own stores, read by its own lanes
    for (int t = 0; t < NTAB; ++t)
      for (int v = tid; v < a.nty; v += kNT)
        sat_walk(a.tmp[t] + (int64_t)v * a.ntx, a.corner[t] + (int64_t)v * a.ntx, a.ntx, 1);
  }
}

template <int MODE>
__global__ __launch_bounds__(kSatWaves * 64) void k_sat_scan(SatArgs a) {
  constexpr int NT = sat_tables(MODE);
  const int lane = threadIdx.x & 63, tx = (int)blockIdx.x * kSatWaves + (int)(threadIdx.x >> 6), ty = blockIdx.y;
  if (tx >= a.ntx) return;  // the whole wave
  const int x = tx * kSatTile + lane, y0 = ty * kSatTile;
  const int rows = min(kSatTile, a.He - y0);
  const bool live = x < a.We;
  const int sx = live ? border_index_dev(x - a.R, a.W, a.border) : -1;
  uint32_t acc[NT], base[NT], left[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc[t] = 0, left[t] = 0;
    // the rows above the tile: every column left of the wave, then the wave's columns up to this one
    base[t] = a.corner[t][(int64_t)ty * a.ntx + tx] + wave_scan(live ? a.colx[t][(int64_t)ty * a.We + x] : 0u);
    if (ty == 0 && live) a.tab[t][x + 1] = 0;
    if (ty == 0 && tx == 0 && lane == 0) a.tab[t][0] = 0;
  }
#pragma unroll 4
  for (int r = 0; r < kSatTile; ++r) {  // a constant trip count, as in k_sat_reduce
    const int y = y0 + r;
    const bool in = r < rows;
    const uint32_t p = in ? sat_load(a, y, sx) : 0u;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc[t] += sat_value<MODE>(p, t);
      left[t] += in ? a.rowx[t][(int64_t)tx * a.He + y] : 0u;  // uniform: the tile's rows so far, left of the wave
      const uint32_t s = wave_scan(acc[t]) + base[t] + left[t];
      uint32_t* o = a.tab[t] + (int64_t)(y + 1) * a.tp;
      if (in && live) o[x + 1] = s;
      if (in && tx == 0 && lane == 0) o[0] = 0;
    }
  }
}

struct WinArgs {
  const uint8_t* src;
  int64_t sp;
  uint8_t* dst;
  int64_t dp;
  const uint32_t* ta;  // sums
  const uint32_t* tb;  // squares (the operations that read B)
  int64_t tp;
  int W, H, K;
  uint32_t N;
  int C, kq;
  int src_al, dst_al;  // the view is aligned to 4 bytes (base and pitch)
};

struct __attribute__((packed, aligned(4))) Dwords4 {
  uint32_t v[4];
};

// the window sums of pixels x .. x + 3 of row y from a table: rows y and y + K at the offsets x and x + K
__device__ __forceinline__ void sat_corners(const uint32_t* t, int64_t tp, int y, int x, int K, uint32_t (&s)[4]) {
  const uint32_t* r0 = t + (int64_t)y * tp + x;
  const uint32_t* r1 = r0 + (int64_t)K * tp;
  const uint4 a = *reinterpret_cast<const uint4*>(r0), c = *reinterpret_cast<const uint4*>(r1);
  const Dwords4 b = *reinterpret_cast<const Dwords4*>(r0 + K), d = *reinterpret_cast<const Dwords4*>(r1 + K);
  s[0] = d.v[0] - b.v[0] - c.x + a.x;
  s[1] = d.v[1] - b.v[1] - c.y + a.y;
  s[2] = d.v[2] - b.v[2] - c.z + a.z;
  s[3] = d.v[3] - b.v[3] - c.w + a.w;
}

template <int OP>
__global__ __launch_bounds__(kNT) void k_sat_window(WinArgs a) {
  const int x = 4 * (int)(blockIdx.x * kNT + threadIdx.x), y = blockIdx.y;
  if (x >= a.W) return;
  constexpr bool kSquares = OP == (int)WindowOp::Std || OP == (int)WindowOp::Niblack || OP == (int)WindowOp::Sauvola;
  constexpr bool kPixel = OP != (int)WindowOp::Box && OP != (int)WindowOp::Std;
  const bool whole = x + 4 <= a.W;
  uint32_t A[4], B[4] = {0, 0, 0, 0}, p[4] = {0, 0, 0, 0};
  sat_corners(a.ta, a.tp, y, x, a.K, A);
  if (kSquares) sat_corners(a.tb, a.tp, y, x, a.K, B);
  if (kPixel) {
    const uint8_t* r = a.src + (int64_t)y * a.sp + x;
    if (a.src_al && whole) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(r);
      p[0] = v & 0xFFu, p[1] = (v >> 8) & 0xFFu, p[2] = (v >> 16) & 0xFFu, p[3] = v >> 24;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (x + i < a.W) p[i] = r[i];
    }
  }
  uint32_t o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = window_rule(OP, p[i], A[i], B[i], a.N, a.C, a.kq);
  uint8_t* w = a.dst + (int64_t)y * a.dp + x;
  if (a.dst_al && whole) {
    *reinterpret_cast<uint32_t*>(w) = pack4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x + i < a.W) w[i] = (uint8_t)o[i];
  }
}

}  // namespace dev

namespace {

constexpr size_t kAlign = 256;
size_t aligned(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

// Per device, stream, extended size and number of tables: work queued on one stream runs in order, so two calls
// never use one buffer at a time.  The lock is held while a call enqueues, so that no buffer is freed between its
// lookup and its launches (hipFree waits for the device).
struct SatScratch {
  std::array<int64_t, 5> key{};  // device, stream, We, He, tables
  uint8_t* agg = nullptr;        // the aggregates and their carries
  uint8_t* tab = nullptr;        // the window operations' tables, on demand
};
constexpr size_t kMaxScratch = 4;
std::mutex g_sat_mu;
std::list<SatScratch>& sat_cache() {
  static std::list<SatScratch>* cache = new std::list<SatScratch>;  // never destroyed before the runtime
  return *cache;
}

int sat_tiles(int n) { return (int)div_up(n, kSatTile); }
int64_t sat_table_pitch(int We) { return div_up((int64_t)We + 1 + 3, 4) * 4; }  // a lane reads 4 dwords from x + K

struct SatSizes {
  size_t col, row, tile;  // bytes of one array, aligned
  size_t agg() const { return 2 * col + 2 * row + 3 * tile; }
};
SatSizes sat_sizes(int We, int He) {
  const size_t ntx = (size_t)sat_tiles(We), nty = (size_t)sat_tiles(He);
  return {aligned(nty * (size_t)We * 4), aligned(ntx * (size_t)He * 4), aligned(nty * ntx * 4)};
}

SatScratch& sat_scratch(int We, int He, int ntab, hipStream_t s, bool need_tab) {
  std::list<SatScratch>& cache = sat_cache();
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  const std::array<int64_t, 5> key{dev, (int64_t) reinterpret_cast<intptr_t>(s), We, He, ntab};
  auto hit = cache.end();
  for (auto it = cache.begin(); it != cache.end(); ++it)
    if (it->key == key) hit = it;
  if (hit != cache.end()) {
    cache.splice(cache.begin(), cache, hit);
  } else {
    while (cache.size() >= kMaxScratch) {
      (void)hipFree(cache.back().agg);
      (void)hipFree(cache.back().tab);
      cache.pop_back();
    }
    SatScratch t;
    t.key = key;
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t.agg), (size_t)ntab * sat_sizes(We, He).agg()));
    cache.push_front(t);
  }
  SatScratch& e = cache.front();
  if (need_tab && !e.tab)
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e.tab),
                        (size_t)ntab * aligned((size_t)sat_table_pitch(We) * ((size_t)He + 1) * 4)));
  return e;
}

// reduce, carry, scan of mode (0 sums, 1 squares, 2 both) into tab[] with row pitch tp; the caller holds g_sat_mu
void enqueue_tables(const uint8_t* src, int64_t sp, int W, int H, int R, Border border, int mode, SatScratch& e,
                    uint32_t* const (&tab)[2], int64_t tp, hipStream_t s) {
  const int ntab = mode == 2 ? 2 : 1;
  dev::SatArgs a{};
  a.src = src, a.sp = sp;
  a.W = W, a.H = H, a.R = R, a.border = (int)border;
  a.We = W + 2 * R, a.He = H + 2 * R;
  a.ntx = sat_tiles(a.We), a.nty = sat_tiles(a.He);
  const SatSizes z = sat_sizes(a.We, a.He);
  uint8_t* p = e.agg;
  const auto take = [&p](size_t n) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    p += n;
    return q;
  };
  for (int t = 0; t < ntab; ++t) {
    a.col[t] = take(z.col), a.colx[t] = take(z.col);
    a.row[t] = take(z.row), a.rowx[t] = take(z.row);
    a.tile[t] = take(z.tile), a.tmp[t] = take(z.tile), a.corner[t] = take(z.tile);
    a.tab[t] = tab[t];
  }
  a.tp = tp;
  const dim3 tiles((unsigned)div_up(a.ntx, kSatWaves), (unsigned)a.nty), block(kSatWaves * 64);
  const int nbc = (int)div_up(a.We, dev::kNT), nbr = (int)div_up(a.He, dev::kNT);
  const dim3 carry((unsigned)(nbc + nbr + 1));
  switch (mode) {
    case 0:
      dev::k_sat_reduce<0><<<tiles, block, 0, s>>>(a);
      dev::k_sat_carry<1><<<carry, dim3(dev::kNT), 0, s>>>(a, nbc, nbr);
      dev::k_sat_scan<0><<<tiles, block, 0, s>>>(a);
      break;
    case 1:
      dev::k_sat_reduce<1><<<tiles, block, 0, s>>>(a);
      dev::k_sat_carry<1><<<carry, dim3(dev::kNT), 0, s>>>(a, nbc, nbr);
      dev::k_sat_scan<1><<<tiles, block, 0, s>>>(a);
      break;
    default:
      dev::k_sat_reduce<2><<<tiles, block, 0, s>>>(a);
      dev::k_sat_carry<2><<<carry, dim3(dev::kNT), 0, s>>>(a, nbc, nbr);
      dev::k_sat_scan<2><<<tiles, block, 0, s>>>(a);
      break;
  }
  HIP_CHECK(hipGetLastError());
}

template <int OP>
void launch_window_op(const dev::WinArgs& w, hipStream_t s) {
  dev::k_sat_window<OP><<<dim3((unsigned)div_up(w.W, 4 * dev::kNT), (unsigned)w.H), dim3(dev::kNT), 0, s>>>(w);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

void launch_integral_kernels(const IntegralLaunch& L, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_sat_mu);
  SatScratch& e = sat_scratch(L.W, L.H, 1, s, false);
  uint32_t* const tab[2] = {reinterpret_cast<uint32_t*>(L.dst), nullptr};
  enqueue_tables(L.src, L.src_pitch, L.W, L.H, 0, Border::Constant, L.squared ? 1 : 0, e, tab, L.dst_pitch, s);
}

void launch_window_kernels(const WindowLaunch& L, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_sat_mu);
  const WindowOp op = (WindowOp)L.op;
  const int R = L.K / 2, We = L.W + 2 * R, He = L.H + 2 * R;
  const bool sq = window_uses_squares(op);
  SatScratch& e = sat_scratch(We, He, sq ? 2 : 1, s, true);
  const int64_t tp = sat_table_pitch(We);
  const size_t tbytes = aligned((size_t)tp * ((size_t)He + 1) * 4);
  uint32_t* const tab[2] = {reinterpret_cast<uint32_t*>(e.tab), sq ? reinterpret_cast<uint32_t*>(e.tab + tbytes) : nullptr};
  enqueue_tables(L.src, L.src_pitch, L.W, L.H, R, (Border)L.border, sq ? 2 : 0, e, tab, tp, s);
  dev::WinArgs w{};
  w.src = L.src, w.sp = L.src_pitch;
  w.dst = L.dst, w.dp = L.dst_pitch;
  w.ta = tab[0], w.tb = tab[1], w.tp = tp;
  w.W = L.W, w.H = L.H, w.K = L.K;
  w.N = (uint32_t)L.K * (uint32_t)L.K;
  w.C = L.C, w.kq = (int)L.kq;
  w.src_al = ((reinterpret_cast<uintptr_t>(L.src) | (uintptr_t)L.src_pitch) & 3) == 0;
  w.dst_al = ((reinterpret_cast<uintptr_t>(L.dst) | (uintptr_t)L.dst_pitch) & 3) == 0;
  switch (op) {
    case WindowOp::Box: launch_window_op<(int)WindowOp::Box>(w, s); break;
    case WindowOp::Std: launch_window_op<(int)WindowOp::Std>(w, s); break;
    case WindowOp::Mean: launch_window_op<(int)WindowOp::Mean>(w, s); break;
    case WindowOp::Niblack: launch_window_op<(int)WindowOp::Niblack>(w, s); break;
    case WindowOp::Sauvola: launch_window_op<(int)WindowOp::Sauvola>(w, s); break;
  }
}

void integral_release_scratch() {
  std::lock_guard<std::mutex> lk(g_sat_mu);
  for (SatScratch& e : sat_cache()) {
    (void)hipFree(e.agg);
    (void)hipFree(e.tab);
  }
  sat_cache().clear();
}

void integral_device(const uint8_t* src, int64_t src_pitch, int W, int H, bool squared, int32_t* dst, int64_t dst_pitch,
                     hipStream_t s) {
  IntegralLaunch L;
  L.src = src, L.src_pitch = src_pitch;
  L.W = W, L.H = H, L.squared = squared;
  L.dst = dst, L.dst_pitch = dst_pitch;
  launch_integral(L, s);
}

void window_device(const uint8_t* src, int64_t src_pitch, int W, int H, int op, int K, int border, int C, int64_t kq,
                   uint8_t* dst, int64_t dst_pitch, hipStream_t s) {
  WindowLaunch L;
  L.src = src, L.src_pitch = src_pitch;
  L.W = W, L.H = H;
  L.op = op, L.K = K, L.border = border, L.C = C, L.kq = kq;
  L.dst = dst, L.dst_pitch = dst_pitch;
  launch_window(L, s);
}

}  // namespace stripe
