// Connected components on the device (k_ccl_*).  The rule is
// stripe/components.h's; labels, N, the statistics and the area filter are
// bit-identical to the golden functions.
//
// The label plane itself is the union-find forest: while a call runs, a slot
// holds 0 (background) or its parent's raster index + 1, and a root holds its
// own.  A parent never has a larger raster index than its child, so a
// component's root is its first pixel in raster order and the numbering falls
// out of a count of the roots.  The passes of components_device, all on the
// caller's stream:
//
//   k_ccl_tile     one workgroup per kCclTile x kCclTile tile.  The tile's
//                  foreground goes to LDS as local raster indices (u32: LDS
//                  atomics are 32 bits wide; ccl_lds_bytes()), every foreground
//                  pixel unites with its W, N (NW, NE) neighbours inside the
//                  tile by LDS atomicMin, and after a barrier every pixel
//                  stores the global index of its local root + 1.  Local raster
//                  order agrees with the global one inside a tile.
//   k_ccl_seam     one thread per pixel of a tile's first row or first column:
//                  the links that cross into another tile, by global union-find
//                  on the label plane (find with path halving, link by
//                  atomicMin of the larger root onto the smaller).
//   k_ccl_flatten  every pixel takes its root; the roots (slot == own index + 1)
//                  are counted per row (__ballot / __popcll, one add a wave).
//                  (These three are the forest passes; launch_ccl_forest queues them
//                  alone for the hysteresis of canny.hip, which needs no numbers.)
//   k_ccl_scan     one workgroup: the exclusive prefix of the H row counts, in
//                  place, H + 1 entries; the last is N.
//   k_ccl_number   one workgroup per row: a root's number is the row's prefix
//                  plus the roots before it in the row, plus 1; the root's own
//                  slot takes MINUS that number (no second label plane).
//   k_ccl_resolve  every pixel takes the number in its root's slot (a root
//                  turns its own -n into n; a reader takes |slot|, so the
//                  order of the two does not matter).
//
// component_stats_device: k_ccl_stats_init, k_ccl_stats (a wave per kCclStatSeg
// pixels of a row; see there), k_ccl_stats_fix (an empty label's minima become
// 0).  area_filter_device: k_ccl_select, a pixel per lane gathering area[label].
//
// Links that other links imply are left out (both kernels, same rule): W links
// are always made; an N link is left out when the W neighbours of both ends are
// foreground (the W neighbour's N link and the two W links imply it); NW is
// made only when neither W nor N is foreground, NE only when neither N nor E is.
//
// Device memory of a call beyond the label plane: (H + 3) u32 (row prefix, N,
// error word), cached per device and H.  A call holds the cache's lock until
// its one host synchronisation (the read-back of N and the error word).
//
// Every find / link loop ends: parents strictly decrease along a chain and a
// link only ever lowers a slot.  Each loop also counts its steps against
// W * H + 2, more than the longest strictly decreasing chain; on overrun the
// thread sets the error word and stops, and the host raises after the
// synchronisation.
//
// Addressing as k_orient: 64-bit on pitched views, any source pitch >= W at any
// alignment, no byte outside a source row's W bytes read, nothing outside a
// label row's W ints written.
#include <array>
#include <climits>
#include <list>
#include <mutex>

#include "dev_common.h"
#include "stripe/components.h"
#include "stripe/kernels.h"

namespace stripe {
namespace dev {

struct CclArgs {
  const uint8_t* src;
  int32_t* lab;
  int64_t sp, lp;    // pitches: bytes, elements
  int W, H;
  int ntx;           // tiles / segments per row
  int conn8;
  uint32_t cap;      // step cap of every find / link loop: W * H + 2
  uint32_t* rows;    // H + 1 row counts / prefixes, then N, then the error word
  uint32_t* err;
};

constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ __forceinline__ void set_err(uint32_t* err) { atomicOr(err, 1u); }

// ---- the tile's forest in LDS: P[l] is the parent's local index, a root its own, kNone background ----
__device__ __forceinline__ uint32_t lds_find(uint32_t* P, uint32_t i, uint32_t cap, uint32_t* err) {
  // ends: P[i] < i for every non-root and slots only decrease, so i strictly decreases; capped all the same
  for (uint32_t step = 0;; ++step) {
    const uint32_t p = __hip_atomic_load(P + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == i) return i;
    const uint32_t g = __hip_atomic_load(P + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (g == p) return p;
    atomicMin(P + i, g);  // path halving; monotone like every other write
    i = g;
    if (step > cap) {
      set_err(err);
      return i;
    }
  }
}

__device__ __forceinline__ void lds_unite(uint32_t* P, uint32_t a, uint32_t b, uint32_t cap, uint32_t* err) {
  // ends: a retry follows an atomicMin that met a slot already lowered, and goes on from that lower index,
  // so max(a, b) strictly decreases from retry to retry; capped all the same
  for (uint32_t step = 0;; ++step) {
    a = lds_find(P, a, cap, err), b = lds_find(P, b, cap, err);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b, b = t;
    }
    const uint32_t old = atomicMin(P + a, b);
    if (old == a) return;
    a = old;
    if (step > cap) {
      set_err(err);
      return;
    }
  }
}

__global__ __launch_bounds__(kNT) void k_ccl_tile(CclArgs a) {
  constexpr int T = kCclTile;
  __shared__ uint32_t P[T * T];
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % a.ntx, by = blockIdx.x / a.ntx;
  const int X0 = bx * T, Y0 = by * T;
  const int nx = min(T, a.W - X0), ny = min(T, a.H - Y0);
#pragma unroll
  for (int it = 0; it < T * T / kNT; ++it) {
    const int l = it * kNT + tid, ly = l / T, lx = l % T;
    bool fg = false;
    if (lx < nx && ly < ny) fg = a.src[(int64_t)(Y0 + ly) * a.sp + (X0 + lx)] != 0;
    P[l] = fg ? (uint32_t)l : kNone;
  }
  __syncthreads();
  for (int it = 0; it < T * T / kNT; ++it) {
    const int l = it * kNT + tid, ly = l / T, lx = l % T;
    if (P[l] == kNone) continue;  // (a foreground slot never becomes kNone)
    // outside the tile: not this kernel's link
    const bool w = lx > 0 && P[l - 1] != kNone;
    const bool n = ly > 0 && P[l - T] != kNone;
    const bool nw = lx > 0 && ly > 0 && P[l - T - 1] != kNone;
    const bool ne = ly > 0 && lx + 1 < T && P[l - T + 1] != kNone;
    const bool e = lx + 1 < T && P[l + 1] != kNone;
    if (w) lds_unite(P, l, l - 1, a.cap, a.err);
    if (n && !(w && nw)) lds_unite(P, l, l - T, a.cap, a.err);
    if (a.conn8) {
      if (nw && !w && !n) lds_unite(P, l, l - T - 1, a.cap, a.err);
      if (ne && !n && !e) lds_unite(P, l, l - T + 1, a.cap, a.err);
    }
  }
  __syncthreads();
  for (int it = 0; it < T * T / kNT; ++it) {
    const int l = it * kNT + tid, ly = l / T, lx = l % T;
    if (lx >= nx || ly >= ny) continue;
    int32_t v = 0;
    uint32_t r = P[l];
    if (r != kNone) {
      // read-only find: ends because parents strictly decrease; capped all the same
      r = l;
      for (uint32_t step = 0;; ++step) {
        const uint32_t p = P[r];
        if (p == r) break;
        r = p;
        if (step > a.cap) {
          set_err(a.err);
          break;
        }
      }
      // W * H <= 2^31 - 2: index + 1 fits int32
      v = (int32_t)((uint32_t)(Y0 + (int)(r / T)) * (uint32_t)a.W + (uint32_t)(X0 + (int)(r % T)) + 1u);
    }
    a.lab[(int64_t)(Y0 + ly) * a.lp + (X0 + lx)] = v;
  }
}

// ---- the global forest: the slot of raster index i holds its parent's index + 1 ----
__device__ __forceinline__ int32_t* slot(const CclArgs& a, uint32_t i) {
  if (a.lp == a.W) return a.lab + i;
  const uint32_t y = i / (uint32_t)a.W;
  return a.lab + (int64_t)y * a.lp + (i - y * (uint32_t)a.W);
}
__device__ __forceinline__ uint32_t parent(const CclArgs& a, uint32_t i) {
  return (uint32_t)__hip_atomic_load(slot(a, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1u;
}

__device__ __forceinline__ uint32_t g_find(const CclArgs& a, uint32_t i) {
  // ends: a parent's index is smaller than its child's and slots only decrease, so i strictly decreases;
  // capped all the same
  for (uint32_t step = 0;; ++step) {
    const uint32_t p = parent(a, i);
    if (p == i) return i;
    const uint32_t g = parent(a, p);
    if (g == p) return p;
    atomicMin(slot(a, i), (int32_t)(g + 1u));  // path halving; monotone like every other write
    i = g;
    if (step > a.cap) {
      set_err(a.err);
      return i;
    }
  }
}

__device__ __forceinline__ void g_unite(const CclArgs& a, uint32_t x, uint32_t y) {
  // ends: a retry follows an atomicMin that met a slot already lowered, and goes on from that lower index,
  // so max(x, y) strictly decreases from retry to retry; capped all the same.  A stale read only costs a retry:
  // the atomicMin returns the slot's true value.
  for (uint32_t step = 0;; ++step) {
    x = g_find(a, x), y = g_find(a, y);
    if (x == y) return;
    if (x < y) {
      const uint32_t t = x;
      x = y, y = t;
    }
    const uint32_t old = (uint32_t)atomicMin(slot(a, x), (int32_t)(y + 1u)) - 1u;
    if (old == x) return;
    x = old;
    if (step > a.cap) {
      set_err(a.err);
      return;
    }
  }
}

__device__ __forceinline__ bool is_fg(const CclArgs& a, int x, int y) {
  return x >= 0 && y >= 0 && x < a.W && y < a.H && a.lab[(int64_t)y * a.lp + x] != 0;
}

// The links of pixel (x, y) towards its W / NW / N / NE neighbours that cross a tile seam.
__global__ __launch_bounds__(kNT) void k_ccl_seam(CclArgs a, int64_t nrow_threads, int64_t total) {
  constexpr int T = kCclTile;
  const int64_t id = (int64_t)blockIdx.x * kNT + threadIdx.x;
  if (id >= total) return;
  int x, y;
  if (id < nrow_threads) {  // the first rows of the tile rows 1, 2, ..
    y = (int)(id / a.W + 1) * T, x = (int)(id % a.W);
  } else {  // the first columns of the tile columns 1, 2, .., and the column left of each for its NE links
    const int64_t k = id - nrow_threads;
    const int c = (int)(k / a.H);
    y = (int)(k % a.H);
    x = (c / 2 + 1) * T - (c & 1);
  }
  if (!is_fg(a, x, y)) return;
  const bool row0 = y % T == 0 && y > 0, col0 = x % T == 0 && x > 0, colL = x % T == T - 1 && x + 1 < a.W;
  const bool w = is_fg(a, x - 1, y), n = is_fg(a, x, y - 1), nw = is_fg(a, x - 1, y - 1);
  const bool ne = is_fg(a, x + 1, y - 1), e = is_fg(a, x + 1, y);
  const uint32_t i = (uint32_t)y * (uint32_t)a.W + (uint32_t)x;
  if (id < nrow_threads) {
    // N, NW and NE cross the seam above; W is the tile kernel's or a column thread's
    if (n && !(w && nw)) g_unite(a, i, i - a.W);
    if (a.conn8) {
      if (nw && !w && !n) g_unite(a, i, i - a.W - 1);
      if (ne && !n && !e) g_unite(a, i, i - a.W + 1);
    }
  } else if (col0) {
    // W crosses the seam on the left; NW too, where a row thread has not made it
    if (w) g_unite(a, i, i - 1);
    if (a.conn8 && !row0 && nw && !w && !n) g_unite(a, i, i - a.W - 1);
  } else if (colL) {
    // the last column's NE link crosses the seam on the right
    if (a.conn8 && !row0 && ne && !n && !e) g_unite(a, i, i - a.W + 1);
  }
}

// Every pixel takes its root; roots are counted per row.  A workgroup owns kNT pixels of one row.
__global__ __launch_bounds__(kNT) void k_ccl_flatten(CclArgs a) {
  const int bx = blockIdx.x % a.ntx, y = blockIdx.x / a.ntx;
  const int x = bx * kNT + threadIdx.x;
  bool root = false;
  if (x < a.W) {
    int32_t* q = a.lab + (int64_t)y * a.lp + x;
    const int32_t v = *q;
    if (v != 0) {
      const uint32_t self = (uint32_t)y * (uint32_t)a.W + (uint32_t)x;
      uint32_t r = (uint32_t)v - 1u;
      root = r == self;
      if (!root) {
        // read-only find (slots on the way are rewritten meanwhile, always to another ancestor; roots stay):
        // ends because parents strictly decrease; capped all the same
        for (uint32_t step = 0;; ++step) {
          const uint32_t p = parent(a, r);
          if (p == r) break;
          r = p;
          if (step > a.cap) {
            set_err(a.err);
            break;
          }
        }
        __hip_atomic_store(q, (int32_t)(r + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  const unsigned long long m = __ballot(root);
  if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(a.rows + y, (uint32_t)__popcll(m));
}

// Exclusive prefix of rows[0 .. H) in place; rows[H] = the total = N.  One workgroup.
__global__ __launch_bounds__(kNT) void k_ccl_scan(uint32_t* rows, int H, uint32_t* n_out) {
  __shared__ uint32_t part[kNT];
  const int tid = threadIdx.x;
  const int64_t chunk = ((int64_t)H + kNT - 1) / kNT;
  const int64_t y0 = min((int64_t)tid * chunk, (int64_t)H), y1 = min(y0 + chunk, (int64_t)H);
  uint32_t s = 0;
  for (int64_t y = y0; y < y1; ++y) s += rows[y];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    uint32_t acc = 0;
    for (int t = 0; t < kNT; ++t) {
      const uint32_t v = part[t];
      part[t] = acc;
      acc += v;
    }
    rows[H] = acc;
    *n_out = acc;
  }
  __syncthreads();
  uint32_t acc = part[tid];
  for (int64_t y = y0; y < y1; ++y) {
    const uint32_t v = rows[y];
    rows[y] = acc;
    acc += v;
  }
}

// One workgroup per row: the roots take minus their number.
__global__ __launch_bounds__(kNT) void k_ccl_number(CclArgs a) {
  __shared__ uint32_t wsum[kNT / 64];
  const int y = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t first = a.rows[y], want = a.rows[y + 1] - first;  // workgroup-uniform
  uint32_t done = 0;
  for (int x0 = 0; x0 < a.W && done < want; x0 += kNT) {
    const int x = x0 + tid;
    bool root = false;
    int32_t* q = a.lab + (int64_t)y * a.lp + x;
    if (x < a.W) root = (uint32_t)*q == (uint32_t)y * (uint32_t)a.W + (uint32_t)x + 1u;
    const unsigned long long m = __ballot(root);
    if (lane == 0) wsum[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kNT / 64; ++k) {
      const uint32_t c = wsum[k];
      before += k < wv ? c : 0u;
      all += c;
    }
    if (root) *q = -(int32_t)(first + done + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) + 1u);
    done += all;
    __syncthreads();
  }
}

// Every pixel takes the number of its root.
__global__ __launch_bounds__(kNT) void k_ccl_resolve(CclArgs a) {
  const int bx = blockIdx.x % a.ntx, y = blockIdx.x / a.ntx;
  const int x = bx * kNT + threadIdx.x;
  if (x >= a.W) return;
  int32_t* q = a.lab + (int64_t)y * a.lp + x;
  const int32_t v = *q;
  if (v == 0) return;
  // a root's slot holds -n until the root's own thread stores n
  const int32_t n = v < 0 ? v : __hip_atomic_load(slot(a, (uint32_t)v - 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(q, n < 0 ? -n : n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- statistics ----
struct StatArgs {
  const int32_t* lab;
  int64_t lp;
  int W, H, N;
  int nseg;  // segments per row
  unsigned long long* tab;  // (N + 1) x kStatCols
  uint32_t* err;
};

__global__ __launch_bounds__(kNT) void k_ccl_stats_init(unsigned long long* tab, int64_t n) {
  const int64_t l = (int64_t)blockIdx.x * kNT + threadIdx.x;
  if (l >= n) return;
  unsigned long long* e = tab + l * kStatCols;
  e[0] = 0, e[1] = ~0ull, e[2] = ~0ull, e[3] = 0, e[4] = 0, e[5] = 0, e[6] = 0;
}
__global__ __launch_bounds__(kNT) void k_ccl_stats_fix(unsigned long long* tab, int64_t n) {
  const int64_t l = (int64_t)blockIdx.x * kNT + threadIdx.x;
  if (l >= n) return;
  unsigned long long* e = tab + l * kStatCols;
  if (e[0] == 0) e[1] = 0, e[2] = 0;
}

// `area` pixels of label l in row y, columns within [x0, x1), their column sum sx
__device__ __forceinline__ void emit_pixels(const StatArgs& a, int32_t l, unsigned long long area, int x0, int x1, int y,
                                            unsigned long long sx) {
  if ((uint32_t)l > (uint32_t)a.N) {  // not this table's label: nothing is written
    set_err(a.err);
    return;
  }
  unsigned long long* e = a.tab + (int64_t)l * kStatCols;
  atomicAdd(e + 0, area);
  atomicMin(e + 1, (unsigned long long)x0);
  atomicMin(e + 2, (unsigned long long)y);
  atomicMax(e + 3, (unsigned long long)x1);
  atomicMax(e + 4, (unsigned long long)y + 1ull);
  atomicAdd(e + 5, sx);
  atomicAdd(e + 6, area * (unsigned long long)y);
}

// the sum of the indices of the set bits
__device__ __forceinline__ uint32_t sum_bit_index(unsigned long long m) {
  return (uint32_t)__popcll(m & 0xAAAAAAAAAAAAAAAAull) + ((uint32_t)__popcll(m & 0xCCCCCCCCCCCCCCCCull) << 1) +
         ((uint32_t)__popcll(m & 0xF0F0F0F0F0F0F0F0ull) << 2) + ((uint32_t)__popcll(m & 0xFF00FF00FF00FF00ull) << 3) +
         ((uint32_t)__popcll(m & 0xFFFF0000FFFF0000ull) << 4) + ((uint32_t)__popcll(m & 0xFFFFFFFF00000000ull) << 5);
}

// What a wave holds of one label over its segment (wave-uniform, from ballots alone).
struct Held {
  int32_t label;
  uint32_t area, sx;  // sx: the sum of (x - s0), at most kCclStatSeg^2 / 2
  int x0, x1;
  __device__ __forceinline__ void reset(int32_t l) { label = l, area = 0, sx = 0, x0 = INT_MAX, x1 = 0; }
  // m: the lanes of chunk c (columns c .. c + 63) that hold the label
  __device__ __forceinline__ void add(unsigned long long m, int c, int s0) {
    if (m == 0) return;
    const uint32_t n = (uint32_t)__popcll(m);
    area += n, sx += n * (uint32_t)(c - s0) + sum_bit_index(m);
    x0 = min(x0, c + (int)__builtin_ctzll(m)), x1 = max(x1, c + 64 - (int)__builtin_clzll(m));
  }
  __device__ __forceinline__ void flush(const StatArgs& a, int s0, int y) const {
    if (area != 0) emit_pixels(a, label, area, x0, x1, y, (unsigned long long)sx + (unsigned long long)area * (unsigned long long)s0);
  }
};

// A wave walks a segment of kCclStatSeg pixels of one row, 64 at a time.  Two labels are held in wave-uniform
// accumulators and cost a ballot and a few scalar popcounts a chunk: the background, and one foreground label, the
// one most frequent in the latest chunk that had a rival (flat frames and the giant component of a dense mask
// would otherwise send every run to the same seven words).  They are flushed when replaced and at the end of the
// segment.  Every other label is work per horizontal run: the heads of the runs of equal labels come from a ballot,
// and each head lane issues one set of atomics for its run (runs end at a chunk's end).
__global__ __launch_bounds__(kNT) void k_ccl_stats(StatArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (kNT / 64) + (threadIdx.x >> 6);
  const int y = (int)(wave / a.nseg);
  if (y >= a.H) return;
  const int s0 = (int)(wave % a.nseg) * kCclStatSeg, s1 = min(s0 + kCclStatSeg, a.W);
  const int32_t* row = a.lab + (int64_t)y * a.lp;
  constexpr int32_t kNoLabel = INT_MIN;  // (an invalid lane reads as -1: neither this nor a label)
  Held bg, hot;
  bg.reset(0), hot.reset(kNoLabel);
  for (int c = s0; c < s1; c += 64) {
    const int x = c + lane;
    const bool valid = x < s1;
    const int32_t l = valid ? row[x] : -1;
    unsigned long long m_hot = __ballot(l == hot.label);
    const unsigned long long m_other = __ballot(valid && l != 0 && l != hot.label);
    if (m_other != 0) {
      // the first rival of the held label: it takes over if this chunk has more of it
      const int32_t rival = __shfl(l, (int)__builtin_ctzll(m_other));
      const unsigned long long m_rival = __ballot(l == rival);
      if (__popcll(m_rival) > __popcll(m_hot)) {
        if (lane == 0) hot.flush(a, s0, y);
        hot.reset(rival);
        m_hot = m_rival;
      }
    }
    bg.add(__ballot(l == 0), c, s0);
    hot.add(m_hot, c, s0);
    // the runs of every other label
    const int32_t prev = __shfl_up(l, 1);
    const unsigned long long heads = __ballot(valid && (lane == 0 || l != prev));
    const int nvalid = min(64, s1 - c);
    if (valid && (lane == 0 || l != prev) && l != 0 && l != hot.label) {
      const unsigned long long next = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
      const int end = next ? (int)__builtin_ctzll(next) : nvalid;
      const unsigned long long len = (unsigned long long)(end - lane);
      emit_pixels(a, l, len, x, c + end, y, len * (unsigned long long)x + len * (len - 1ull) / 2ull);
    }
  }
  if (lane == 0) {
    bg.flush(a, s0, y);
    hot.flush(a, s0, y);
  }
}

// ---- area filter ----
struct SelectArgs {
  const uint8_t* src;
  const int32_t* lab;
  uint8_t* dst;
  const unsigned long long* tab;
  int64_t sp, lp, dp;
  int W, H, N, ntx;
  unsigned long long amin, amax;
};

__global__ __launch_bounds__(kNT) void k_ccl_select(SelectArgs a) {
  const int bx = blockIdx.x % a.ntx, y = blockIdx.x / a.ntx;
  const int x = bx * kNT + threadIdx.x;
  if (x >= a.W) return;
  const uint8_t s = a.src[(int64_t)y * a.sp + x];
  const int32_t l = a.lab[(int64_t)y * a.lp + x];
  bool keep = false;
  if (s != 0 && l > 0 && l <= a.N) {  // (a label outside the table keeps nothing and reads nothing)
    const unsigned long long area = a.tab[(int64_t)l * kStatCols];
    keep = area >= a.amin && area <= a.amax;
  }
  a.dst[(int64_t)y * a.dp + x] = keep ? s : (uint8_t)0;
}

}  // namespace dev

namespace {

// Per device and H: (H + 1) row prefixes, N, the error word.  The lock is held by a call from its first launch
// to its synchronisation, so that two streams never share the words.
struct CclTemp {
  std::array<int64_t, 2> key{};  // device, H
  uint32_t* d = nullptr;
};
constexpr size_t kMaxTemps = 16;
std::mutex g_ccl_mu;

uint32_t* ccl_temp(int H) {
  static std::list<CclTemp> cache;  // most recently used first; never destroyed before the runtime
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  const std::array<int64_t, 2> key{dev, H};
  for (auto it = cache.begin(); it != cache.end(); ++it)
    if (it->key == key) {
      cache.splice(cache.begin(), cache, it);
      return cache.front().d;
    }
  while (cache.size() >= kMaxTemps) {
    (void)hipFree(cache.back().d);
    cache.pop_back();
  }
  CclTemp t;
  t.key = key;
  HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t.d), ((size_t)H + 3) * sizeof(uint32_t)));
  cache.push_front(t);
  return t.d;
}

unsigned grid_of(int64_t n, const char* what) {
  STRIPE_CHECK(n >= 1 && n < (int64_t(1) << 31), "components: too many workgroups (" << what << ")");
  return (unsigned)n;
}

// The forest passes: the words cleared, k_ccl_tile, k_ccl_seam, k_ccl_flatten.  The caller holds g_ccl_mu and
// goes on with the argument block returned (ntx: the row segments of kNT pixels).
dev::CclArgs enqueue_forest(const ComponentsLaunch& L, uint32_t* tmp, hipStream_t s) {
  dev::CclArgs a{};
  a.src = L.src, a.lab = L.labels;
  a.sp = L.src_pitch, a.lp = L.labels_pitch;
  a.W = L.W, a.H = L.H;
  a.conn8 = L.conn == 8;
  a.cap = (uint32_t)((int64_t)L.W * L.H + 2);
  a.rows = tmp;
  a.err = tmp + L.H + 2;
  HIP_CHECK(hipMemsetAsync(tmp, 0, ((size_t)L.H + 3) * sizeof(uint32_t), s));
  const int64_t tx = div_up(L.W, kCclTile), ty = div_up(L.H, kCclTile);
  a.ntx = (int)tx;
  dev::k_ccl_tile<<<grid_of(tx * ty, "tiles"), dev::kNT, 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
  const int64_t nrow = (ty - 1) * L.W, ncol = 2 * (tx - 1) * L.H;
  if (nrow + ncol > 0) {
    dev::k_ccl_seam<<<grid_of(div_up(nrow + ncol, dev::kNT), "seams"), dev::kNT, 0, s>>>(a, nrow, nrow + ncol);
    HIP_CHECK(hipGetLastError());
  }
  const int64_t segs = div_up(L.W, dev::kNT);
  a.ntx = (int)segs;
  dev::k_ccl_flatten<<<grid_of(segs * L.H, "rows"), dev::kNT, 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
  return a;
}

}  // namespace

CclForest launch_ccl_forest(const ComponentsLaunch& L, hipStream_t s) {
  CclForest f;
  f.lock = std::unique_lock<std::mutex>(g_ccl_mu);
  const dev::CclArgs a = enqueue_forest(L, ccl_temp(L.H), s);
  f.err = a.err, f.cap = a.cap;
  return f;
}

int launch_components_kernels(const ComponentsLaunch& L, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_ccl_mu);
  uint32_t* tmp = ccl_temp(L.H);
  const dev::CclArgs a = enqueue_forest(L, tmp, s);
  uint32_t* n_word = tmp + L.H + 1;
  const int64_t segs = a.ntx;
  dev::k_ccl_scan<<<1, dev::kNT, 0, s>>>(tmp, L.H, n_word);
  HIP_CHECK(hipGetLastError());
  dev::k_ccl_number<<<grid_of(L.H, "rows"), dev::kNT, 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
  dev::k_ccl_resolve<<<grid_of(segs * L.H, "rows"), dev::kNT, 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
  uint32_t back[2] = {0, 0};  // N, the error word
  HIP_CHECK(hipMemcpyAsync(back, n_word, sizeof(back), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  STRIPE_CHECK(back[1] == 0, "components: a union-find loop overran its step cap of " << a.cap
                                 << " (a kernel bug; the labels are not valid)");
  return (int)back[0];
}

void launch_component_stats_kernels(const ComponentStatsLaunch& L, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_ccl_mu);
  uint32_t* tmp = ccl_temp(L.H);
  uint32_t* err = tmp + L.H + 2;
  HIP_CHECK(hipMemsetAsync(err, 0, sizeof(uint32_t), s));
  dev::StatArgs a{};
  a.lab = L.labels, a.lp = L.labels_pitch;
  a.W = L.W, a.H = L.H, a.N = L.N;
  a.nseg = (int)div_up(L.W, kCclStatSeg);
  a.tab = reinterpret_cast<unsigned long long*>(L.stats);
  a.err = err;
  const int64_t n = (int64_t)L.N + 1;
  dev::k_ccl_stats_init<<<grid_of(div_up(n, dev::kNT), "table"), dev::kNT, 0, s>>>(a.tab, n);
  HIP_CHECK(hipGetLastError());
  const int64_t waves = (int64_t)a.nseg * L.H;
  dev::k_ccl_stats<<<grid_of(div_up(waves, dev::kNT / 64), "runs"), dev::kNT, 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
  dev::k_ccl_stats_fix<<<grid_of(div_up(n, dev::kNT), "table"), dev::kNT, 0, s>>>(a.tab, n);
  HIP_CHECK(hipGetLastError());
  uint32_t back = 0;
  HIP_CHECK(hipMemcpyAsync(&back, err, sizeof(back), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  STRIPE_CHECK(back == 0, "components: a label outside 0.." << L.N);
}

void launch_area_filter_kernel(const AreaFilterLaunch& L, hipStream_t s) {
  dev::SelectArgs a{};
  a.src = L.src, a.lab = L.labels, a.dst = L.dst;
  a.tab = reinterpret_cast<const unsigned long long*>(L.stats);
  a.sp = L.src_pitch, a.lp = L.labels_pitch, a.dp = L.dst_pitch;
  a.W = L.W, a.H = L.H, a.N = L.N;
  a.ntx = (int)div_up(L.W, dev::kNT);
  a.amin = (unsigned long long)L.amin, a.amax = (unsigned long long)L.amax;
  dev::k_ccl_select<<<grid_of((int64_t)a.ntx * L.H, "rows"), dev::kNT, 0, s>>>(a);
  HIP_CHECK(hipGetLastError());
}

int components_device(const uint8_t* src, int64_t src_pitch, int W, int H, int conn, int32_t* labels,
                      int64_t labels_pitch, hipStream_t s) {
  ComponentsLaunch L;
  L.src = src, L.src_pitch = src_pitch;
  L.W = W, L.H = H, L.conn = conn;
  L.labels = labels, L.labels_pitch = labels_pitch;
  return launch_components(L, s);
}

void component_stats_device(const int32_t* labels, int64_t labels_pitch, int W, int H, int N, int64_t* stats,
                            hipStream_t s) {
  ComponentStatsLaunch L;
  L.labels = labels, L.labels_pitch = labels_pitch;
  L.W = W, L.H = H, L.N = N;
  L.stats = stats;
  launch_component_stats(L, s);
}

void area_filter_device(const uint8_t* src, int64_t src_pitch, int W, int H, const int32_t* labels,
                        int64_t labels_pitch, const int64_t* stats, int N, int64_t amin, int64_t amax, uint8_t* dst,
                        int64_t dst_pitch, hipStream_t s) {
  AreaFilterLaunch L;
  L.src = src, L.src_pitch = src_pitch;
  L.W = W, L.H = H;
  L.labels = labels, L.labels_pitch = labels_pitch;
  L.stats = stats, L.N = N;
  L.amin = amin, L.amax = amax;
  L.dst = dst, L.dst_pitch = dst_pitch;
  launch_area_filter(L, s);
}

}  // namespace stripe
