// Pass dispatch: one entry point for every compiled pass kind.
// Every launch is shape-checked before it runs and error-checked after (the
// reference launches three kernels with no checks, kernel.cu:192-195).
#include "stripe/kernels.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>

#include "launch_policy.h"
#include "stripe/common.h"

namespace stripe {

size_t nt_lds_reserve(const void* fn, int target) {
  if (target <= 0) return 0;
  static std::mutex mu;
  static std::map<std::tuple<const void*, int, int>, size_t> cache;
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({fn, dev, target});
  if (it != cache.end()) return it->second;
  int lds_cu = 0;
  HIP_CHECK(hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev));
  hipFuncAttributes fa{};
  HIP_CHECK(hipFuncGetAttributes(&fa, fn));
  const size_t dyn = (size_t)policy::lds_reserve_bytes(lds_cu, (int64_t)fa.sharedSizeBytes, target);
  cache[{fn, dev, target}] = dyn;
  return dyn;
}

namespace {

using policy::desc_limit;

int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// A stencil / conv pass over buffers larger than one descriptor view (an image
// that fits HBM but not 2 GiB: 32768^2 RGB is 3 GiB): split the output rows
// into chunks and re-base both views on each chunk.  Rows a chunk's kernels
// read past its own span (the 32-row groups of the MFMA blur, the 16*MT-row
// tiles of the MFMA conv round up) only feed outputs that are not stored; the
// Constant border's zero row becomes an out-of-range offset, which buffer loads
// return as zeros.
void launch_chunked(const Pass& p, const PassConsts& pc, const PassLaunch& L, hipStream_t s) {
  const int64_t lim = desc_limit();
  const int Rs = p.R + 64;
  const int64_t maxp = std::max(L.in_pitch, L.out_pitch);
  const int64_t cr = lim / maxp - 2 * Rs - 2;
  STRIPE_CHECK(cr >= 16, "rows too wide for " << lim << "-byte descriptor views (pitch " << maxp << ")");
  // local rows whose whole padded row lies inside each allocation
  const int64_t in_lo = floor_div(kMarginBytes - L.in_org + L.in_pitch - 1, L.in_pitch);
  const int64_t in_hi = floor_div(L.in_bytes - L.in_org + kMarginBytes, L.in_pitch);
  for (int r = 0; r < L.nrange; ++r) {
    for (int64_t c0 = L.ry[2 * r]; c0 < L.ry[2 * r + 1]; c0 += cr) {
      const int64_t c1 = std::min<int64_t>(c0 + cr, L.ry[2 * r + 1]);
      PassLaunch C = L;
      C.rebased = true;
      C.nrange = 1;
      C.ry[0] = (int)c0;
      C.ry[1] = (int)c1;
      const int64_t lo = std::max(c0 - Rs, in_lo), hi = std::min(c1 + Rs, in_hi);
      const int64_t ib = L.in_org + lo * L.in_pitch - kMarginBytes;
      C.in_base = L.in_base + ib;
      C.in_bytes = std::min((hi - lo) * L.in_pitch, L.in_bytes - ib);
      C.in_org = L.in_org - ib;
      C.in_zero = (int64_t)1 << 31;  // out of range: loads read zeros
      const int64_t ob = L.out_org + c0 * L.out_pitch - kMarginBytes;
      STRIPE_CHECK(ib >= 0 && ob >= 0 && ob + (c1 - c0) * L.out_pitch <= L.out_bytes + kMarginBytes,
                   "chunk outside its buffers");
      C.out_base = L.out_base + ob;
      C.out_bytes = std::min((c1 - c0) * L.out_pitch, L.out_bytes - ob);
      C.out_org = L.out_org - ob;
      if (p.kind == PassKind::Conv) launch_conv(p, pc, C, s);
      else launch_stencil(p, pc, C, s);
    }
  }
}

}  // namespace

void launch_histogram(const HistLaunch& L, hipStream_t s) {
  // host-side shape checks before the kernel touches memory
  STRIPE_CHECK(L.in && L.bins && L.W >= 1 && L.rows >= 0, "bad histogram launch");
  STRIPE_CHECK(L.C == 1 || L.C == 3, "histogram needs 1 or 3 channels, got " << L.C);
  STRIPE_CHECK((int64_t)L.W * L.C < (int64_t(1) << 31) - 16, "histogram: row of " << L.W << " pixels too wide");
  STRIPE_CHECK(L.pitch >= align_up((int64_t)L.W * L.C, 16), "pitch too small for the histogram's rows");
  // per-stripe bins are u32: a stripe holds fewer than 2^32 pixels
  STRIPE_CHECK((int64_t)L.W * L.rows < (int64_t(1) << 32),
               "histogram: a stripe of " << L.W << "x" << L.rows << " pixels overflows the u32 bins");
  // the rows read (whole 16-byte groups) lie inside the allocation
  STRIPE_CHECK(L.in_base && L.in >= L.in_base &&
                   (L.rows == 0 || (L.in - L.in_base) + (int64_t)(L.rows - 1) * L.pitch +
                                           align_up((int64_t)L.W * L.C, 16) <= L.in_bytes),
               "histogram rows outside their buffer");
  STRIPE_CHECK(((uintptr_t)L.in % 16 == 0) && L.pitch % 16 == 0, "histogram rows must be 16-byte aligned");
  (void)hipGetLastError();  // sticky errors of other libraries (see launch_pass)
  launch_hist_kernel(L, s);
}

namespace {

// One pitched view of a whole-frame launch: h rows of w pixels of px bytes, `pitch` bytes apart; base / bytes
// name the allocation it lies in where the caller knows it.  `name` and `rows` word the messages.
struct View {
  const char *name, *rows;
  const void* p;
  int64_t pitch;
  int w, h, px;
  const uint8_t* base;
  int64_t bytes;
};

void check_pitch(const char* op, const View& v) {
  STRIPE_CHECK(v.pitch >= (int64_t)v.w * v.px,
               op << ": " << v.name << "_pitch " << v.pitch << " < row bytes " << (int64_t)v.w * v.px);
}

// the kernels address with 64-bit pointers: no size limit beyond the axes'.  Where the caller names the
// allocation, the rows touched lie inside it.
void check_inside(const char* op, const View& v) {
  const uint8_t* p = static_cast<const uint8_t*>(v.p);
  if (v.base)
    STRIPE_CHECK(p >= v.base && (p - v.base) + (int64_t)(v.h - 1) * v.pitch + (int64_t)v.w * v.px <= v.bytes,
                 op << ": " << v.rows << " rows outside their buffer");
}

// The checks every geometry stage makes on its two views before the kernel touches memory.
void check_frame(const char* op, int C, int max_size, const View& src, const View& dst) {
  STRIPE_CHECK(src.p && dst.p, "bad " << op << " launch: null src or dst");
  STRIPE_CHECK(C == 1 || C == 3, op << " needs 1 or 3 channels, got C = " << C);
  for (const View* v : {&src, &dst})
    STRIPE_CHECK(v->w >= 1 && v->w <= max_size && v->h >= 1 && v->h <= max_size,
                 op << ": " << v->rows << " size " << v->w << "x" << v->h << " outside 1.." << max_size);
  check_pitch(op, src);
  check_pitch(op, dst);
  check_inside(op, src);
  check_inside(op, dst);
  (void)hipGetLastError();  // sticky errors of other libraries (see launch_pass)
}

// the two views of a *Launch with the geometry stages' field names
template <class L>
void check_frame(const char* op, int max_size, const L& l, int W, int H, int W2, int H2) {
  check_frame(op, l.C, max_size, {"src", "source", l.src, l.src_pitch, W, H, l.C, l.src_base, l.src_bytes},
              {"dst", "destination", l.dst, l.dst_pitch, W2, H2, l.C, l.dst_base, l.dst_bytes});
}

}  // namespace

void launch_resize(const ResizeLaunch& L, hipStream_t s) {
  check_frame("resize", kResizeMaxSize, L, L.W, L.H, L.W2, L.H2);
  STRIPE_CHECK(L.fx && L.ox && L.wx && L.fy && L.oy && L.wy, "resize: missing tap tables");
  // the tile plan fits the instance it names (the kernel's LDS arrays)
  STRIPE_CHECK(L.cls >= 0 && L.cls < 4 && L.tile >= 4 && L.tile <= kResizeTile && L.tile % 4 == 0,
               "resize: bad tile plan (tile " << L.tile << ", class " << L.cls << ")");
  const ResizeClass& rc = kResizeClasses[L.cls];
  STRIPE_CHECK(L.max_span >= 1 && L.max_span + 15 <= rc.src_bytes && L.max_span <= L.W * L.C,
               "resize: a tile's source span of " << L.max_span << " bytes does not fit class " << L.cls);
  STRIPE_CHECK(rc.w_entries == 0 ? L.max_count_x <= 2 : L.max_weights <= rc.w_entries,
               "resize: a tile's x-weights do not fit class " << L.cls);
  launch_resize_kernel(L, s);
}

void launch_orient(const OrientLaunch& L, hipStream_t s) {
  STRIPE_CHECK((int)L.op >= 0 && (int)L.op < 8, "orient: bad orientation " << (int)L.op);
  check_frame("orient", kOrientMaxSize, L, L.w, L.h, orient_t(L.op) ? L.h : L.w, orient_t(L.op) ? L.w : L.h);
  launch_orient_kernel(L, s);
}

void launch_warp(const WarpLaunch& L, hipStream_t s) {
  const WarpMap& m = L.map;
  check_frame("warp", kWarpMaxSize, L, L.W, L.H, m.W2, m.H2);
  // the quantiser's ranges: every term of the map stays below 2^48
  for (int i = 0; i < 2; ++i) {
    STRIPE_CHECK(m.A[i][0] > -(int64_t(64) << kWarpQ) && m.A[i][0] < (int64_t(64) << kWarpQ) &&
                     m.A[i][1] > -(int64_t(64) << kWarpQ) && m.A[i][1] < (int64_t(64) << kWarpQ),
                 "warp: map coefficient outside (-64, 64)");
    STRIPE_CHECK(m.B[i] > -(int64_t(1) << (20 + kWarpQ)) && m.B[i] < (int64_t(1) << (20 + kWarpQ)),
                 "warp: map offset outside (-2^20, 2^20)");
  }
  STRIPE_CHECK((int)m.mode >= 0 && (int)m.mode < 2 && (int)m.border >= 0 && (int)m.border < 2,
               "warp: bad mode or border");
  launch_warp_kernel(L, s);
}

void launch_remap(const RemapLaunch& L, hipStream_t s) {
  // (the nodes themselves stay on the device: the kernel clamps or tests every index that follows from them)
  const RemapMesh& m = L.mesh;
  check_mesh(m, L.mesh_count, false, "launch");  // (and with it the destination's size)
  check_frame("remap", kWarpMaxSize, L, L.W, L.H, m.W2, m.H2);
  STRIPE_CHECK((reinterpret_cast<uintptr_t>(m.nodes) & 3) == 0, "remap: the mesh must be aligned to 4 bytes");
  launch_remap_kernel(L, s);
}

int launch_components(const ComponentsLaunch& L, hipStream_t s) {
  // host-side shape checks before any kernel touches memory
  const View src{"src", "source", L.src, L.src_pitch, L.W, L.H, 1, L.src_base, L.src_bytes};
  const View labels{"labels", "label", L.labels, L.labels_pitch * 4, L.W, L.H, 4, L.labels_base, L.labels_bytes};
  STRIPE_CHECK(L.src && L.labels, "bad components launch: null src or labels");
  check_components(L.W, L.H, 1, L.conn);
  check_pitch("components", src);
  STRIPE_CHECK(L.labels_pitch >= (int64_t)L.W,
               "components: labels_pitch " << L.labels_pitch << " < the row's " << L.W << " elements");
  STRIPE_CHECK((reinterpret_cast<uintptr_t>(L.labels) & 3) == 0, "components: the labels must be aligned to 4 bytes");
  check_inside("components", src);
  check_inside("components", labels);
  (void)hipGetLastError();  // sticky errors of other libraries (see launch_pass)
  return launch_components_kernels(L, s);
}

void launch_component_stats(const ComponentStatsLaunch& L, hipStream_t s) {
  STRIPE_CHECK(L.labels && L.stats, "bad component stats launch: null labels or stats");
  check_components(L.W, L.H, 1, 8);
  STRIPE_CHECK(L.N >= 0 && (int64_t)L.N <= (int64_t)L.W * L.H, "components: N = " << L.N << " outside 0..W * H");
  STRIPE_CHECK(L.labels_pitch >= (int64_t)L.W,
               "components: labels_pitch " << L.labels_pitch << " < the row's " << L.W << " elements");
  STRIPE_CHECK((reinterpret_cast<uintptr_t>(L.labels) & 3) == 0 && (reinterpret_cast<uintptr_t>(L.stats) & 7) == 0,
               "components: the labels must be aligned to 4 bytes, the table to 8");
  (void)hipGetLastError();
  launch_component_stats_kernels(L, s);
}

void launch_area_filter(const AreaFilterLaunch& L, hipStream_t s) {
  STRIPE_CHECK(L.src && L.labels && L.stats && L.dst, "bad area filter launch: null src, labels, stats or dst");
  check_components(L.W, L.H, 1, 8);
  check_area_bounds(L.amin, L.amax);
  STRIPE_CHECK(L.N >= 0 && (int64_t)L.N <= (int64_t)L.W * L.H, "components: N = " << L.N << " outside 0..W * H");
  STRIPE_CHECK(L.src_pitch >= (int64_t)L.W && L.dst_pitch >= (int64_t)L.W && L.labels_pitch >= (int64_t)L.W,
               "components: pitch smaller than a row");
  STRIPE_CHECK((reinterpret_cast<uintptr_t>(L.labels) & 3) == 0 && (reinterpret_cast<uintptr_t>(L.stats) & 7) == 0,
               "components: the labels must be aligned to 4 bytes, the table to 8");
  (void)hipGetLastError();
  launch_area_filter_kernel(L, s);
}

namespace {
void check_distance_launch(const DistanceLaunch& L) {
  // host-side shape checks before any kernel touches memory
  STRIPE_CHECK(L.src && L.dst, "bad distance launch: null src or dst");
  check_distance(L.W, L.H, 1);
  check_distance_mode(L.mode, L.t);
  STRIPE_CHECK(L.src_pitch >= (int64_t)L.W, "distance: src_pitch " << L.src_pitch << " < row bytes " << L.W);
  STRIPE_CHECK(L.dst_pitch >= (int64_t)L.W,
               "distance: dst_pitch " << L.dst_pitch << " < the row's " << L.W << " elements");
  STRIPE_CHECK(L.mode != (int)DistanceMode::Squared || (reinterpret_cast<uintptr_t>(L.dst) & 3) == 0,
               "distance: the int32 plane must be aligned to 4 bytes");
}
}  // namespace

void launch_distance(const DistanceLaunch& L, hipStream_t s) {
  check_distance_launch(L);
  (void)hipGetLastError();  // sticky errors of other libraries (see launch_pass)
  launch_distance_kernels(L, s);
}

void launch_disk_morph(const DistanceLaunch& L, int op, hipStream_t s) {
  STRIPE_CHECK(op >= 0 && op <= (int)DiskOp::Close, "distance: unknown disc operation " << op);
  check_distance_launch(L);
  STRIPE_CHECK(L.mode != (int)DistanceMode::Squared, "distance: a disc operation stores a u8 mask");
  (void)hipGetLastError();
  launch_disk_morph_kernels(L, op, s);
}

void launch_integral(const IntegralLaunch& L, hipStream_t s) {
  // host-side shape checks before any kernel touches memory
  STRIPE_CHECK(L.src && L.dst, "bad integral launch: null src or dst");
  check_integral(L.W, L.H, 1);
  STRIPE_CHECK(L.src_pitch >= (int64_t)L.W, "integral: src_pitch " << L.src_pitch << " < row bytes " << L.W);
  STRIPE_CHECK(L.dst_pitch >= (int64_t)L.W + 1,
               "integral: dst_pitch " << L.dst_pitch << " < the row's " << L.W + 1 << " elements");
  STRIPE_CHECK((reinterpret_cast<uintptr_t>(L.dst) & 3) == 0, "integral: the int32 plane must be aligned to 4 bytes");
  (void)hipGetLastError();  // sticky errors of other libraries (see launch_pass)
  launch_integral_kernels(L, s);
}

void launch_window(const WindowLaunch& L, hipStream_t s) {
  STRIPE_CHECK(L.src && L.dst, "bad window launch: null src or dst");
  check_integral(L.W, L.H, 1);
  STRIPE_CHECK(L.border >= 0 && L.border <= (int)Border::Skip, "integral: unknown border " << L.border);
  check_window(L.op, L.K, (Border)L.border, L.C, L.kq);
  STRIPE_CHECK(L.src_pitch >= (int64_t)L.W, "integral: src_pitch " << L.src_pitch << " < row bytes " << L.W);
  STRIPE_CHECK(L.dst_pitch >= (int64_t)L.W, "integral: dst_pitch " << L.dst_pitch << " < row bytes " << L.W);
  (void)hipGetLastError();
  launch_window_kernels(L, s);
}

void launch_canny(const CannyLaunch& L, hipStream_t s) {
  // host-side shape checks before any kernel touches memory
  STRIPE_CHECK(L.src && L.dst, "bad canny launch: null src or dst");
  STRIPE_CHECK(L.stage >= 0 && L.stage <= (int)CannyStage::Hysteresis, "canny: unknown stage " << L.stage);
  if (L.stage == (int)CannyStage::Hysteresis) {
    check_hysteresis(L.W, L.H, 1, L.low, L.high, L.conn);
  } else {
    STRIPE_CHECK(L.border >= 0 && L.border <= (int)Border::Skip, "canny: unknown border " << L.border);
    check_canny(L.W, L.H, 1, L.low, L.high, L.norm, (Border)L.border);
  }
  STRIPE_CHECK(L.src_pitch >= (int64_t)L.W, "canny: src_pitch " << L.src_pitch << " < row bytes " << L.W);
  STRIPE_CHECK(L.dst_pitch >= (int64_t)L.W, "canny: dst_pitch " << L.dst_pitch << " < row bytes " << L.W);
  (void)hipGetLastError();  // sticky errors of other libraries (see launch_pass)
  launch_canny_kernels(L, s);
}

void launch_pass(const Pass& p, const PassConsts& pc, const PassLaunch& L, hipStream_t s) {
  // host-side shape checks before any kernel touches memory
  STRIPE_CHECK(L.in && L.out && L.W >= 1 && L.rows >= 0, "bad pass launch");
  STRIPE_CHECK(L.nrange == 1 || L.nrange == 2, "nrange must be 1 or 2");
  STRIPE_CHECK(L.ext >= 0 && (L.ext == 0 || p.kind == PassKind::Separable || p.kind == PassKind::Direct ||
                               p.kind == PassKind::Pointwise),
               "halo-row outputs (ext) are for stencil and pointwise passes only");
  for (int r = 0; r < L.nrange; ++r)
    STRIPE_CHECK(-L.ext <= L.ry[2 * r] && L.ry[2 * r] <= L.ry[2 * r + 1] && L.ry[2 * r + 1] <= L.rows + L.ext,
                 "row range [" << L.ry[2 * r] << "," << L.ry[2 * r + 1] << ") outside stripe of " << L.rows
                               << " (+" << L.ext << " halo rows)");
  STRIPE_CHECK(L.in_pitch >= padded_pitch(L.W, p.cin) && L.out_pitch >= padded_pitch(L.W, p.cout),
               "pitch too small for the pass");
  STRIPE_CHECK(p.R <= kMaxRadius && p.out_margin_px <= margin_pixels(p.cout), "radius/margin too large");
  STRIPE_CHECK(L.Hg >= 1 && L.row0 >= 0 && L.row0 + L.rows <= L.Hg, "bad border geometry");
  STRIPE_CHECK(p.border != Border::Constant || L.zero_row != nullptr, "constant border needs a zero row");
  // hipGetLastError is sticky per thread and libraries (RCCL) may leave benign
  // errors behind: clear it so the post-launch check reports only our launch
  (void)hipGetLastError();
  if (p.kind == PassKind::Combine) {
    // plain 64-bit row pointers (no descriptor views): the rows the kernel
    // touches, whole 16-byte groups of [0, W * C), lie inside all three allocations
    STRIPE_CHECK(L.in2 != nullptr && p.cin == p.cout && L.ext == 0, "bad combine launch");
    const int64_t span = align_up((int64_t)L.W * p.cin, 16);
    auto inside = [&](const uint8_t* org, const uint8_t* base, int64_t bytes, int64_t pitch) {
      if (!base || org < base) return false;
      for (int r = 0; r < L.nrange; ++r) {
        const int y0 = L.ry[2 * r], y1 = L.ry[2 * r + 1];
        if (y1 > y0 && (org - base) + (int64_t)(y1 - 1) * pitch + span > bytes) return false;
      }
      return true;
    };
    STRIPE_CHECK(inside(L.in, L.in_base, L.in_bytes, L.in_pitch) && inside(L.in2, L.in2_base, L.in2_bytes, L.in_pitch) &&
                     inside(L.out, L.out_base, L.out_bytes, L.out_pitch),
                 "combine rows outside their buffers");
    STRIPE_CHECK(((uintptr_t)L.in | (uintptr_t)L.in2 | (uintptr_t)L.out) % 16 == 0 && L.in_pitch % 16 == 0 &&
                     L.out_pitch % 16 == 0,
                 "combine rows must be 16-byte aligned");
    launch_combine(p, pc, L, s);
    return;
  }
  if (p.kind != PassKind::Pointwise && (L.in_bytes > desc_limit() || L.out_bytes > desc_limit())) {
    launch_chunked(p, pc, L, s);
    return;
  }
  switch (p.kind) {
    case PassKind::Pointwise: launch_pointwise(p, pc, L, s); break;
    case PassKind::Separable:
    case PassKind::Direct: launch_stencil(p, pc, L, s); break;
    case PassKind::Conv: launch_conv(p, pc, L, s); break;
    case PassKind::Combine: break;  // (launched above)
  }
}

}  // namespace stripe
