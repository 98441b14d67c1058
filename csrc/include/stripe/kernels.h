// Host-side launch API of the HIP kernels (csrc/hip/*.hip).
//
// All launches are asynchronous on the given stream and error-checked
// (hipGetLastError after every launch; the reference never checks its three
// launches, kernel.cu:192-195, Q10).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "stripe/canny.h"
#include "stripe/chain.h"
#include "stripe/components.h"
#include "stripe/distance.h"
#include "stripe/image.h"
#include "stripe/integral.h"
#include "stripe/orient.h"
#include "stripe/remap.h"
#include "stripe/resize.h"
#include "stripe/warp.h"

namespace stripe {

#define HIP_CHECK(expr)                                                              \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      std::ostringstream _os;                                                        \
      _os << __FILE__ << ":" << __LINE__ << ": " #expr " failed: " << hipGetErrorString(_e); \
      ::stripe::fail(_os.str());                                                     \
    }                                                                                \
  } while (0)

// Device-resident per-pass constants, built once by the engine.
// Per-pass LUT block: [pre 256 | post 256 | epi 256] (the gray:ref terms are
// computed by multiply-shift in the kernels).
// A bilateral pass appends its range table: [pre | post | epi | range], 1024
// bytes.  Run-time tables (statistic ops) re-upload the first kLutBytes only.
constexpr int kLutBytes = 768;
constexpr int kRangeBytes = 256;

struct PassConsts {
  uint8_t* luts = nullptr;   // kLutBytes, layout above
  size_t luts_bytes = kLutBytes;  // kLutBytes + kRangeBytes for a bilateral pass
  void* conv = nullptr;      // conv pass: packed MFMA operand tables
  size_t conv_bytes = 0;
  int conv_mode = 0;         // general conv: 0 f16 hi+lo row pairs, 1 i8 weight digits (k_conv_i8)
  double conv_scale = 0;     // i8 digits: weights = W_int * conv_scale (a power of two)
  double conv_bias = 0;      // i8 digits: 128 * sum(w), the exact f32 weights (the x - 128 shift)
  double sep_hinit = 0;      // separable blur, subnormal staging: horizontal accumulator start (lsb centring)
};

struct PassLaunch {
  const uint8_t* in = nullptr;   // origin (local row 0, byte 0) of the input stripe
  int64_t in_pitch = 0;
  uint8_t* out = nullptr;        // origin of the output stripe
  int64_t out_pitch = 0;
  // combine passes: origin of the held image's stripe (pitch in_pitch) and the
  // allocation it lies in (checked by launch_pass)
  const uint8_t* in2 = nullptr;
  const uint8_t* in2_base = nullptr;
  int64_t in2_bytes = 0;
  int W = 0;                     // pixels per row
  int rows = 0;                  // local rows owned
  int row0 = 0, Hg = 0;          // border geometry (global row of local 0, global H)
  int nrange = 1;                // 1 or 2 output row ranges
  int ry[4] = {0, 0, 0, 0};      // [ry0, ry1) and [ry2, ry3)
  int ext = 0;                   // halo rows above/below the stripe that an output range may
                                 // cover (deep-halo schedule; stencil passes only)
  const uint8_t* zero_row = nullptr;  // origin of an all-zero row (Constant y-border)
  int band = 0;                  // rows per workgroup (0 = auto)
  int wgs = -1;                  // stencil occupancy cap, resident workgroups per CU
                                 // (-1: the kernel family's default, 0: no cap)
  int nt = -1;                   // stencil memory policy: 1 HBM-streaming (nt stores, linear
                                 // workgroup order), 0 cache-resident (default stores, XCD-aware
                                 // order), -1 chosen by the launch's size against the
                                 // Infinity Cache
  int order = 0;                 // separable stencil task order: 0 one band of one tile
                                 // column per wave, band-major; 1 XCD-local runs of bands
                                 // in alternating directions (kRuns, plain separable
                                 // filters: halo rows read twice within one L2)
  // Allocation view for buffer-descriptor kernels (branch-free OOB masking):
  // origin = base + org, zero row origin = in_base + in_zero; sizes < 2 GiB.
  const uint8_t* in_base = nullptr;
  int64_t in_bytes = 0, in_org = 0, in_zero = 0;
  uint8_t* out_base = nullptr;
  int64_t out_bytes = 0, out_org = 0;
  // Set by launch_pass when it splits a launch whose buffers exceed the
  // descriptor range: the views are re-based on each row chunk, so origin
  // offsets may precede the base (they wrap in the kernels' 32-bit offsets).
  bool rebased = false;
};

// Occupancy cap as an LDS reservation: the dynamic shared memory (bytes) that
// lets only `target` workgroups of kernel `fn` fit a CU's LDS on the current
// device (policy::lds_reserve_bytes of the kernel's static LDS; 0 for
// target <= 0).  Cached per kernel, device and target (dispatch.cpp).
size_t nt_lds_reserve(const void* fn, int target);

void launch_pass(const Pass& p, const PassConsts& pc, const PassLaunch& L, hipStream_t s);
void launch_pointwise(const Pass& p, const PassConsts& pc, const PassLaunch& L, hipStream_t s);
void launch_stencil(const Pass& p, const PassConsts& pc, const PassLaunch& L, hipStream_t s);
void launch_conv(const Pass& p, const PassConsts& pc, const PassLaunch& L, hipStream_t s);
// Two-input pointwise pass (csrc/hip/combine.hip k_combine): out = post(op(in, in2)).
void launch_combine(const Pass& p, const PassConsts& pc, const PassLaunch& L, hipStream_t s);

// Histogram of rows [0, rows) of a stripe (csrc/hip/histogram.hip k_hist): a
// read-only pass that ADDS the counts of exactly the rows' W * C bytes (no
// margin, halo row or pitch padding) to `bins`, 256 x C u32 on the device,
// [c * 256 + v].  The caller zeroes `bins` on the same stream first.  A stripe
// holds fewer than 2^32 pixels (checked), so a u32 bin cannot wrap.
struct HistLaunch {
  const uint8_t* in = nullptr;  // origin (local row 0, byte 0) of the stripe
  int64_t pitch = 0;
  int W = 0, C = 0, rows = 0;
  const uint8_t* in_base = nullptr;  // the allocation `in` lies in (checked against the rows read)
  int64_t in_bytes = 0;
  uint32_t* bins = nullptr;
};
constexpr int kHistBins = 256 * 3;  // bins of the device table (RGB; gray uses the first 256)
void launch_histogram(const HistLaunch& L, hipStream_t s);    // dispatch.cpp: checks, then the kernel
void launch_hist_kernel(const HistLaunch& L, hipStream_t s);  // histogram.hip

// Resize of a whole frame (csrc/hip/resize.hip k_resize; the rule: stripe/resize.h).
// Plain 64-bit addressing on arbitrary pitched buffers: no alignment of base
// pointers or pitches is assumed, no byte outside [src, src + (H-1) pitch + W C)
// is read and no byte outside the W2 * C bytes of each destination row is written.
//
// A workgroup owns `tile` output bytes (4 per thread) of kResizeBand output rows.
// It stages the source bytes its tile reads, row by row, in LDS; the instance
// (`cls`) fixes how many source bytes and x-weights fit:
//   cls 0, 1: at most 2 taps per output pixel in x, weights in registers
//   cls 2, 3: any tap count, the tile's x-weights in LDS
constexpr int kResizeTile = 1024;  // largest tile, output bytes
constexpr int kResizeBand = 8;     // output rows per workgroup
struct ResizeClass {
  int src_bytes;  // LDS bytes of one source row's span (15 of them are alignment slack)
  int w_entries;  // LDS u16 entries of the tile's x-weights (0: registers)
};
constexpr ResizeClass kResizeClasses[4] = {{4608, 0}, {36864, 0}, {9216, 6144}, {36864, 12288}};
struct ResizeLaunch {
  const uint8_t* src = nullptr;
  int64_t src_pitch = 0;
  int W = 0, H = 0, C = 0;
  uint8_t* dst = nullptr;
  int64_t dst_pitch = 0;
  int W2 = 0, H2 = 0;
  // tap tables on the device (ResizeTaps::first / offset / w of each axis)
  const int32_t *fx = nullptr, *ox = nullptr, *fy = nullptr, *oy = nullptr;
  const uint16_t *wx = nullptr, *wy = nullptr;
  // the tile plan of the x tables (resize_tile_plan) and what it measured on them
  int tile = 0, cls = 0;
  int max_count_x = 0;  // most taps of an output pixel in x
  int max_span = 0;     // most source bytes a tile reads of one row
  int max_weights = 0;  // most x-weights of a tile
  // optional: the allocations the views lie in (checked against the rows touched)
  const uint8_t* src_base = nullptr;
  int64_t src_bytes = 0;
  const uint8_t* dst_base = nullptr;
  int64_t dst_bytes = 0;
};
// Largest tile (a multiple of 4 bytes, at most kResizeTile) and smallest class
// that hold every tile's source span and weights; fills tile, cls, max_*.
void resize_tile_plan(const ResizeTaps& tx, int C, ResizeLaunch* L);
void launch_resize(const ResizeLaunch& L, hipStream_t s);         // dispatch.cpp: checks, then the kernel
void launch_resize_kernel(const ResizeLaunch& L, hipStream_t s);  // resize.hip
// Convenience: builds the two tap tables, uploads them on the stream and launches.
void resize_device(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch, int W2,
                   int H2, ResizeMode mode, hipStream_t s);

// Orientation and crop of a whole frame (csrc/hip/orient.hip k_orient; the rule:
// stripe/orient.h).  Plain 64-bit addressing on arbitrary pitched views: no
// alignment of base pointers or pitches is assumed, no byte outside the w * C
// bytes of each source-window row is read and no byte outside the W2 * C bytes
// of each destination row is written, so a crop is only a view of the source
// (src + y0 * pitch + x0 * C).
//
// `none` and `flipv` copy rows (kOrientCopyRows per workgroup, 16 bytes per
// lane at the destination's own 16-byte boundaries).  Every other orientation
// stages a tile of the source in LDS, orient_tile_rows(T) source rows of
// orient_seg_px(C, T) pixels, and gathers destination dwords from it: the
// destination tile is seg x rows pixels (w x h) for `fliph` / `rot180` and
// rows x seg for the transposing four.  For those the LDS image pads behind
// every group of four rows, so that the four-byte gathers of 32 neighbouring
// lanes, which are four source rows apart, fall on different banks.
constexpr int kOrientCopyRows = 4;  // rows per workgroup of the copying instances
constexpr int orient_tile_rows(bool T) { return T ? 128 : 64; }  // source rows of a tile
constexpr int orient_seg_px(int C, bool T) {                     // source pixels per tile row
  return T ? (C == 1 ? 128 : 64) : (C == 1 ? 256 : 128);
}
// seg bytes + 3 bytes of address phase
constexpr int orient_row_dwords(int C, bool T) { return (orient_seg_px(C, T) * C + 3 + 3) / 4; }
// four rows and the pad
constexpr int orient_group_dwords(int C, bool T) { return 4 * orient_row_dwords(C, T) + (T ? (C == 1 ? 1 : 2) : 0); }
constexpr int orient_lds_bytes(int C, bool T) { return orient_tile_rows(T) / 4 * orient_group_dwords(C, T) * 4; }
struct OrientLaunch {
  const uint8_t* src = nullptr;  // the source window (already cropped)
  int64_t src_pitch = 0;
  int w = 0, h = 0, C = 0;       // the source window, pixels
  uint8_t* dst = nullptr;        // (T ? h : w) x (T ? w : h) pixels
  int64_t dst_pitch = 0;
  Orient op = Orient::None;
  // optional: the allocations the views lie in (checked against the rows touched)
  const uint8_t* src_base = nullptr;
  int64_t src_bytes = 0;
  const uint8_t* dst_base = nullptr;
  int64_t dst_bytes = 0;
};
void launch_orient(const OrientLaunch& L, hipStream_t s);         // dispatch.cpp: checks, then the kernel
void launch_orient_kernel(const OrientLaunch& L, hipStream_t s);  // orient.hip
// Convenience: `crop` is a window of the oriented W x H frame (empty: all of
// it); maps it to the source window and launches.  dst holds crop.w x crop.h
// pixels (the whole oriented frame without a crop).
void orient_device(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch,
                   Orient op, const CropRect& crop, hipStream_t s);

// Affine warp of a whole frame (csrc/hip/warp.hip k_warp; the rule:
// stripe/warp.h).  Addressing as k_orient: 64-bit on arbitrary pitched views,
// no alignment assumed, no byte outside the W * C bytes of a source row read,
// no byte outside the W2 * C bytes of a destination row written.
//
// A workgroup owns a destination tile of kWarpTile x kWarpTile pixels; a lane
// computes four neighbouring pixels of a row and stores them as dwords.  Two
// instances per (C, mode, border, nt):
//   * staged: the exact integer map at the tile's four corners bounds the
//     source box (the map is affine), which is clipped to the frame and staged
//     in LDS, kWarpBox rows of kWarpBox pixels at most (16-byte loads from each
//     row's own first byte, single bytes at its end); the taps are gathered
//     from LDS.  kWarpBox covers every rotation at scale <= 1: a row of A with
//     |A[i][0]| + |A[i][1]| <= sqrt(2) * 2^24 spans floor(63 * sqrt(2)) = 89
//     pixels over a tile, + 1 for the rounding of the two ends, + 1 for the
//     tap, + 1 for the count.
//   * direct: per-tap global byte loads with the same arithmetic, for every
//     other map (strong minification), so that no valid map is refused.
// warp_plan is the choice, from A and the tile constants alone.
constexpr int kWarpTile = 64;  // destination pixels per tile side
constexpr int kWarpBox = 92;   // source pixels per side of the staged box, at most
// bytes of a staged row in LDS: the box's bytes in whole dwords, an odd number of
// them (23 gray, 69 RGB), so that a gather that walks down the rows (a quarter
// turn) spreads over the banks
constexpr int warp_row_bytes(int C) { return (((kWarpBox * C + 3) / 4) | 1) * 4; }
constexpr int warp_lds_bytes(int C) { return kWarpBox * warp_row_bytes(C); }
// pixels a row of A spans over a tile, taps and rounding included
inline int64_t warp_box_span(int32_t a0, int32_t a1) {
  const int64_t s = (int64_t)(kWarpTile - 1) * ((a0 < 0 ? -(int64_t)a0 : a0) + (a1 < 0 ? -(int64_t)a1 : a1));
  return (s >> kWarpQ) + 3;
}
inline bool warp_plan_staged(const WarpMap& m) {
  return warp_box_span(m.A[0][0], m.A[0][1]) <= kWarpBox && warp_box_span(m.A[1][0], m.A[1][1]) <= kWarpBox;
}
struct WarpLaunch {
  const uint8_t* src = nullptr;
  int64_t src_pitch = 0;
  int W = 0, H = 0, C = 0;  // the source, pixels
  uint8_t* dst = nullptr;   // map.W2 x map.H2 pixels
  int64_t dst_pitch = 0;
  WarpMap map;
  // optional: the allocations the views lie in (checked against the rows touched)
  const uint8_t* src_base = nullptr;
  int64_t src_bytes = 0;
  const uint8_t* dst_base = nullptr;
  int64_t dst_bytes = 0;
};
void launch_warp(const WarpLaunch& L, hipStream_t s);         // dispatch.cpp: checks, then the kernel
void launch_warp_kernel(const WarpLaunch& L, hipStream_t s);  // warp.hip
void warp_device(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch,
                 const WarpMap& map, hipStream_t s);

// Mesh warp of a whole frame (csrc/hip/remap.hip k_remap; the rule:
// stripe/remap.h).  Addressing as k_warp.  The mesh lives on the device; the
// host never reads it, so the kernel decides per tile:
//   * spacing >= kRemapLdsSpacing: the tile's nodes (at most kRemapNodes a
//     side) go to LDS and their minimum and maximum bound the tile's source box
//     (a bilinear patch lies in the hull of its nodes).  A box of at most
//     kWarpBox pixels a side is staged in LDS with k_warp's loads and gathered
//     with coordinates relative to it (32 bits); a larger one gathers from
//     global memory in int64, for that tile alone (a workgroup-uniform branch).
//     A box that misses the frame under `constant` stores the fill byte.
//   * smaller spacings: nodes from global memory per pixel, taps from global
//     memory.
// Every node index is clamped to the mesh and every tap clamped or tested, so
// no mesh, whatever it holds, reads outside the frame.
constexpr int kRemapLdsSpacing = 4;
constexpr int kRemapNodes = kWarpTile / kRemapLdsSpacing + 1;  // 17
constexpr int remap_node_bytes() { return kRemapNodes * kRemapNodes * 2 * 4; }
constexpr int kRemapReduceBytes = 4 * 4 * 4;  // four waves' minima and maxima
constexpr int remap_lds_bytes(int C) { return warp_lds_bytes(C) + remap_node_bytes() + kRemapReduceBytes; }
struct RemapLaunch {
  const uint8_t* src = nullptr;
  int64_t src_pitch = 0;
  int W = 0, H = 0, C = 0;  // the source, pixels
  uint8_t* dst = nullptr;   // mesh.W2 x mesh.H2 pixels
  int64_t dst_pitch = 0;
  RemapMesh mesh;           // nodes: device memory
  int64_t mesh_count = 0;   // int32 values behind mesh.nodes
  // optional: the allocations the views lie in (checked against the rows touched)
  const uint8_t* src_base = nullptr;
  int64_t src_bytes = 0;
  const uint8_t* dst_base = nullptr;
  int64_t dst_bytes = 0;
};
void launch_remap(const RemapLaunch& L, hipStream_t s);         // dispatch.cpp: checks, then the kernel
void launch_remap_kernel(const RemapLaunch& L, hipStream_t s);  // remap.hip
void remap_device(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch,
                  const RemapMesh& mesh, int64_t mesh_count, hipStream_t s);

// Connected components of a 1-channel mask (csrc/hip/components.hip k_ccl_*; the
// rule: stripe/components.h).  Addressing as k_orient: 64-bit on pitched views,
// the source pitch any value >= W at any alignment, no byte outside a source
// row's W bytes read, nothing outside a label row's W ints written (the label
// pitch counts int32 elements; the plane is aligned to 4 bytes).
//
// The label plane is the union-find forest while a call runs (a slot holds its
// parent's raster index + 1; the numbers pass through the roots' own slots as
// negatives), so a call needs no second plane: beyond the labels it uses
// (H + 3) u32 of device memory, cached per device and H.  k_ccl_tile labels
// kCclTile x kCclTile tiles in LDS, ccl_lds_bytes() of u32 local indices (LDS
// atomics are 32 bits wide); k_ccl_number keeps one count per wave.
// components_device returns N after the call's one host synchronisation, and
// raises there if a union-find loop overran its step cap of W * H + 2.
constexpr int kCclTile = 64;       // pixels per tile side
constexpr int kCclStatSeg = 4096;  // pixels of a row that one wave of k_ccl_stats walks
constexpr int ccl_lds_bytes() { return kCclTile * kCclTile * 4; }
constexpr int ccl_number_lds_bytes() { return 4 * 4; }  // four waves' root counts
constexpr int ccl_scan_lds_bytes() { return 256 * 4; }  // one partial sum per thread
struct ComponentsLaunch {
  const uint8_t* src = nullptr;
  int64_t src_pitch = 0;  // bytes
  int W = 0, H = 0, conn = 8;
  int32_t* labels = nullptr;
  int64_t labels_pitch = 0;  // int32 elements
  // optional: the allocations the views lie in (checked against the rows touched)
  const uint8_t* src_base = nullptr;
  int64_t src_bytes = 0;
  const uint8_t* labels_base = nullptr;
  int64_t labels_bytes = 0;
};
int launch_components(const ComponentsLaunch& L, hipStream_t s);          // dispatch.cpp: checks, then the kernels
int launch_components_kernels(const ComponentsLaunch& L, hipStream_t s);  // components.hip
int components_device(const uint8_t* src, int64_t src_pitch, int W, int H, int conn, int32_t* labels,
                      int64_t labels_pitch, hipStream_t s);
// The table of the labels 0 .. N into `stats`, (N + 1) x kStatCols int64 on the
// device (k_ccl_stats: 64-bit atomics, exact and independent of their order; a
// wave holds the background and its most frequent foreground label in registers
// over kCclStatSeg pixels of a row and issues one set of atomics per horizontal
// run of every other label).  Synchronises the stream and refuses a plane
// that holds a label outside 0 .. N (such a label writes nothing).
struct ComponentStatsLaunch {
  const int32_t* labels = nullptr;
  int64_t labels_pitch = 0;
  int W = 0, H = 0, N = 0;
  int64_t* stats = nullptr;
};
void launch_component_stats(const ComponentStatsLaunch& L, hipStream_t s);          // dispatch.cpp
void launch_component_stats_kernels(const ComponentStatsLaunch& L, hipStream_t s);  // components.hip
void component_stats_device(const int32_t* labels, int64_t labels_pitch, int W, int H, int N, int64_t* stats,
                            hipStream_t s);
// The area filter (k_ccl_select): dst = src where the pixel is foreground and
// its label's area lies in amin .. amax, else 0.  Asynchronous.
struct AreaFilterLaunch {
  const uint8_t* src = nullptr;
  int64_t src_pitch = 0;
  int W = 0, H = 0;
  const int32_t* labels = nullptr;
  int64_t labels_pitch = 0;
  const int64_t* stats = nullptr;  // the device table of component_stats_device
  int N = 0;
  int64_t amin = 1, amax = kAreaNoLimit;
  uint8_t* dst = nullptr;
  int64_t dst_pitch = 0;
};
void launch_area_filter(const AreaFilterLaunch& L, hipStream_t s);         // dispatch.cpp
void launch_area_filter_kernel(const AreaFilterLaunch& L, hipStream_t s);  // components.hip
void area_filter_device(const uint8_t* src, int64_t src_pitch, int W, int H, const int32_t* labels,
                        int64_t labels_pitch, const int64_t* stats, int N, int64_t amin, int64_t amax, uint8_t* dst,
                        int64_t dst_pitch, hipStream_t s);

// Exact squared Euclidean distance transform of a 1-channel mask and the disc
// morphology on it (csrc/hip/distance.hip k_edt_*; the rule: stripe/distance.h).
// Addressing as k_orient: 64-bit on pitched views, the source pitch any value
// >= W at any alignment, no byte outside a source row's W bytes read, nothing
// outside a destination row's W elements written (the pitch of an int32 plane
// counts elements; the plane is aligned to 4 bytes).
//
// Column pass: k_edt_bits packs the site bits of bands of kEdtBand rows into one
// u64 per column and band, k_edt_carry walks the H / kEdtBand words per column,
// k_edt_band writes g (u16, 0xFFFF: no site in the column).  Row pass: k_edt_row,
// one workgroup of kEdtRowThreads per row (kEdtRowsPerGroup = 1) with g and the
// arg-mins in LDS, edt_row_lds_bytes(wmax) for the width class wmax of
// kEdtWidths; divide and conquer on the monotone arg-min, O(W log W) per row
// whatever the mask holds; ranges of more than kEdtLong candidates are scanned
// by a wave each from a list of kEdtList entries.  The store is templated on
// int32 d2 / u8 floor(sqrt) / u8 mask.  No host synchronisation; scratch
// (2 B / pixel of g and 1 bit / pixel of site words, for open / close one u8
// mask) is cached per device, stream, W and H until distance_release_scratch.
constexpr int kEdtBand = 64;          // rows per band of the column pass: one u64 of site bits
constexpr int kEdtRowThreads = 512;   // threads of a row-pass workgroup
constexpr int kEdtRowsPerGroup = 1;   // rows per row-pass workgroup
constexpr int kEdtLong = 64;          // a range of more candidates than this is scanned by a wave
constexpr int kEdtList = 1024;        // entries of a level's list of long ranges
constexpr int kEdtCounters = 20;      // one list length per level (at most 17)
constexpr int kEdtWidths[3] = {4096, 16384, 32768};  // the row pass's LDS classes: W <= these
constexpr int edt_width_class(int W) { return W <= kEdtWidths[0] ? 0 : W <= kEdtWidths[1] ? 1 : 2; }
constexpr int edt_row_lds_bytes(int wmax) { return 4 * wmax + 2 * kEdtList + 4 * kEdtCounters; }
struct DistanceLaunch {
  const uint8_t* src = nullptr;
  int64_t src_pitch = 0;  // bytes
  int W = 0, H = 0;
  bool to_foreground = false;
  int mode = 0;   // DistanceMode
  int64_t t = 0;  // the masks' threshold
  void* dst = nullptr;    // int32 (Squared) or u8
  int64_t dst_pitch = 0;  // elements of the destination's type
};
void launch_distance(const DistanceLaunch& L, hipStream_t s);          // dispatch.cpp: checks, then the kernels
void launch_distance_kernels(const DistanceLaunch& L, hipStream_t s);  // distance.hip
// op: DiskOp; L.t = floor(r^2); L.mode and L.to_foreground are set per step.
void launch_disk_morph(const DistanceLaunch& L, int op, hipStream_t s);          // dispatch.cpp
void launch_disk_morph_kernels(const DistanceLaunch& L, int op, hipStream_t s);  // distance.hip
void distance_device(const uint8_t* src, int64_t src_pitch, int W, int H, bool to_foreground, int mode, int64_t t,
                     void* dst, int64_t dst_pitch, hipStream_t s);
void disk_morph_device(const uint8_t* src, int64_t src_pitch, int W, int H, int op, int64_t t, uint8_t* dst,
                       int64_t dst_pitch, hipStream_t s);
void distance_release_scratch();  // frees the cached scratch of every device (waits for the devices)

// Integral images and the window operations on them (csrc/hip/integral.hip
// k_sat_*; the rule: stripe/integral.h).  Addressing as k_orient: 64-bit on
// pitched views, the source pitch any value >= W at any alignment, no byte
// outside a source row's W bytes read, nothing outside a destination row's
// elements written (W + 1 int32 per row of the integral, whose pitch counts
// elements and whose plane is aligned to 4 bytes; W bytes of a window result).
//
// Reduce, carry, scan over wave tiles of kSatTile x kSatTile pixels of the
// extended frame, kSatWaves tiles side by side per workgroup: k_sat_reduce
// writes column, row and tile totals, k_sat_carry prefix-sums them,
// k_sat_scan writes the wrapping u32 table with a DPP wave scan per row; no
// kernel uses LDS (sat_lds_bytes).  k_sat_window reads four corners per table
// and stores kSatWindowPixels bytes per lane.  No host synchronisation; the
// aggregates and the window operations' tables are cached per device, stream,
// extended size and number of tables until integral_release_scratch.
constexpr int kSatTile = 64;          // rows and columns of a wave's tile
constexpr int kSatWaves = 4;          // wave tiles side by side in a workgroup
constexpr int kSatWindowPixels = 4;   // pixels per lane of k_sat_window
constexpr int sat_lds_bytes() { return 0; }
struct IntegralLaunch {
  const uint8_t* src = nullptr;
  int64_t src_pitch = 0;  // bytes
  int W = 0, H = 0;
  bool squared = false;
  int32_t* dst = nullptr;  // (H + 1) x (W + 1)
  int64_t dst_pitch = 0;   // elements
};
struct WindowLaunch {
  const uint8_t* src = nullptr;
  int64_t src_pitch = 0;
  int W = 0, H = 0;
  int op = 0;  // WindowOp
  int K = 1;
  int border = 0;  // Border
  int C = 0;
  int64_t kq = 0;
  uint8_t* dst = nullptr;
  int64_t dst_pitch = 0;
};
void launch_integral(const IntegralLaunch& L, hipStream_t s);          // dispatch.cpp: checks, then the kernels
void launch_integral_kernels(const IntegralLaunch& L, hipStream_t s);  // integral.hip
void launch_window(const WindowLaunch& L, hipStream_t s);              // dispatch.cpp
void launch_window_kernels(const WindowLaunch& L, hipStream_t s);      // integral.hip
void integral_device(const uint8_t* src, int64_t src_pitch, int W, int H, bool squared, int32_t* dst, int64_t dst_pitch,
                     hipStream_t s);
void window_device(const uint8_t* src, int64_t src_pitch, int W, int H, int op, int K, int border, int C, int64_t kq,
                   uint8_t* dst, int64_t dst_pitch, hipStream_t s);
void integral_release_scratch();  // frees the cached scratch of every device (waits for the devices)

// The first three passes of the labelling (k_ccl_tile, k_ccl_seam, k_ccl_flatten)
// on their own, for callers that need the forest but no numbering (the
// hysteresis of canny.hip): queued on s, after which every foreground slot of
// the label plane holds its root's raster index + 1 (the root its own) and the
// background 0.  The call takes the components' cache lock and hands it over:
// the caller queues its own kernels, reads *err back (non-zero: a union-find
// loop overran its cap of `cap` steps), synchronises s once and only then lets
// the lock go, the same contract as components_device.
struct CclForest {
  std::unique_lock<std::mutex> lock;
  const uint32_t* err = nullptr;  // device
  uint32_t cap = 0;
};
CclForest launch_ccl_forest(const ComponentsLaunch& L, hipStream_t s);  // components.hip; L is taken as checked

// Canny edge detection and hysteresis thresholding of a 1-channel frame
// (csrc/hip/canny.hip k_canny_*; the rule: stripe/canny.h).  Addressing as
// k_orient: 64-bit on pitched views, the source pitch any value >= W at any
// alignment, no byte outside a source row's W bytes read, nothing outside a
// destination row's W bytes written.
//
// k_canny_nms<L2>: a workgroup per tile of kCannyTileX x kCannyTileY pixels.
// The source goes once into LDS with a 2-pixel apron, the border applied at load
// time; the magnitudes (with the sector in the top bits) of the tile plus a
// 1-pixel apron go to LDS, 0 outside the frame; after a barrier every lane
// classifies kCannyPixels pixels in a row and stores their class bytes
// (canny_nms_lds_bytes()).  k_canny_classify is hysteresis_threshold's
// pointwise class map.  The hysteresis runs launch_ccl_forest on the class
// plane (class != 0 is foreground), then k_canny_mark (every class 2 pixel
// stores -(r) into the slot of its root r - 1; all writers store the same
// value, a reader takes |slot|) and k_canny_select (255 where the class is >= 1
// and the root's slot is negative).  No kernel but k_canny_nms uses LDS.
// The class plane (H rows of W bytes at a pitch rounded up to 4) and the forest
// plane (W * H int32) are cached per device, stream and size until
// canny_release_scratch.  canny_device and hysteresis_device synchronise the
// stream once, to read the forest's error word; canny_classes_device does not.
constexpr int kCannyTileX = 64;  // pixels of a tile of k_canny_nms across
constexpr int kCannyTileY = 32;  // and down
constexpr int kCannyPixels = 4;  // pixels in a row per lane (all k_canny_* kernels)
constexpr int canny_nms_lds_bytes() {
  return (kCannyTileX + 4) * (kCannyTileY + 4) + (kCannyTileX + 2) * (kCannyTileY + 2) * 4;  // source bytes, u32
}
enum class CannyStage : int { Canny = 0, Classes = 1, Hysteresis = 2 };
struct CannyLaunch {
  const uint8_t* src = nullptr;
  int64_t src_pitch = 0;  // bytes
  int W = 0, H = 0;
  int stage = 0;          // CannyStage
  int64_t low = 0, high = 0;
  int norm = 0;           // CannyNorm (Canny, Classes)
  int border = 0;         // Border (Canny, Classes)
  int conn = 8;           // Hysteresis (Canny: 8)
  uint8_t* dst = nullptr;
  int64_t dst_pitch = 0;
};
void launch_canny(const CannyLaunch& L, hipStream_t s);          // dispatch.cpp: checks, then the kernels
void launch_canny_kernels(const CannyLaunch& L, hipStream_t s);  // canny.hip
void canny_device(const uint8_t* src, int64_t src_pitch, int W, int H, int low, int high, int norm, int border,
                  uint8_t* dst, int64_t dst_pitch, hipStream_t s);
void canny_classes_device(const uint8_t* src, int64_t src_pitch, int W, int H, int low, int high, int norm, int border,
                          uint8_t* dst, int64_t dst_pitch, hipStream_t s);
void hysteresis_device(const uint8_t* src, int64_t src_pitch, int W, int H, int low, int high, int conn, uint8_t* dst,
                       int64_t dst_pitch, hipStream_t s);
void canny_release_scratch();  // frees the cached scratch of every device (waits for the devices)

// Write the x-margins of rows [y0, y1) of a stripe from its own pixels.
void launch_fill_margins(uint8_t* origin, int64_t pitch, int W, int C, int y0, int y1, int px,
                         Border b, hipStream_t s);

// Copy `rows` rows of E bytes between pitched device buffers (packed staging
// buffers <-> padded stripes; the e2e path's SDMA-friendly 1-D transfers).
void launch_copy_rows(uint8_t* dst, int64_t dpitch, const uint8_t* src, int64_t spitch, int64_t E, int rows,
                      hipStream_t s);

// Up to kCopyMultiMax independent device copies in one launch (the `local`
// hub's halo rounds: every rank's halo rows of one exchange).
constexpr int kCopyMultiMax = 16;
struct CopyDesc {
  const uint8_t* src = nullptr;
  uint8_t* dst = nullptr;
  int64_t bytes = 0;
};
void launch_copy_multi(const CopyDesc* d, int n, hipStream_t s);

// Same-box streaming floor: a hand-written linear device copy of `bytes`
// (csrc/hip/pointwise.hip k_copy_linear) rotating over `frames` buffer pairs
// (frames x 2 x bytes > 2 x 256 MiB: every copy reads cache-cold data), the
// faster of two store policies.  event_ms: median device time of one copy
// (events between copies); burst_ms: mean per copy of `reps` back-to-back.
struct CopyRoofline {
  double event_ms = 0, burst_ms = 0;
  int64_t bytes = 0;
  int frames = 0;
  int policy = 0;  // store aux of the faster per-copy time (0 default, 16 write-through)
};
CopyRoofline copy_roofline(int device, int64_t bytes, int frames, int reps);

// Transport check (comm_ring_check): fill `bytes` (a multiple of 4) with the
// pattern of `tag` / add the number of differing words to *errors (device).
void launch_pattern_fill(void* p, int64_t bytes, uint32_t tag, hipStream_t s);
void launch_pattern_check(const void* p, int64_t bytes, uint32_t tag, unsigned long long* errors, hipStream_t s);

// Synthetic pixels for local rows [0, rows) (global row0..), margins included.
void launch_synth(uint8_t* origin, int64_t pitch, int W, int C, int row0, int rows, uint64_t seed,
                  int margin_px, Border b, hipStream_t s);

// Build the device constant block of a conv pass (MFMA operand tables).
void prepare_conv_consts(const Pass& p, PassConsts* pc, hipStream_t s);

// Small general conv (K <= 7) on the VALU (csrc/hip/stencil.hip k_conv_small).
bool conv_small_supported(const Pass& p);
// The stencil launch honours PassLaunch::order (separable task order) for
// this pass: plain separable passes with symmetric vertical taps (no gray /
// LUT prologue, no expand epilogue).  The autotuner probes the order only here.
bool sep_order_supported(const Pass& p);
void launch_conv_small(const Pass& p, const PassLaunch& L, hipStream_t s);

// Separable (rank-one) conv on MFMA (csrc/hip/blur_sep.hip).
bool sep_supported(const Pass& p);
void prepare_sep_consts(const Pass& p, PassConsts* pc, hipStream_t s);
void launch_blur_sep(const Pass& p, const PassConsts& pc, const PassLaunch& L, hipStream_t s);

// ---- JPEG pixel stages on the device (csrc/hip/jpeg_dev.hip) ----
// IDCT + chroma upsampling + YCbCr -> RGB of entropy-decoded coefficients into
// interleaved rows of `pitch` bytes at dst (device), queued on s.
void jpeg_pixels_device(const JpegCoefs& jc, uint8_t* dst, int64_t pitch, hipStream_t s);
// Colour conversion, chroma subsampling, forward DCT and quantisation of an
// interleaved device frame; returns the coefficients (host) for
// jpeg_entropy_encode (synchronises s).
JpegQuant jpeg_quantise_device(const uint8_t* src, int64_t pitch, int W, int H, int C, int quality, bool subsample,
                               hipStream_t s);

}  // namespace stripe
