// Canny edge detection and hysteresis thresholding of a 1-channel frame (a
// whole-frame operation behind the chain, with entry points of its own; not a
// chain token).  Everything is integer and bit-exact across golden_*, the host
// executor (cpu_canny / cpu_hysteresis_threshold, cpu_exec.cpp) and the GPU
// kernels (csrc/hip/canny.hip k_canny_*, with the forest passes of
// csrc/hip/components.hip).
//
// Input: one frame, 1 channel, u8, W, H >= 1, W * H <= kComponentsMaxPixels.
//
// canny(x, low, high, norm, border) -> u8, 255 on an edge, 0 elsewhere.
//
// Border: reflect101, replicate or constant through border_index of common.h
// (skip is refused).  P is the frame extended with it.
//
// Gradient, at every pixel of the frame, from the 3 x 3 neighbourhood in P with
// stencil_defs.h's Sobel taps:
//   Gx = [1,2,1]^T (x) [-1,0,1],  Gy = [-1,0,1]^T (x) [1,2,1];  |Gx|, |Gy| <= 1020.
//
// Magnitude m:  norm l1: |Gx| + |Gy| (<= 2040), compared with low and high;
//               norm l2: Gx^2 + Gy^2 (<= 2 080 800, fits u32), compared with
//               low^2 and high^2; no square root is taken.
// The magnitude of a position outside the frame is 0: the gradient is not
// evaluated there, so frame-edge pixels can be edges.
//
// Thresholds: integers, 0 <= low <= high <= kCannyMaxThreshold (2040).
//
// Direction sector, integers only, ax = |Gx|, ay = |Gy|, T = kCannyTan = 13573 =
// round(tan 22.5 deg * 2^15) (every term stays below 2^31):
//   (ay << 15) < ax T               horizontal gradient: the neighbours (x-1, y), (x+1, y);
//                                   the pixel survives iff m > m(x-1, y) and m >= m(x+1, y)
//   (ay << 15) > ax T + (ax << 16)  vertical gradient: (x, y-1), (x, y+1);
//                                   survives iff m > m(x, y-1) and m >= m(x, y+1)
//   otherwise                       diagonal: (x-s, y-1), (x+s, y+1) with s = +1 if Gx and
//                                   Gy have the same sign, else -1 (both are nonzero here:
//                                   ax = 0 or ay = 0 lands in the first two rows; Gx = Gy = 0
//                                   falls through to this row, where m = 0 survives nothing);
//                                   survives iff m > both, strictly
// The asymmetric > / >= of the horizontal and vertical sectors is deliberate:
// of a plateau two pixels wide across the gradient exactly one pixel survives
// (the left / upper one), where two strict tests would drop both and two
// non-strict ones keep both.  The diagonal tests are both strict.
//
// Class: 0 unless the pixel survives and m > low; otherwise 2 if m > high,
// else 1.  (canny_classes gives this plane: 0 / 1 / 2.)
//
// hysteresis_threshold(x, low, high, connectivity) -> u8 mask, 255 or 0: the
// class comes straight from the pixel, 2 if p > high, 1 if p > low, else 0,
// with 0 <= low <= high <= kHysteresisMaxThreshold (255).
//
// Hysteresis: a pixel is an edge iff its class is >= 1 and its connected
// component among the pixels of class >= 1 holds at least one pixel of class 2.
// Connectivity is 8 for canny, 4 or 8 for hysteresis_threshold.  The result is
// a fixed point and does not depend on any visiting order.
//
// Out of scope: apertures other than 3, a built-in pre-blur (chain gaussian5
// in front, as `stripe edges --chain gaussian5` does), RGB and batches,
// fractional thresholds, multi-rank frames, a chain token, sub-pixel edges,
// gradient and direction planes as outputs.
#pragma once

#include <cstdint>
#include <string>

#include "stripe/common.h"
#include "stripe/components.h"
#include "stripe/image.h"

namespace stripe {

constexpr int kCannyMaxThreshold = 2040;      // 2 * 1020: the largest l1 magnitude
constexpr int kHysteresisMaxThreshold = 255;  // the largest pixel
constexpr int kCannyTan = 13573;              // round(tan 22.5 deg * 2^15)

enum class CannyNorm : int { L1 = 0, L2 = 1 };

// "l1" / "l2"; anything else is refused.
CannyNorm parse_canny_norm(const std::string& token);
const char* canny_norm_name(CannyNorm n);
// The one message for thresholds: refuses unless 0 <= low <= high <= max.
void check_thresholds(int64_t low, int64_t high, int max);
// Refuses, with the messages every layer shares: C != 1 (says to convert first), W or H < 1,
// W * H > kComponentsMaxPixels, thresholds outside 0 <= low <= high <= 2040, an unknown norm, the skip border.
void check_canny(int W, int H, int C, int64_t low, int64_t high, int norm, Border border);
// The same for the frame; thresholds up to 255; a connectivity other than 4 / 8.
void check_hysteresis(int W, int H, int C, int64_t low, int64_t high, int conn);

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STRIPE_CANNY_HD __host__ __device__
#else
#define STRIPE_CANNY_HD
#endif

// Sectors: the two neighbours of (x, y) are (x - dx, y - dy) and (x + dx, y + dy).
constexpr int kCannyHorizontal = 0, kCannyVertical = 1, kCannyDiagonal = 2, kCannyAntiDiagonal = 3;

STRIPE_CANNY_HD inline uint32_t canny_magnitude(int gx, int gy, bool l2) {
  const uint32_t ax = (uint32_t)(gx < 0 ? -gx : gx), ay = (uint32_t)(gy < 0 ? -gy : gy);
  return l2 ? ax * ax + ay * ay : ax + ay;
}

STRIPE_CANNY_HD inline int canny_sector(int gx, int gy) {
  const int ax = gx < 0 ? -gx : gx, ay = gy < 0 ? -gy : gy;
  if ((ay << 15) < ax * kCannyTan) return kCannyHorizontal;
  if ((ay << 15) > ax * kCannyTan + (ax << 16)) return kCannyVertical;
  return (gx < 0) == (gy < 0) ? kCannyDiagonal : kCannyAntiDiagonal;  // s = +1 : s = -1
}
// (dx, dy) of a sector
STRIPE_CANNY_HD inline int canny_dx(int sector) {
  return sector == kCannyVertical ? 0 : sector == kCannyAntiDiagonal ? -1 : 1;
}
STRIPE_CANNY_HD inline int canny_dy(int sector) { return sector == kCannyHorizontal ? 0 : 1; }

// The class of a pixel of magnitude m whose neighbours along its gradient have the magnitudes before (at
// (x - dx, y - dy)) and after; lo, hi: low, high under l1, their squares under l2.
STRIPE_CANNY_HD inline uint8_t canny_class(uint32_t m, uint32_t before, uint32_t after, int sector, uint32_t lo,
                                           uint32_t hi) {
  const bool survives = m > before && (sector <= kCannyVertical ? m >= after : m > after);
  return !survives || m <= lo ? 0 : m > hi ? 2 : 1;
}
STRIPE_CANNY_HD inline uint8_t hysteresis_class(uint32_t p, uint32_t lo, uint32_t hi) { return p > hi ? 2 : p > lo ? 1 : 0; }

// The plain oracle of the class plane (0 / 1 / 2): the extended frame written out, then a magnitude plane, then
// the rule, as plain loops.
Image golden_canny_classes(const Image& img, int low, int high, CannyNorm norm, Border border);
// 255 where the class is >= 1 and the component (among class >= 1, connectivity conn) holds a class 2 pixel: a
// raster scan that starts a flood fill with an explicit stack at every unvisited class 2 pixel.
Image golden_hysteresis(const Image& classes, int conn);
Image golden_canny(const Image& img, int low, int high, CannyNorm norm, Border border);
Image golden_hysteresis_threshold(const Image& img, int low, int high, int conn);

// Host executor on pitched views (pitches in bytes).  cpu_canny_classes: row blocks on threads, each
// recomputing the magnitude rows it needs above and below (identical at any thread count).  cpu_hysteresis:
// cpu_components on the class plane, a flag per label from the class 2 pixels, and the selection.
void cpu_canny_classes(const uint8_t* src, int64_t src_pitch, int W, int H, int low, int high, CannyNorm norm,
                       Border border, uint8_t* dst, int64_t dst_pitch, int threads);
void cpu_hysteresis(const uint8_t* classes, int64_t classes_pitch, int W, int H, int conn, uint8_t* dst,
                    int64_t dst_pitch, int threads);
void cpu_canny(const uint8_t* src, int64_t src_pitch, int W, int H, int low, int high, CannyNorm norm, Border border,
               uint8_t* dst, int64_t dst_pitch, int threads);
void cpu_hysteresis_threshold(const uint8_t* src, int64_t src_pitch, int W, int H, int low, int high, int conn,
                              uint8_t* dst, int64_t dst_pitch, int threads);

}  // namespace stripe
