// Distance transform of a mask: the exact squared Euclidean distance plane and
// what follows from it, morphology by a disc of any radius (a whole-frame
// operation behind the chain, with entry points of its own; not a chain token).
//
// Input: one frame, 1 channel, u8, 1 <= W, H <= kDistanceMaxSide (d^2 then stays
// below 2 * 32766^2 < 2^31).  A pixel is foreground iff its byte is != 0.
//
// Polarity: `to background` (the default, scipy's distance_transform_edt): the
// sites are the background pixels, every pixel gets the squared distance to the
// nearest site and a site gets 0.  `to foreground`: the same with the roles
// swapped.  Pixels outside the frame are neither: the frame edge is not a site.
//
// squared: int32, H x W, d2(p) = min over the sites q of (px - qx)^2 + (py - qy)^2.
// A frame without any site is kDistanceNone everywhere.  Only distances are
// returned, so the plane is unique: no tie has to be broken.
//
// Derived from d2:
//   u8     min(255, floor(sqrt(d2))) with an exact integer root; kDistanceNone -> 255
//   float  the front end's: sqrt in float64 rounded to float32, kDistanceNone -> +inf
//   mask   u8, 255 where d2 > t (keep_above) or d2 <= t (keep_within), else 0
//
// Disc morphology, by composition, with t = floor(r^2) for a real radius r >= 0
// (the structuring element is {dx^2 + dy^2 <= t}); the results are 0 / 255 masks:
//   erode_disk  = mask(d2 to background >  t)   (the frame edge does not erode)
//   dilate_disk = mask(d2 to foreground <= t)
//   open_disk   = dilate(erode),  close_disk = erode(dilate)
// r = 0 is the identity on the binarised mask.
//
// golden_distance is the one definition (column scans, then the minimum over
// every column by brute force); the host executor (cpu_distance, cpu_exec.cpp)
// and the GPU kernels (csrc/hip/distance.hip k_edt_*) are bit-identical to it.
//
// Out of scope: the nearest-site indices (feature transform), cityblock and
// chessboard metrics, multi-rank frames, batches, watershed and skeletons, a
// chain token.
#pragma once

#include <climits>
#include <cstdint>
#include <string>
#include <vector>

#include "stripe/image.h"

namespace stripe {

constexpr int kDistanceMaxSide = 32767;
constexpr int32_t kDistanceNone = INT32_MAX;

// What the row pass stores (the _C bindings' `mode`).
enum class DistanceMode : int { Squared = 0, U8 = 1, MaskAbove = 2, MaskWithin = 3 };
enum class DiskOp : int { Erode = 0, Dilate = 1, Open = 2, Close = 3 };

// "background" / "foreground" -> to_foreground; "erode" / "dilate" / "open" / "close".
bool parse_distance_to(const std::string& token);
DiskOp parse_disk_op(const std::string& token);
// Refuses, with the messages every layer shares: C != 1 (says to convert first),
// W or H < 1, a side > kDistanceMaxSide.
void check_distance(int W, int H, int C);
// Refuses a negative or non-finite radius; returns t = floor(r^2), at most
// INT32_MAX - 1 (kDistanceNone stays above every threshold).
int32_t check_radius(double r);
// Refuses a mode outside DistanceMode and a negative threshold.
void check_distance_mode(int mode, int64_t t);

// floor(sqrt(d2)) clamped to 255, exact.
inline uint8_t distance_u8(int32_t d2) {
  if (d2 >= 255 * 255) return 255;
  int r = 0;
  while ((r + 1) * (r + 1) <= d2) ++r;  // at most 255 steps
  return (uint8_t)r;
}
inline uint8_t distance_mask(int32_t d2, int32_t t, bool keep_above) { return (d2 > t) == keep_above ? 255 : 0; }

// The plain oracle, O(W^2 H): out is resized to W * H.
void golden_distance(const Image& img, bool to_foreground, std::vector<int32_t>* out);
Image golden_distance_u8(const Image& img, bool to_foreground);
Image golden_distance_mask(const Image& img, bool to_foreground, int32_t t, bool keep_above);
Image golden_disk_morph(const Image& img, DiskOp op, double radius);

// Host executor on pitched views (out_pitch in int32 elements): a column pass
// over column blocks, then per row the lower envelope of the parabolas
// (Meijster's form, integers only) over row blocks.  golden_distance's plane at
// any thread count.
void cpu_distance(const uint8_t* src, int64_t src_pitch, int W, int H, bool to_foreground, int32_t* out,
                  int64_t out_pitch, int threads);
Image cpu_distance_u8(const Image& img, bool to_foreground, int threads);
Image cpu_distance_mask(const Image& img, bool to_foreground, int32_t t, bool keep_above, int threads);
Image cpu_disk_morph(const Image& img, DiskOp op, double radius, int threads);

}  // namespace stripe
