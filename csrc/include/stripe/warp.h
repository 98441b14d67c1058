// Affine warp of a whole frame: rotation by any angle and warpAffine (a stage in
// front of the chain, after orientation / crop and before resize; not a chain
// token).
//
// A warp is a 2 x 3 matrix.  The parser takes the forward matrix M (source ->
// destination, as cv::warpAffine without WARP_INVERSE_MAP), an inverse matrix,
// or a rotation; it inverts in double and quantises the inverse map Minv to
// Q24.  Nothing after the parser touches floating point:
//
//   A[i][j] = nearbyint(2^24 * Minv[i][j])   int32, |Minv[i][j]| < 64
//   B[i]    = nearbyint(2^24 * Minv[i][2])   int64, |Minv[i][2]| < 2^20
//
// Integer pixel indices are pixel centres (OpenCV's convention).  For the
// output pixel (x, y), in int64 (every term below 2^48):
//
//   sx = A00 * x + A01 * y + B0        sy = A10 * x + A11 * y + B1
//
//   nearest:  ix = (sx + 2^23) >> 24, iy likewise (>> is floor); out = p(iy, ix)
//   bilinear: X = (sx + 2^15) >> 16 (a Q8 position), ix = X >> 8, fx = X & 255,
//             the same for Y, iy, fy;
//             top = (256 - fx) * p(iy, ix) + fx * p(iy, ix + 1), bot on row iy + 1,
//             out = ((256 - fy) * top + fy * bot + 32768) >> 16      (<= 255)
//
// A tap outside the frame is an ordinary tap: the fill byte under `constant`
// (one value for all channels), the clamped pixel under `replicate`.  A map
// that shrinks is not antialiased (as bilinear resize).
//
// golden_warp is the one definition of the pixels; the host executor
// (cpu_warp) and the GPU kernel (csrc/hip/warp.hip k_warp) are bit-identical
// to it.
#pragma once

#include <cstdint>
#include <string>

#include "stripe/image.h"

namespace stripe {

enum class WarpMode : int { Bilinear = 0, Nearest = 1 };
enum class WarpBorder : int { Constant = 0, Replicate = 1 };

constexpr int kWarpMaxSize = 65535;  // largest size of an axis
constexpr int kWarpQ = 24;           // fraction bits of the map
constexpr double kWarpMaxLinear = 64.0;               // |Minv[i][j]| below this
constexpr double kWarpMaxOffset = 1048576.0;          // |Minv[i][2]| below this (2^20)

struct WarpMap {
  int32_t A[2][2] = {{1 << kWarpQ, 0}, {0, 1 << kWarpQ}};
  int64_t B[2] = {0, 0};
  int W2 = 0, H2 = 0;  // the destination
  WarpMode mode = WarpMode::Bilinear;
  WarpBorder border = WarpBorder::Constant;
  uint8_t fill = 0;
};

const char* warp_mode_name(WarpMode m);
const char* warp_border_name(WarpBorder b);
WarpMode parse_warp_mode(const std::string& token);  // bilinear | nearest
// constant[:V] | replicate; V in 0..255 (default 0)
void parse_warp_border(const std::string& token, WarpBorder* border, uint8_t* fill);

// The one quantiser.  M is row-major {a, b, c, d, e, f}: the forward matrix, or
// (inverse) the map from destination to source itself.  W x H is the source,
// W2 x H2 the destination.  Refuses, naming `token`: non-finite numbers, a
// singular matrix, an inverse outside the ranges above, sizes outside
// 1..kWarpMaxSize.
WarpMap warp_quantise(const double M[6], bool inverse, int W, int H, int W2, int H2,
                      WarpMode mode = WarpMode::Bilinear, WarpBorder border = WarpBorder::Constant, uint8_t fill = 0,
                      const std::string& token = "matrix");

// Rotation by `deg` degrees, counter-clockwise as seen (cv::getRotationMatrix2D,
// PIL), about the source centre ((W - 1) / 2, (H - 1) / 2), which maps to the
// destination's centre.  With c, s = cos, sin of the angle reduced mod 360
// (exactly 0, +-1 at multiples of 90):
//   minv = {c, -s, csx - c cdx + s cdy,  s, c, csy - s cdx - c cdy}
// fit: W2 = max(1, ceil(W |c| + H |s| - 1e-6)), H2 = max(1, ceil(W |s| + H |c| - 1e-6));
// otherwise W2 x H2 = W x H.
struct Rotation {
  double minv[6];
  int W2, H2;
};
Rotation rotate_matrix(double deg, bool fit, int W, int H);

// "a;b;c;d;e;f[:WxH]": the forward matrix and the destination size (0 x 0: the source's).
struct WarpSpec {
  double M[6];
  int W2 = 0, H2 = 0;
};
WarpSpec parse_warp_spec(const std::string& token);
// "DEG[:same|fit]"
struct RotateSpec {
  double deg = 0;
  bool fit = false;
};
RotateSpec parse_rotate_spec(const std::string& token);
// The canonical tokens the CLIs report: "rotate:DEG:same|fit", "affine:a;b;c;d;e;f:WxH".
std::string rotate_token(const RotateSpec& r);
std::string warp_token(const WarpSpec& s, int W2, int H2);
// The number handling of these specs and of the mesh warp's (remap.h).
namespace spec {
// all of s as a decimal number (digits, sign, point, exponent) or inf / nan, which the callers
// refuse by name; false for anything else (hexadecimal floats and white space included)
bool parse_number(const std::string& s, double* v);
// all of s as a decimal integer in [0, kWarpMaxSize]; -1 otherwise
int parse_uint(const std::string& s);
// the shortest decimal form that reads back exactly, without an exponent where there is one
std::string num(double v);
}  // namespace spec

// Source coordinates of one output pixel (shared by all layers).
inline int64_t warp_sx(const WarpMap& m, int x, int y) { return (int64_t)m.A[0][0] * x + (int64_t)m.A[0][1] * y + m.B[0]; }
inline int64_t warp_sy(const WarpMap& m, int x, int y) { return (int64_t)m.A[1][0] * x + (int64_t)m.A[1][1] * y + m.B[1]; }
#if defined(__HIPCC__) || defined(__CUDACC__)
#define STRIPE_WARP_HD __host__ __device__
#else
#define STRIPE_WARP_HD
#endif
// The bilinear blend of four taps with Q8 fractions (shared by all layers).
STRIPE_WARP_HD inline uint32_t warp_bilinear(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t fx,
                                             uint32_t fy) {
  const uint32_t top = (256u - fx) * p00 + fx * p01;
  const uint32_t bot = (256u - fx) * p10 + fx * p11;
  return ((256u - fy) * top + fy * bot + 32768u) >> 16;
}

// The per-pixel loop of the rule.
Image golden_warp(const Image& in, const WarpMap& map);

// Host executor on pitched views: src is W x H, dst map.W2 x map.H2.  Row
// blocks on `threads` threads; per output row the span of pixels whose taps
// are all inside the frame is found in integers and runs without border
// tests.  Bit-identical to golden_warp at any thread count.
void cpu_warp(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch,
              const WarpMap& map, int threads);
Image cpu_warp(const Image& in, const WarpMap& map, int threads);

}  // namespace stripe
