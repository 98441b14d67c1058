// Integral images: the summed-area table of a 1-channel frame and the window
// operations that read it in O(1) per pixel for any odd window K: box filter,
// local standard deviation and the mean / Niblack / Sauvola local thresholds (a
// whole-frame operation behind the chain, with entry points of its own; not a
// chain token).  Everything is integer and bit-exact across golden_*, the host
// executor (cpu_integral / cpu_window, cpu_exec.cpp) and the GPU kernels
// (csrc/hip/integral.hip k_sat_*).
//
// Input: one frame, 1 channel, u8, 1 <= W, H <= kIntegralMaxSide.
//
// Window: K odd, R = K / 2, N = K * K.  The frame is extended by R on every side
// with the Border (reflect101, replicate, constant; skip is refused) through
// border_index of common.h, which is applied repeatedly, so R may exceed the
// frame.  With P the extended frame: A = sum of P and B = sum of P^2 over the
// K x K window centred on the pixel.
//
// Limits: K <= kWindowMaxK (4095) for the operations that use A only
// (255 N + N / 2 < 2^32), K <= kWindowMaxKSquares (255) for those that use B
// (65025 N < 2^32).
//
// integral (the public form, OpenCV's layout): (H + 1) x (W + 1) int32, row 0 and
// column 0 zero, I[y][x] = sum over y' < y, x' < x of p (of p^2 with `squared`),
// modulo 2^32 in two's complement like cv::integral CV_32S.
//
// Wrapped tables: a rectangle sum below 2^32 is exact as I[d] - I[b] - I[c] + I[a]
// in wrapping u32 even when the table itself has wrapped, and the two K limits
// keep every window sum below 2^32.  Every layer works this way; none keeps a
// 64-bit table.
//
// Window operations (m = (A + N / 2) / N, V = N B - A^2 in u64, never negative,
// below 2^48; isqrt is the exact floor root):
//   box          m                                      (box3 / box5's rule, DIV = N)
//   std          isqrt(V) / N, floor (<= 127)
//   mean:C       p > m - C ? 255 : 0, C in [-255, 255]  (threshold:adaptive:K:C)
//   niblack:k:C  4096 (p N - A + C N) > kq isqrt(V) ? 255 : 0
//   sauvola:k    4096 (p N - A) N 128 > kq A (isqrt(V) - 128 N) ? 255 : 0
//                (p > m (1 + k (s / 128 - 1)) with m = A / N, s = isqrt(V) / N)
// kq = nearbyint(4096 k), ties to even, |k| <= kWindowMaxAbsK = 4.  All sides fit
// int64 (the largest: 16384 * 255 N * 128 N, about 0.25 * 2^63 at K = 255).
//
// Out of scope: RGB (planes can go through one at a time), rectangular windows,
// a chain token, multi-rank frames, a fused sliding-sum box that never writes the
// table, 64-bit tables.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "stripe/common.h"
#include "stripe/image.h"

namespace stripe {

constexpr int kIntegralMaxSide = 32767;
constexpr int kWindowMaxK = 4095;         // operations that use A only
constexpr int kWindowMaxKSquares = 255;   // operations that use B
constexpr int kWindowMaxAbsK = 4;         // |k| of niblack / sauvola
constexpr int kWindowMaxAbsC = 255;       // |C| of mean / niblack

enum class WindowOp : int { Box = 0, Std = 1, Mean = 2, Niblack = 3, Sauvola = 4 };
constexpr int kWindowOps = 5;
inline bool window_uses_squares(WindowOp op) { return op == WindowOp::Std || op == WindowOp::Niblack || op == WindowOp::Sauvola; }

struct WindowSpec {
  WindowOp op = WindowOp::Box;
  int K = 1;
  int C = 0;   // mean, niblack
  int kq = 0;  // niblack, sauvola: nearbyint(4096 k)
};

// "box" / "std" / "mean" / "niblack" / "sauvola".
WindowOp parse_window_op(const std::string& token);
const char* window_op_name(WindowOp op);
// nearbyint(4096 k), ties to even; refuses a non-finite k and |k| > kWindowMaxAbsK.
int window_kq(double k);
// Refuses, with the messages every layer shares: C != 1 (says to convert first),
// W or H < 1, a side > kIntegralMaxSide.
void check_integral(int W, int H, int C);
// Refuses an unknown operation, an even K, K < 1, K above the operation's limit,
// the skip border, C or kq out of range (and C != 0 for sauvola).
void check_window(int op, int K, Border border, int C, int64_t kq);

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STRIPE_INTEGRAL_HD __host__ __device__
#else
#define STRIPE_INTEGRAL_HD
#endif

// The exact floor root of v < 2^48: the double-precision root plus a one-step correction either way.
STRIPE_INTEGRAL_HD inline uint64_t window_isqrt(uint64_t v) {
  uint64_t r = (uint64_t)sqrt((double)v);
  r -= r * r > v ? 1u : 0u;
  r += (r + 1) * (r + 1) <= v ? 1u : 0u;
  return r;
}

// One output byte from the pixel p, the window sums A and B (B is not read by box and mean) and N = K * K.
STRIPE_INTEGRAL_HD inline uint8_t window_rule(int op, uint32_t p, uint32_t A, uint32_t B, uint32_t N, int C, int kq) {
  if (op == (int)WindowOp::Box) return (uint8_t)((A + N / 2) / N);
  if (op == (int)WindowOp::Mean) return (int)p > (int)((A + N / 2) / N) - C ? 255 : 0;
  const uint64_t V = (uint64_t)N * B - (uint64_t)A * A;
  const int64_t s = (int64_t)window_isqrt(V);
  if (op == (int)WindowOp::Std) return (uint8_t)((uint32_t)s / N);
  const int64_t d = (int64_t)p * N - (int64_t)A;
  if (op == (int)WindowOp::Niblack) return 4096 * (d + (int64_t)C * N) > (int64_t)kq * s ? 255 : 0;
  return 4096 * d * N * 128 > (int64_t)kq * A * (s - 128 * (int64_t)N) ? 255 : 0;
}

// The public integral: (H + 1) x (W + 1) int32, packed; a plain double loop.
void golden_integral(const Image& img, bool squared, std::vector<int32_t>* out);
// The plain oracle: the extended frame written out, window sums by a separable K + K loop per pixel in u64.
Image golden_window(const Image& img, const WindowSpec& spec, Border border);

// Host executor on pitched views (out_pitch in int32 elements): block-local scans over row blocks plus carries.
void cpu_integral(const uint8_t* src, int64_t src_pitch, int W, int H, bool squared, int32_t* out, int64_t out_pitch,
                  int threads);
// The wrapping u32 tables of the extended frame, then four corners per table and pixel over row blocks.
void cpu_window(const uint8_t* src, int64_t src_pitch, int W, int H, const WindowSpec& spec, Border border, uint8_t* dst,
                int64_t dst_pitch, int threads);

}  // namespace stripe
