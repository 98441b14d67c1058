// Resize: nearest, bilinear and area scaling of a whole frame (a stage in
// front of the chain, like JPEG decode; not a chain token).
//
// One rule, bit-identical in every layer.  resize_taps() is the only place
// that computes weights, in integer arithmetic; the golden loop, the host
// executor (cpu_resize) and the GPU kernel (csrc/hip/resize.hip k_resize)
// consume its Q15 output.  Per channel, horizontal first, then vertical:
//
//   h'(y, ox)  = (sum_t wx[ox][t] * p(y, fx[ox] + t) + 64) >> 7          8.8 fixed point, <= 65280
//   out(oy,ox) = (sum_t wy[oy][t] * h'(fy[oy] + t, ox) + (1 << 22)) >> 23  <= 255 without a clamp
//
// The weights of one output index sum to exactly 32768, so flat images are
// fixed points and equal sizes give the identity in every mode.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "stripe/image.h"

namespace stripe {

enum class ResizeMode : int {
  Auto = 0,      // per axis: area where it shrinks, bilinear where it grows, identity where unchanged
  Nearest = 1,   // i = floor((2o + 1) n_in / (2 n_out))
  Bilinear = 2,  // half-pixel centres, replicate at the ends, no antialiasing (cv::INTER_LINEAR geometry)
  Area = 3,      // exact overlap of output cell and input pixels (cv::INTER_AREA geometry), n_out <= n_in
};

constexpr int kResizeOne = 32768;      // Q15 one
constexpr int kResizeMaxFactor = 32;   // largest n_in / n_out of an area axis (count <= 33)
constexpr int kResizeMaxSize = 65535;  // largest size of an axis

const char* resize_mode_name(ResizeMode m);
ResizeMode parse_resize_mode(const std::string& s);

// "WxH[:mode]"
struct ResizeSpec {
  int W = 0, H = 0;
  ResizeMode mode = ResizeMode::Auto;
};
ResizeSpec parse_resize_spec(const std::string& token);

// Taps of one axis.  Output index o reads inputs first[o] .. first[o] + count[o] - 1
// with weights w[offset[o] .. offset[o + 1]); first and first + count are
// non-decreasing in o, and first[o] + count[o] <= n_in.
struct ResizeTaps {
  int n_in = 0, n_out = 0;
  int max_count = 0;
  std::vector<int32_t> first;
  std::vector<int32_t> offset;  // n_out + 1 entries; count[o] = offset[o + 1] - offset[o]
  std::vector<uint16_t> w;      // Q15, each in [0, 32768]
  int count(int o) const { return offset[(size_t)o + 1] - offset[(size_t)o]; }
};
ResizeTaps resize_taps(int n_in, int n_out, ResizeMode mode);

// The per-pixel oracle: the rule above as a plain loop.
Image golden_resize(const Image& in, int W2, int H2, ResizeMode mode);

// Host executor: a horizontal pass per input row into a u16 row, a vertical
// pass over the rows an output row needs, row blocks on `threads` threads.
// Each source row of a block is reduced horizontally once.  Bit-identical to
// golden_resize at any thread count.  Views are pitched (pitch >= W * C).
void cpu_resize(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch, int W2,
                int H2, ResizeMode mode, int threads);
Image cpu_resize(const Image& in, int W2, int H2, ResizeMode mode, int threads);

}  // namespace stripe
