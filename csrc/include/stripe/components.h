// Connected components of a mask: labels, a table of statistics and an area
// filter (a whole-frame operation behind the chain, with entry points of its
// own; not a chain token).
//
// Input: one frame, 1 channel, u8, W * H <= 2^31 - 2.  A pixel is foreground
// iff its byte is != 0.  Connectivity 4 joins the W / E / N / S neighbours,
// 8 adds the four diagonals.
//
// Labels: int32, H x W.  0 is the background; the components are numbered
// 1 .. N in raster order of their first pixel (smallest y, then smallest x).
// That is the numbering scipy.ndimage.label gives, and the one a union-find
// whose parents always point at the smaller raster index gives for free: a
// component's root is its first pixel.  Nothing depends on thread counts, tile
// sizes or the order atomics arrive in.
//
// Stats: int64, (N + 1) x kStatCols, row l for label l (row 0: the background):
//
//   area, x0, y0, x1, y1, sum_x, sum_y
//
// x0, y0 are inclusive minima, x1, y1 exclusive maxima (the slices of
// ndimage.find_objects), sum_x / sum_y the sums of the pixel coordinates (a
// centroid is sum / area; no rounding is decided here).  A label without pixels
// (only the background of an all-foreground frame) is all zeros.
//
// Area filter: out[p] = src[p] if p is foreground and
// amin <= area(label[p]) <= amax, else 0; shape and dtype of the source.
//
// golden_components is the one definition (a raster scan that starts a flood
// fill with an explicit stack at every unlabelled foreground pixel); the host
// executor (cpu_components, cpu_exec.cpp) and the GPU kernels
// (csrc/hip/components.hip k_ccl_*) are bit-identical to it.
//
// Out of scope: multi-rank labelling (merging labels across the stripe seams
// between ranks), batches, labels as a chain token, contours and moments beyond
// the seven columns.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "stripe/image.h"

namespace stripe {

constexpr int kStatCols = 7;  // area, x0, y0, x1, y1, sum_x, sum_y
constexpr int64_t kComponentsMaxPixels = (int64_t(1) << 31) - 2;
constexpr int64_t kAreaNoLimit = INT64_MAX;

// "4" or "8"; anything else is refused.
int parse_connectivity(const std::string& token);
// Refuses, with the messages every layer shares: W or H < 1, C != 1 (says to
// convert first), W * H > kComponentsMaxPixels, a connectivity other than 4 / 8.
void check_components(int W, int H, int C, int conn);
// Refuses amin < 1 and amax < amin.
void check_area_bounds(int64_t amin, int64_t amax);

// The plain oracle: labels is resized to W * H; returns N.
int golden_components(const Image& img, int conn, std::vector<int32_t>* labels);
// The table of the labels 0 .. N; refuses a label outside 0 .. N.
std::vector<int64_t> component_stats(const int32_t* labels, int64_t labels_pitch, int W, int H, int N);
Image golden_area_filter(const Image& img, int conn, int64_t amin, int64_t amax);

// Host executor on pitched views (pitches in elements).  Run-based two-pass
// union-find with the label plane itself as the forest (a slot holds its
// parent's raster index + 1): row blocks on `threads` threads, each linking
// the runs of its rows, then the block seams, a flatten, a prefix count of the
// roots per block and the numbering.  Parents always point at the smaller
// raster index, so the result is golden_components' at any thread count.
// The rows are split into min(threads, H) blocks whatever the frame's size.
int cpu_components(const uint8_t* src, int64_t src_pitch, int W, int H, int conn, int32_t* labels, int64_t labels_pitch,
                   int threads);
// Row blocks on threads, per-thread tables reduced at the end.
std::vector<int64_t> cpu_component_stats(const int32_t* labels, int64_t labels_pitch, int W, int H, int N, int threads);
Image cpu_area_filter(const Image& img, int conn, int64_t amin, int64_t amax, int threads);

}  // namespace stripe
