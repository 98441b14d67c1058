// Mesh warp of a whole frame: perspective warps, lens undistortion and remap
// (a stage in front of the chain, in the affine warp's slot; not a chain token).
//
// A mesh is a coarse grid of exact source positions, interpolated bilinearly in
// integers.  Spacing S = 2^s, s = 0..6; destination W2 x H2;
//
//   gw = ((W2 - 1) >> s) + 2,  gh = ((H2 - 1) >> s) + 2
//
// node (i, j) sits at destination pixel (j * S, i * S), so j + 1 and i + 1 exist
// for every pixel.  int32 mesh[gh][gw][2] holds the source position (mx, my) of
// each node in Q12, |v| < 2^18 pixels.  Integer indices are pixel centres, as in
// warp.h.  For the output pixel (x, y), in int64, per coordinate:
//
//   j = x >> s, tx = x & (S - 1);  i = y >> s, ty = y & (S - 1)
//   P = (S - tx)(S - ty) M[i][j] + tx (S - ty) M[i][j+1]
//     + (S - tx) ty M[i+1][j] + tx ty M[i+1][j+1]            Q(12 + 2s), |P| < 2^43
//
//   bilinear: X = (P + 2^(3+2s)) >> (4 + 2s) (a Q8 position, >> is floor),
//             ix = X >> 8, fx = X & 255, the same for Y; the four taps go
//             through warp_bilinear of warp.h
//   nearest:  ix = (P + 2^(11+2s)) >> (12 + 2s)
//
// A tap outside the frame is an ordinary tap: the fill byte or the clamped
// pixel, as in warp.h (WarpMode and WarpBorder are reused).  It follows that the
// identity mesh is the identity at every spacing, meshes of integer
// translations are exact, flat images are fixed points under `replicate`, and at
// S = 1 nothing is interpolated.
//
// Only the mesh builders touch floating point (double); each node is
// nearbyint(4096 * pos).  The automatic spacing is the largest S in 64, 32, .., 1
// whose interpolation error bound S^2 / 8 * (max|f_xx| + max|f_yy|) is at most
// 2^-10 pixel for both coordinates, from these sufficient bounds:
//   perspective, coordinate (a x + b y + c) / w with w = g x + h y + i:
//     2 (|g| (|a| + F |g|) + |h| (|b| + F |h|)) / w_min^2,
//     F the largest |f| and w_min the smallest w over the grid's corners
//   radial: (8 |k1| rho + 32 |k2| rho^3) / f, rho the farthest grid corner's
//     distance from the centre divided by f
// S = 1 always qualifies.  Against the same sampling in float64 with the exact
// map the pixels stay within 0.5 + 510 (2^-9 + 2^-10 + 2^-13) levels (Q8
// rounding, interpolation, node rounding).
//
// golden_remap is the one definition of the pixels; the host executor
// (cpu_remap) and the GPU kernel (csrc/hip/remap.hip k_remap) are bit-identical
// to it.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "stripe/image.h"
#include "stripe/warp.h"

namespace stripe {

constexpr int kRemapQ = 12;         // fraction bits of a node
constexpr int kRemapMaxShift = 6;   // S <= 64
constexpr int kRemapNodeBits = 18;  // |node| < 2^18 pixels

constexpr int remap_grid(int n, int s) { return ((n - 1) >> s) + 2; }

// A view of a mesh (host or device memory, as the layer that takes it).
struct RemapMesh {
  const int32_t* nodes = nullptr;  // gh x gw x 2
  int shift = 0;                   // s
  int W2 = 0, H2 = 0;              // the destination
  WarpMode mode = WarpMode::Bilinear;
  WarpBorder border = WarpBorder::Constant;
  uint8_t fill = 0;
  int gw() const { return remap_grid(W2, shift); }
  int gh() const { return remap_grid(H2, shift); }
};

// A mesh a builder made.
struct Mesh {
  std::vector<int32_t> nodes;
  int shift = 0, W2 = 0, H2 = 0;
  int spacing() const { return 1 << shift; }
  int gw() const { return remap_grid(W2, shift); }
  int gh() const { return remap_grid(H2, shift); }
  RemapMesh view(WarpMode mode, WarpBorder border, uint8_t fill) const {
    RemapMesh m;
    m.nodes = nodes.data(), m.shift = shift, m.W2 = W2, m.H2 = H2, m.mode = mode, m.border = border, m.fill = fill;
    return m;
  }
};

// s of a spacing; refuses, naming `token`, what is not a power of two in 1..64
int remap_shift(int spacing, const std::string& token = "mesh");
// Refuses a destination outside 1..kWarpMaxSize, a bad spacing, a node count that is not gh * gw * 2 and
// (host meshes: check_nodes) a node at or beyond 2^18 pixels.
void check_mesh(const RemapMesh& m, int64_t count, bool check_nodes, const std::string& token = "mesh");

// The perspective map of a 3 x 3 matrix Hm (row-major; the forward matrix, source -> destination, as
// cv::warpPerspective, or with `inverse` the map from destination to source itself).  spacing 0: automatic.
// Refuses, naming `token`: non-finite numbers, a singular matrix, the horizon crossing the destination,
// a node at or beyond 2^18 pixels, sizes outside 1..kWarpMaxSize, a bad spacing.
Mesh perspective_mesh(const double Hm[9], bool inverse, int W, int H, int W2, int H2, int spacing = 0,
                      const std::string& token = "perspective");
// cv::getPerspectiveTransform: the forward matrix (h22 = 1) that maps src[k] to dst[k]; points as x, y pairs.
void perspective_from_points(const double src[8], const double dst[8], double Hm[9],
                             const std::string& token = "points");

// "x0,y0;x1,y1;x2,y2;x3,y3[:WxH]": the source points TL, TR, BR, BL that map to the destination's corners.
// Without a size: rint(max(|TR - TL|, |BR - BL|)) + 1 by rint(max(|BL - TL|, |BR - TR|)) + 1.
struct QuadSpec {
  double pts[8];
  int W2 = 0, H2 = 0;
};
QuadSpec parse_quad_spec(const std::string& token);
void quad_default_size(const double pts[8], int* W2, int* H2, const std::string& token = "quad");
// the forward matrix of a quad and its destination size
void quad_matrix(const double pts[8], int W2, int H2, double Hm[9], const std::string& token = "quad");
// "h00;...;h22[:WxH]"
struct PerspectiveSpec {
  double Hm[9];
  int W2 = 0, H2 = 0;
};
PerspectiveSpec parse_perspective_spec(const std::string& token);
// "k1[;k2[;f[;cx;cy]]]"
struct RadialSpec {
  double k1 = 0, k2 = 0;
  bool has_f = false, has_centre = false;
  double f = 0, cx = 0, cy = 0;
};
RadialSpec parse_undistort_spec(const std::string& token);
// Radial undistortion: the destination has the source's size; xn = (x - cx) / f, yn = (y - cy) / f,
// r2 = xn^2 + yn^2, k = 1 + k1 r2 + k2 r2^2, pos = (cx + f xn k, cy + f yn k): cv::initUndistortRectifyMap
// with K = newK = [[f, 0, cx], [0, f, cy]] and dist = (k1, k2, 0, 0).  Defaults: f half the diagonal, the
// centre ((W - 1) / 2, (H - 1) / 2).  Refuses f <= 0 and what perspective_mesh refuses.
Mesh radial_mesh(const RadialSpec& r, int W, int H, int spacing = 0, const std::string& token = "undistort");

// f and the centre filled in with their defaults for a W x H frame
RadialSpec radial_resolve(const RadialSpec& r, int W, int H);
// The canonical tokens the CLIs report: "perspective:h00;...;h22:WxH", "quad:x0,y0;...;x3,y3:WxH",
// "undistort:k1;k2;f;cx;cy" (a resolved spec).
std::string perspective_token(const double Hm[9], int W2, int H2);
std::string quad_token(const double pts[8], int W2, int H2);
std::string undistort_token(const RadialSpec& resolved);

// P of one coordinate (c = 0: x, 1: y) of an output pixel (shared by the host layers).
inline int64_t remap_P(const int32_t* nodes, int gw, int s, int x, int y, int c) {
  const int64_t S = int64_t(1) << s;
  const int j = x >> s, i = y >> s;
  const int64_t tx = x & (S - 1), ty = y & (S - 1);
  const int32_t* n0 = nodes + ((size_t)i * gw + j) * 2 + c;
  const int32_t* n1 = n0 + (size_t)gw * 2;
  return (S - tx) * (S - ty) * n0[0] + tx * (S - ty) * n0[2] + (S - tx) * ty * n1[0] + tx * ty * n1[2];
}

// The per-pixel loop of the rule.
Image golden_remap(const Image& in, const RemapMesh& mesh);

// Host executor on pitched views: src is W x H, dst mesh.W2 x mesh.H2.  Row blocks on `threads` threads;
// per row and cell the incremental form of P (P = S L + tx (R - L), L and R the cell's left and right
// edges at the row).  Bit-identical to golden_remap at any thread count.
void cpu_remap(const uint8_t* src, int64_t src_pitch, int W, int H, int C, uint8_t* dst, int64_t dst_pitch,
               const RemapMesh& mesh, int threads);
Image cpu_remap(const Image& in, const RemapMesh& mesh, int threads);

}  // namespace stripe
