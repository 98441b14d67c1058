// Orientation and crop of a whole frame (a stage in front of the chain, like
// JPEG decode and resize; not a chain token).
//
// The eight orientations are the dihedral group of the rectangle.  Each is
// three bits, T (transpose), FX and FY.  The source is h rows x w pixels:
//
//   (u, v) = T ? (x, y) : (y, x)            u: source row index, v: source column index
//   out[y][x] = in[FY ? h-1-u : u][FX ? w-1-v : v]      output: (T ? w : h) rows x (T ? h : w) pixels
//
//   name        T FX FY  Exif   numpy
//   none        0 0  0   1      a
//   fliph       0 1  0   2      a[:, ::-1]
//   rot180      0 1  1   3      a[::-1, ::-1]
//   flipv       0 0  1   4      a[::-1]
//   transpose   1 0  0   5      a.transpose(1, 0, 2)
//   rot90 (cw)  1 0  1   6      np.rot90(a, -1)
//   transverse  1 1  1   7      a[::-1, ::-1].transpose(1, 0, 2)
//   rot270(ccw) 1 1  0   8      np.rot90(a, 1)
//
// The Exif column is the operation that displays an image stored with that
// Orientation tag value upright.  golden_orient is the one definition of the
// pixels; the host executor (cpu_orient) and the GPU kernel
// (csrc/hip/orient.hip k_orient) are bit-identical to it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "stripe/image.h"

namespace stripe {

// bits: T << 2 | FX << 1 | FY
enum class Orient : int {
  None = 0,
  FlipV = 1,
  FlipH = 2,
  Rot180 = 3,
  Transpose = 4,
  Rot90 = 5,
  Rot270 = 6,
  Transverse = 7,
};
constexpr bool orient_t(Orient o) { return ((int)o & 4) != 0; }
constexpr bool orient_fx(Orient o) { return ((int)o & 2) != 0; }
constexpr bool orient_fy(Orient o) { return ((int)o & 1) != 0; }

constexpr int kOrientMaxSize = 65535;  // largest size of an axis

// The eight names in Exif order (index i is Exif value i + 1).
const std::vector<std::string>& orient_names();
const char* orient_name(Orient o);
Orient orient_from_exif(int v);  // 1..8
// A name, an alias (cw = rot90, ccw = rot270) or exif:N, N = 1..8.
Orient parse_orient(const std::string& token);
Orient orient_inverse(Orient a);
Orient orient_compose(Orient a, Orient b);  // a, then b

// A window of x0 .. x0 + w - 1, y0 .. y0 + h - 1; w == 0: the whole frame.
struct CropRect {
  int x0 = 0, y0 = 0, w = 0, h = 0;
  bool empty() const { return w == 0; }
};
// "WxH+X+Y": a window in the oriented frame (the frame the user sees).
CropRect parse_crop_spec(const std::string& token);
// Refuses a window that is empty or leaves the W x H frame; `token` names it.
void check_crop(const CropRect& c, int W, int H, const std::string& token);
// The window of the w x h source whose orientation by `op` is the window
// `crop` of the oriented frame (crop.empty(): the whole source).
CropRect orient_source_window(Orient op, int w, int h, const CropRect& crop);

// The per-pixel loop of the rule; `crop` in the oriented frame.
Image golden_orient(const Image& in, Orient op, const CropRect& crop = {});

// Host executor on pitched views: src is the w x h source window (already
// cropped: see orient_source_window), dst the (T ? h : w) x (T ? w : h)
// result.  Row blocks on `threads` threads; the non-transposing ops are row
// copies (FX: a pixel-order reversal of the row), the transposing ops go
// through square tiles so that neither side is walked at a whole row's stride.
// Bit-identical to golden_orient at any thread count.
constexpr int kCpuOrientTile = 32;  // pixels per tile side of the transposing ops
void cpu_orient(const uint8_t* src, int64_t src_pitch, int w, int h, int C, uint8_t* dst, int64_t dst_pitch, Orient op,
                int threads);
Image cpu_orient(const Image& in, Orient op, const CropRect& crop, int threads);

// Exif Orientation (tag 0x0112 of IFD0) of a JPEG stream, 1..8; 1 whenever the
// stream does not carry a well-formed one: no APP1 segment beginning with
// "Exif\0\0" in front of the first SOS, a truncated segment or stream (the
// marker segments up to SOS must be whole and an EOI must follow it), offsets
// outside the segment, a type other than SHORT, a count other than 1, a value
// outside 1..8.  The input is untrusted: every read is bounds-checked, nothing
// outside [p, p + n) is read, and nothing is thrown.
int jpeg_orientation(const uint8_t* p, size_t n) noexcept;

}  // namespace stripe
