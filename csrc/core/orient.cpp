// Orientation rule (see orient.h): names, the group table, the crop parser, the
// golden loop and the Exif Orientation reader.
#include "stripe/orient.h"

#include <cstring>

namespace stripe {

namespace {
// Exif order: index i is Exif value i + 1
constexpr Orient kExifOrder[8] = {Orient::None,      Orient::FlipH, Orient::Rot180,     Orient::FlipV,
                                  Orient::Transpose, Orient::Rot90, Orient::Transverse, Orient::Rot270};

// source (row, column) of output pixel (y, x); the source is h x w
inline void source_of(Orient op, int w, int h, int y, int x, int* r, int* c) {
  const int u = orient_t(op) ? x : y, v = orient_t(op) ? y : x;
  *r = orient_fy(op) ? h - 1 - u : u;
  *c = orient_fx(op) ? w - 1 - v : v;
}

std::string name_list() {
  std::string s;
  for (const std::string& n : orient_names()) s += (s.empty() ? "" : " | ") + n;
  return s + " | cw | ccw | exif:1..8";
}

// all of s as a decimal integer in [0, kOrientMaxSize]; -1 otherwise
int parse_uint(const std::string& s) {
  if (s.empty() || s.size() > 5) return -1;
  int v = 0;
  for (char c : s) {
    if (c < '0' || c > '9') return -1;
    v = v * 10 + (c - '0');
  }
  return v <= kOrientMaxSize ? v : -1;
}
}  // namespace

const std::vector<std::string>& orient_names() {
  static const std::vector<std::string> names = {"none",      "fliph", "rot180",     "flipv",
                                                 "transpose", "rot90", "transverse", "rot270"};
  return names;
}

const char* orient_name(Orient o) {
  for (int i = 0; i < 8; ++i)
    if (kExifOrder[i] == o) return orient_names()[(size_t)i].c_str();
  return "?";
}

Orient orient_from_exif(int v) {
  STRIPE_CHECK(v >= 1 && v <= 8, "orient: Exif orientation " << v << " outside 1..8");
  return kExifOrder[v - 1];
}

Orient parse_orient(const std::string& token) {
  const std::vector<std::string>& names = orient_names();
  for (int i = 0; i < 8; ++i)
    if (token == names[(size_t)i]) return kExifOrder[i];
  if (token == "cw") return Orient::Rot90;
  if (token == "ccw") return Orient::Rot270;
  if (token.size() == 6 && token.compare(0, 5, "exif:") == 0 && token[5] >= '1' && token[5] <= '8')
    return kExifOrder[token[5] - '1'];
  fail("orient: unknown orientation '" + token + "' (" + name_list() + ")");
}

// The table comes from the rule itself: a 2 x 3 frame has no symmetry, so the
// composite of two ops matches exactly one of the eight.
Orient orient_compose(Orient a, Orient b) {
  const int w = 3, h = 2;
  const int wa = orient_t(a) ? h : w, ha = orient_t(a) ? w : h;  // the frame after a
  const int wb = orient_t(b) ? ha : wa, hb = orient_t(b) ? wa : ha;
  for (int k = 0; k < 8; ++k) {
    const Orient c = (Orient)k;
    if ((orient_t(c) ? h : w) != wb) continue;
    bool same = true;
    for (int y = 0; y < hb && same; ++y)
      for (int x = 0; x < wb && same; ++x) {
        int r1, c1, r0, c0, rc, cc;
        source_of(b, wa, ha, y, x, &r1, &c1);
        source_of(a, w, h, r1, c1, &r0, &c0);
        source_of(c, w, h, y, x, &rc, &cc);
        same = r0 == rc && c0 == cc;
      }
    if (same) return c;
  }
  fail("orient: composition not found");
}

Orient orient_inverse(Orient a) {
  for (int k = 0; k < 8; ++k)
    if (orient_compose(a, (Orient)k) == Orient::None) return (Orient)k;
  fail("orient: inverse not found");
}

CropRect parse_crop_spec(const std::string& token) {
  const std::string what = "crop spec '" + token + "': ";
  const size_t x = token.find('x');
  const size_t p1 = token.find('+');
  const size_t p2 = p1 == std::string::npos ? p1 : token.find('+', p1 + 1);
  STRIPE_CHECK(x != std::string::npos && p1 != std::string::npos && p2 != std::string::npos && x < p1,
               what << "expected WxH+X+Y");
  CropRect c;
  c.w = parse_uint(token.substr(0, x));
  c.h = parse_uint(token.substr(x + 1, p1 - x - 1));
  c.x0 = parse_uint(token.substr(p1 + 1, p2 - p1 - 1));
  c.y0 = parse_uint(token.substr(p2 + 1));
  STRIPE_CHECK(c.w >= 0 && c.h >= 0 && c.x0 >= 0 && c.y0 >= 0,
               what << "W, H, X and Y must be integers in 0.." << kOrientMaxSize);
  STRIPE_CHECK(c.w >= 1 && c.h >= 1, what << "empty window");
  return c;
}

void check_crop(const CropRect& c, int W, int H, const std::string& token) {
  STRIPE_CHECK(c.w >= 1 && c.h >= 1, "crop '" << token << "': empty window (frame " << W << "x" << H << ")");
  STRIPE_CHECK(c.x0 >= 0 && c.y0 >= 0 && (int64_t)c.x0 + c.w <= W && (int64_t)c.y0 + c.h <= H,
               "crop '" << token << "': window " << c.w << "x" << c.h << "+" << c.x0 << "+" << c.y0
                        << " leaves the frame of " << W << "x" << H);
}

CropRect orient_source_window(Orient op, int w, int h, const CropRect& crop) {
  if (crop.empty()) return CropRect{0, 0, w, h};
  // the oriented frame's x runs over source columns (T = 0) or source rows (T = 1)
  const bool t = orient_t(op);
  const int u0 = t ? crop.x0 : crop.y0, un = t ? crop.w : crop.h;  // source rows, before FY
  const int v0 = t ? crop.y0 : crop.x0, vn = t ? crop.h : crop.w;  // source columns, before FX
  CropRect s;
  s.y0 = orient_fy(op) ? h - u0 - un : u0;
  s.h = un;
  s.x0 = orient_fx(op) ? w - v0 - vn : v0;
  s.w = vn;
  return s;
}

Image golden_orient(const Image& in, Orient op, const CropRect& crop) {
  STRIPE_CHECK(in.C == 1 || in.C == 3, "orient: image must have 1 or 3 channels, got C = " << in.C);
  STRIPE_CHECK(in.W >= 1 && in.H >= 1 && in.W <= kOrientMaxSize && in.H <= kOrientMaxSize,
               "orient: size " << in.W << "x" << in.H << " outside 1.." << kOrientMaxSize);
  const int OW = orient_t(op) ? in.H : in.W, OH = orient_t(op) ? in.W : in.H;
  CropRect c = crop;
  if (c.empty()) c = CropRect{0, 0, OW, OH};
  check_crop(c, OW, OH, std::to_string(c.w) + "x" + std::to_string(c.h) + "+" + std::to_string(c.x0) + "+" +
                            std::to_string(c.y0));
  Image out(c.w, c.h, in.C, NoInit{});
  for (int y = 0; y < c.h; ++y)
    for (int x = 0; x < c.w; ++x) {
      int r, col;
      source_of(op, in.W, in.H, c.y0 + y, c.x0 + x, &r, &col);
      for (int ch = 0; ch < in.C; ++ch) out.row(y)[(size_t)x * in.C + ch] = in.row(r)[(size_t)col * in.C + ch];
    }
  return out;
}

// ---- Exif Orientation of a JPEG stream ----
namespace {
struct Span {
  const uint8_t* p;
  size_t n;
  bool le;
  bool has(size_t off, size_t len) const { return off <= n && len <= n - off; }
  uint32_t u16(size_t off) const { return le ? p[off] | (p[off + 1] << 8) : (p[off] << 8) | p[off + 1]; }
  uint32_t u32(size_t off) const {
    return le ? (uint32_t)p[off] | ((uint32_t)p[off + 1] << 8) | ((uint32_t)p[off + 2] << 16) |
                    ((uint32_t)p[off + 3] << 24)
              : ((uint32_t)p[off] << 24) | ((uint32_t)p[off + 1] << 16) | ((uint32_t)p[off + 2] << 8) |
                    (uint32_t)p[off + 3];
  }
};

// the TIFF structure of an Exif segment: header, IFD0, tag 0x0112
int tiff_orientation(const uint8_t* p, size_t n) {
  Span t{p, n, true};
  if (!t.has(0, 8)) return 1;
  if (p[0] == 'I' && p[1] == 'I') t.le = true;
  else if (p[0] == 'M' && p[1] == 'M') t.le = false;
  else return 1;
  if (t.u16(2) != 42) return 1;
  const size_t ifd = t.u32(4);
  if (!t.has(ifd, 2)) return 1;
  const size_t count = t.u16(ifd);
  for (size_t e = 0; e < count; ++e) {
    const size_t eo = ifd + 2 + 12 * e;
    if (!t.has(eo, 12)) return 1;
    if (t.u16(eo) != 0x0112) continue;
    if (t.u16(eo + 2) != 3 || t.u32(eo + 4) != 1) return 1;  // SHORT, count 1
    const uint32_t v = t.u16(eo + 8);
    return v >= 1 && v <= 8 ? (int)v : 1;
  }
  return 1;
}
}  // namespace

int jpeg_orientation(const uint8_t* p, size_t n) noexcept {
  if (!p || n < 4 || p[0] != 0xFF || p[1] != 0xD8) return 1;
  int found = 1;
  bool seen = false;
  size_t pos = 2;
  for (;;) {
    if (n - pos < 2 || p[pos] != 0xFF) return 1;
    const uint8_t m = p[pos + 1];
    if (m == 0xFF) {  // fill byte
      ++pos;
      continue;
    }
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) {  // stand-alone markers
      pos += 2;
      continue;
    }
    if (m == 0xD9) return 1;  // EOI before any scan
    if (n - pos < 4) return 1;
    const size_t len = ((size_t)p[pos + 2] << 8) | p[pos + 3];
    if (len < 2 || len > n - pos - 2) return 1;  // truncated segment
    if (m == 0xDA) {                             // first SOS: the stream must close behind it
      for (size_t q = n - 1; q > pos + 2 + len; --q)
        if (p[q] == 0xD9 && p[q - 1] == 0xFF) return found;
      return 1;
    }
    if (m == 0xE1 && !seen && len >= 8 && std::memcmp(p + pos + 4, "Exif\0\0", 6) == 0) {
      seen = true;  // the first Exif segment decides
      found = tiff_orientation(p + pos + 10, len - 8);
    }
    pos += 2 + len;
  }
}

}  // namespace stripe
