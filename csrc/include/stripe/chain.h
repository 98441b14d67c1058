// Chain compiler: turns the parsed filter list into fused passes.
//
// The reference launches one kernel per filter on the default stream
// (kernel.cu:192-195: gray, contrast, emboss = three full passes over the stripe,
// ~8 B/px of DRAM traffic).  Here every run of pointwise ops is folded into a
// 256-entry LUT program and fused into the load path (prologue) of the next
// stencil, or into the store path (epilogue) of the last one, so the reference's
// whole GPU chain becomes ONE kernel (3 B in + 1 B out per pixel).
#pragma once

#include <array>
#include <string>
#include <vector>

#include "stripe/filters.h"

namespace stripe {

// out = expand?( post( (gray | cmat)?( pre(p) ) ) )  -- all per-byte LUTs are exact
// u8 maps; cmat is a 3 -> 3 colour matrix (filters.h) in the slot gray has, and a
// program holds at most one of the two
struct PointwiseProgram {
  bool has_pre = false;
  std::array<uint8_t, 256> pre{};
  bool gray = false;
  GrayMode gmode = GrayMode::BT601;
  bool cmat = false;
  std::array<int, 12> cm{};  // Op::cm: q row-major, then qb
  bool has_post = false;
  std::array<uint8_t, 256> post{};
  bool expand = false;
  // A statistic op (OpKind::Stat: equalize, autocontrast, threshold:otsu) as the
  // program's FIRST stage.  Its table is built at run time from the histogram of
  // the pass's input (resolve_stat) and composed in front of `pre` (programs
  // with a gray or matrix stage; has_pre is set) or of `post` (otherwise;
  // has_post is set).  The tables here hold the static ops after it, so the
  // plan's structure never depends on table contents.
  bool has_stat = false;
  Op stat;

  bool identity() const { return !has_pre && !gray && !cmat && !has_post && !expand && !has_stat; }
  bool lut_only() const { return !gray && !cmat && !expand && !has_pre; }
  // Prologue of a stencil pass may gray-convert and LUT, but not pre-LUT, expand
  // or mix channels (a colour matrix always runs as a pointwise pass of its own).
  bool prologue_ok() const { return !has_pre && !expand && !cmat; }
  int channels_out(int cin) const { return expand ? 3 : (gray ? 1 : cin); }
  uint8_t apply_channel_lut(uint8_t v) const;  // post(pre(v)) when no gray
};

// Combine: a two-input pointwise pass (current, held) -> new current image; its
// `pro` holds at most a `post` table, the LUT-only run that followed the op.
enum class PassKind : int { Pointwise = 0, Separable = 1, Direct = 2, Conv = 3, Combine = 4 };

struct Pass {
  PassKind kind = PassKind::Pointwise;
  int cin = 3, cout = 3;   // channels read / written
  int cmid = 3;            // channels after the prologue (= stencil channel count)
  PointwiseProgram pro;    // Pointwise: the whole program; stencil: prologue
  bool has_epi = false;    // stencil epilogue LUT (channel count unchanged)
  std::array<uint8_t, 256> epi{};
  // stencil epilogue `expand`: the 1-channel result (after epi) is stored as 3
  // equal channels (cmid 1 -> cout 3), so gray -> stencil -> expand is one pass
  bool epi_expand = false;
  StencilId sid = StencilId::Gaussian5;
  int K = 1, R = 0;
  Border border = Border::Reflect101;
  std::vector<float> conv_w;  // Conv: K*K weights
  int conv_digits = 3;        // Conv: weight digits of the i8 MFMA path (Op::conv_digits)
  std::vector<float> sep_h, sep_v;  // Conv: 1-D factors of a rank-one window (separable MFMA path)
  // x-margin contract for the output (what the next stencil consumer needs)
  int out_margin_px = 0;
  Border out_margin_border = Border::Reflect101;
  // a gray:ref prologue's post LUT as clamp((a * v + b) >> k, 0, 255) when
  // that is exact for every v (contrast with a dyadic factor, brightness,
  // invert ...): the stencil kernels then map pixel pairs in packed i16
  // instead of LDS lookups
  bool post_aff = false;
  int post_a = 1, post_b = 0, post_k = 0;
  // Combine: the op (filters.h combine_rule)
  CombineKind comb = CombineKind::Add;
  int cq[3] = {0, 0, 0};
  int cd = 0;
  // bilateral stencil: the range sigma and its table (Op::sigma, Op::range)
  bool bilateral = false;
  double sigma = 0.0;
  std::array<uint8_t, 256> range{};
  // slot actions that precede the pass, in order: 'h' hold (the current image
  // also becomes the held image), 's' swap (current and held exchange roles)
  std::string slots;
  // branched plans: the pass writes the x-margins of its input (R pixels, its
  // border mode) before it reads them.  An image that more than one later op
  // may read (held, swapped back in) has no single consumer whose margins its
  // producer could maintain, so in a branched plan no producer maintains any
  // (out_margin_px = 0 throughout) and every stencil fills its own.
  bool fill_in = false;
  std::string desc;
  // the pass's LUT block is filled at run time from its input's histogram
  bool data_dependent() const { return pro.has_stat; }
  bool branches() const { return !slots.empty() || kind == PassKind::Combine; }
};

struct Plan {
  std::string spec;
  int cin = 3, cout = 3;
  int max_radius = 0;
  int max_channels = 3;
  int in_margin_px = 0;                      // margins the input must carry
  Border in_margin_border = Border::Reflect101;
  int held_c = 0;  // channels of an external held image the chain starts with (0: none)
  std::vector<Pass> passes;
  std::string describe() const;
  // some pass holds, swaps or combines: the engine keeps a third stripe buffer
  bool branched() const {
    for (const Pass& p : passes)
      if (p.branches()) return true;
    return false;
  }
  // some pass holds or swaps (an external held image then cannot be iterated)
  bool moves_slots() const {
    for (const Pass& p : passes)
      if (!p.slots.empty()) return true;
    return false;
  }
  // some pass carries a statistic op (a table built from its input at run time)
  bool data_dependent() const {
    for (const Pass& p : passes)
      if (p.data_dependent()) return true;
    return false;
  }
  // Every pass reads the current buffer and writes the other one of a ping-pong
  // pair, with constants fixed at plan time.  The engine's deep halo and deep
  // steps, its pipelined schedule, posted halos, graph replay and the chunked
  // e2e / dist / to-host steps all rely on this and decline a plan without it.
  // A new plan property that breaks the static two-buffer assumption belongs
  // in this predicate, not at those sites.
  bool static_chain() const { return !data_dependent() && !branched(); }
};

// default_border: border for every stencil without an explicit @mode suffix.
// held_c > 0: the chain starts with an external held image of that many channels.
Plan compile_chain(const std::vector<Op>& ops, int cin, Border default_border,
                   bool fuse = true, int held_c = 0);

// The pass with its statistic op resolved against `h`, the histogram of the
// pass's input over the WHOLE frame (p.cin channels): stat_lut's table composed
// in front of the static one, has_stat cleared.  A pass without one is returned
// as it is.
Pass resolve_stat(const Pass& p, const Histogram& h);

// Gray-conversion parameters in the form the kernels use.
// Find (a, b, k) with lut[v] == clamp((a * v + b) >> k, 0, 255) for every v
// in [0, 255], |a| * 255 + |b| < 2^15 (packed i16 arithmetic), smallest k.
bool lut_affine(const std::array<uint8_t, 256>& lut, int* a, int* b, int* k);

struct GrayParams {
  int mode = 0;           // 0 = bt601, 1 = ref (per-channel trunc magic)
  uint32_t mult[3] = {0, 0, 0};  // R, G, B
  int shift[3] = {0, 0, 0};
};
GrayParams gray_params(GrayMode m);

}  // namespace stripe
