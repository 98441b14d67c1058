// Launch policy of the HIP kernels: every decision about *how* a pass is
// launched (store policy, workgroup order, occupancy cap, the environment
// knobs behind them), as pure host functions.  Plain C++, no HIP calls: the
// launchers (stencil.hip, pointwise.hip, blur_sep.hip, conv.hip, dispatch.cpp)
// ask here, and `_C.launch_policy` exposes the same functions to the tests.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace stripe {
namespace dev {

// A pass counts as streaming from HBM above this size (policy::stream_policy).
constexpr int64_t kNtMinBytes = 224ll << 20;
// resident workgroups per CU of nt-store (HBM-streaming) stencil launches
constexpr int kNtWgsSep = 2;     // separable (k_sep)
constexpr int kNtWgsDirect = 3;  // direct (k_direct) without a gray prologue
constexpr int kXcdCount = 8;  // MI355X: 8 XCDs of 32 CUs, one L2 each

}  // namespace dev

namespace policy {

// ------------------------------------------------------------------------------
// Environment knobs read under csrc/hip
// ------------------------------------------------------------------------------
inline int env_int(const char* name, int fallback) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : fallback;
}
// Cached knobs are read once per process.
#define STRIPE_CACHED_KNOB(fn, type, ...) \
  inline type fn() {                      \
    static const type v = (__VA_ARGS__);  \
    return v;                             \
  }

// STRIPE_NT=0|1: A/B switch of the store policy.  Live: read at every launch
// (tests and tools change it inside one process), once per launch.
// -1: unset, else 0 / 1.
inline int env_nt() {
  const char* e = std::getenv("STRIPE_NT");
  return e ? (std::atoi(e) != 0 ? 1 : 0) : -1;
}

// XCD-aware workgroup remap (xcd_remap): the caller sets a.nxcd (launch_stencil:
// on for passes whose working set stays in the Infinity Cache, where halo rows
// shared by vertically adjacent bands become L2 hits); STRIPE_XCD=<n> forces it
// (0 = off) for A/B runs.
STRIPE_CACHED_KNOB(env_nxcd, int, env_int("STRIPE_XCD", -1))

// Occupancy cap of the HBM-streaming (nt-store) stencil launches: fewer
// resident waves per SIMD keep fewer concurrent row streams open against HBM
// (16384^2 RGB, band autotune on, profiles/r2d/nt_wgs_ab.txt: separable
// gaussian5 0.311 -> 0.282 ms at 2 workgroups per CU, gaussian3 0.299 -> 0.269,
// sobel 0.315 -> 0.293; direct emboss3 0.300 -> 0.283 at 3; the gray-prologue
// direct kernels read 3 bytes per output byte and gain nothing).  The cap is an
// LDS reservation (dynamic shared memory the kernel never touches) sized so
// only `target` workgroups fit a CU's LDS; STRIPE_NT_WGS overrides the cap of
// HBM-streaming launches (stencil_cap; 0 = no cap).
struct NtWgsKnob {
  bool set;  // the autotuner leaves the caps alone then: A/B runs pin the cap
  int wgs;
};
STRIPE_CACHED_KNOB(nt_wgs_knob, NtWgsKnob,
                   NtWgsKnob{std::getenv("STRIPE_NT_WGS") != nullptr, env_int("STRIPE_NT_WGS", -1)})
inline int env_nt_wgs() { return nt_wgs_knob().wgs; }

// streaming flat passes: at most 3 resident workgroups per CU (an LDS
// reservation the kernel never touches; fewer concurrent streams against
// HBM: 16K RGB invert 0.287 -> 0.269 ms, brightness 0.290 -> 0.268,
// profiles/r2d/pw_wgs_ab.txt); STRIPE_PW_WGS overrides (0 = no cap)
// Colour matrix, HBM-streaming launches: the residency cap of the flat passes
// (STRIPE_PW_WGS; 0 = no cap).  Default 3 workgroups per CU for the bare
// matrix (16K RGB sepia 0.277 ms uncapped, 0.305 at 2, 0.269 at 3, 0.268
// at 4) and 6 with a LUT stage, whose LDS lookups need more waves in
// flight (invert,sepia,brightness:10: 0.411 at 2, 0.313 at 3, 0.292 at 4,
// 0.268 at 6, 0.271 uncapped; profiles/colormatrix/README.md)
// kKnobUnset: unset (the family's default).
constexpr int kKnobUnset = INT32_MIN;
STRIPE_CACHED_KNOB(env_pw_wgs, int, env_int("STRIPE_PW_WGS", kKnobUnset))
constexpr int kPwWgsFlat = 3, kPwWgsMix = 3, kPwWgsMixLut = 6;
// Combine passes (k_combine), HBM-streaming launches: the flat passes' knob,
// a cap of 2 workgroups per CU.  A workgroup keeps two input streams and one
// output stream open, so fewer of them fill HBM's queues (16K RGB unsharp, six
// interleaved rounds: 0.747-0.753 ms at 1, 0.655-0.668 at 2, 0.675-0.710 at 3,
// 0.687-0.697 at 4, 0.699-0.717 uncapped; profiles/combine/README.md)
constexpr int kPwWgsCombine = 2;

// A/B knob, off: capping the resident workgroups of channel-changing passes
// (STRIPE_PWG_WGS, LDS reservation) only slows them - 16K gray:ref 0.187 ms
// uncapped, 0.212 at 4 per CU, 0.284 at 2 (profiles/r2d/pw_wgs_ab.txt)
STRIPE_CACHED_KNOB(env_pwg_wgs, int, env_int("STRIPE_PWG_WGS", 0))

// gray L1 sobel on row pairs (STRIPE_SOBEL_RP=0: the k_sep form, A/B)
STRIPE_CACHED_KNOB(sobel_rp, bool, env_int("STRIPE_SOBEL_RP", 1) != 0)
// 8-row bands request all ten input rows up front (the autotuner's
// band-8 candidate; full 8192^2 frame 2-3.5 % faster than the best
// streamed band, profiles/r5/cfg3/README.md); STRIPE_SOBEL_PB=8|12
// forces bands of that height with up-front loads (A/B)
STRIPE_CACHED_KNOB(sobel_pb, int, [] {
  const int v = env_int("STRIPE_SOBEL_PB", -1);
  return v == 0 || v == 8 || v == 12 ? v : -1;
}())
// 1 KiB tiles with edge loads (STRIPE_SOBEL_WIDE=0: 62-lane tiles, A/B)
STRIPE_CACHED_KNOB(sobel_wide, bool, env_int("STRIPE_SOBEL_WIDE", 1) != 0)

// A/B variants of the RGB non-edge MFMA blur kernel (STRIPE_BLUR_VARIANT=n,
// described beside the variant table in launch_blur_sep)
STRIPE_CACHED_KNOB(blur_variant, int, env_int("STRIPE_BLUR_VARIANT", 0))

// STRIPE_CONV_F16=1: the f16 hi+lo kernel (k_conv_mfma) instead of the i8
// weight-digit kernel (A/B runs)
STRIPE_CACHED_KNOB(conv_f16, bool, env_int("STRIPE_CONV_F16", 0) != 0)
// STRIPE_CONV_SPLIT=1: two-part epilogue at every K (A/B)
STRIPE_CACHED_KNOB(conv_split, int, env_int("STRIPE_CONV_SPLIT", 0) == 1 ? 1 : 0)
// m-tiles per wave (STRIPE_CONV_MT overrides for A/B runs)
STRIPE_CACHED_KNOB(conv_mt, int, env_int("STRIPE_CONV_MT", 0))
// output tiles per workgroup: 1, or 4 with STRIPE_CONV_NT=4 (the next
// tile's staging under the current tile's MFMAs, k_conv_i8 NT).  Measured
// on 16K RGB conv:31 (profiles/r5/conv/): 4 tiles at 2 m-tiles 2.32-2.36 ms
// exact / 1.85 ms lsb against 2.09-2.10 / 1.54-1.55 ms for one tile at 3
// m-tiles (4 tiles at 3 m-tiles spill): one tile stays the default
STRIPE_CACHED_KNOB(conv_nt, int, env_int("STRIPE_CONV_NT", 0))
// single-buffered A fragments (k_conv_i8 A1) wherever an instance exists;
// STRIPE_CONV_A1=0 for A/B runs against the double-buffered kernels
STRIPE_CACHED_KNOB(conv_a1, bool, env_int("STRIPE_CONV_A1", 1) != 0)

// Byte range of one buffer-descriptor view: the stencil / conv kernels address
// rows with 32-bit offsets and bias masked lanes by 2^31 (dev::kOOB), so a view
// must stay below 2 GiB (minus slack for the bias arithmetic).
// STRIPE_DESC_LIMIT (bytes) lowers it so tests can exercise the chunked path.
STRIPE_CACHED_KNOB(desc_limit, int64_t, [] {
  const char* e = std::getenv("STRIPE_DESC_LIMIT");
  const int64_t def = (1ll << 31) - (1ll << 20);
  return e ? std::max<int64_t>(1 << 16, std::min<int64_t>(def, std::atoll(e))) : def;
}())

// STRIPE_JPEG_PIN=0 keeps the pageable coefficient upload (A/B switch)
STRIPE_CACHED_KNOB(jpeg_pin, bool, env_int("STRIPE_JPEG_PIN", 1) != 0)

#undef STRIPE_CACHED_KNOB

// ------------------------------------------------------------------------------
// Output row ranges of a launch
// ------------------------------------------------------------------------------
// PassLaunch::ry / nrange as the kernels take them: [ry0, ry1) of n0 rows and
// [ry2, ry3) of n1 rows (an empty or absent second range is 0, 0).
struct RowRanges {
  int n0, n1, ry0, ry1, ry2, ry3;
  int rows() const { return n0 + n1; }
};
inline RowRanges row_ranges(const int (&ry)[4], int nrange) {
  RowRanges r;
  r.n0 = std::max(0, ry[1] - ry[0]);
  r.n1 = nrange > 1 ? std::max(0, ry[3] - ry[2]) : 0;
  r.ry0 = ry[0];
  r.ry1 = ry[0] + r.n0;
  r.ry2 = r.n1 ? ry[2] : 0;
  r.ry3 = r.n1 ? ry[3] : 0;
  return r;
}

// ------------------------------------------------------------------------------
// The streaming decision
// ------------------------------------------------------------------------------
enum class Family {
  Sep,            // k_sep
  SobelRp,        // k_sobel_rp
  Direct,         // k_direct
  Rank,           // k_rank
  Bilateral,      // k_bilateral
  ConvSmall,      // k_conv_small
  PointwiseChan,  // k_pointwise (channel-changing)
  PointwiseFlat,  // k_pointwise_flat
  ColorMix,       // k_colormix
  Blur,           // k_blur_pl
  Combine,        // k_combine
  Resize,         // k_resize
  Orient,         // k_orient
  Warp,           // k_warp
  Remap,          // k_remap
};

struct PolicyIn {
  Family family;
  int cin = 3, cout = 3, cmid = 3;  // channels of the pass (Pass::cin / cout / cmid)
  int W = 0, rows = 0;              // pixels per row, output rows of the launch (n0 + n1)
  int nt = -1;                      // PassLaunch::nt
  int wgs = -1;                     // PassLaunch::wgs
  bool gray_prologue = false;       // stencil with a gray prologue (3 input bytes per output byte)
  bool lut_stage = false;           // colour matrix with a pre or post LUT stage
  int W2 = 0, rows2 = 0;            // resize, warp, remap: pixels per row and rows of the destination (W, rows: the source)
  int64_t mesh_bytes = 0;           // remap: bytes of the mesh
};

struct StreamPolicy {
  bool nt_stores = false;    // the nt-store kernel instance
  bool streaming = false;    // the pass counts as streaming from HBM
  int nxcd = 0;              // KArgs::nxcd (XCD-aware workgroup remap; 0 = linear order)
  int cap = 0;               // resident workgroups per CU the family would cap at (0 = none)
  bool cap_applied = false;  // this launch reserves LDS for `cap`
};

// Occupancy cap of one launch: wgs >= 0 is the engine's choice (its autotuner
// times the caps per pass and box, since the best cap depends on the clock
// and memory behaviour of the box: round-2 driver run);
// wgs < 0 takes the family default, applied to HBM-streaming launches only.
inline int stencil_cap(bool nt, int wgs, int family_default) {
  if (nt && env_nt_wgs() >= 0) return env_nt_wgs();  // A/B runs pin the streaming cap only
  if (wgs >= 0) return wgs;
  return nt ? family_default : 0;
}
// Family default of stencil_cap (the gray-prologue direct / rank kernels gain nothing;
// the bilateral family starts from the rank family's values).
constexpr int stencil_cap_default(Family f, bool gray_prologue) {
  return f == Family::Sep || f == Family::SobelRp ? dev::kNtWgsSep : gray_prologue ? 0 : dev::kNtWgsDirect;
}

// One decision per launch, per family.  The families differ in the bytes they
// compare with kNtMinBytes, in whether PassLaunch::nt and STRIPE_NT count, and
// in when the cap applies; each difference is an explicit case below.
//
// Asymmetries kept as they were measured or grew; candidates for a later
// change with measurements, not fixed here:
//   * flat pointwise: STRIPE_NT can only turn nt stores off (=0), never on;
//   * channel-changing pointwise: STRIPE_NT=1 forces nt stores onto 3-channel
//     output, which the size rule excludes as slow (partial lines);
//   * all pointwise families and k_conv_small ignore PassLaunch::nt;
//   * channel-changing pointwise applies its cap by size, whatever nt is;
//   * the MFMA blur does not read STRIPE_NT;
//   * resize, orient, warp and remap have no occupancy cap and ignore PassLaunch::nt / wgs.
inline StreamPolicy stream_policy(const PolicyIn& in) {
  StreamPolicy r;
  const int64_t px = (int64_t)in.rows * in.W;
  switch (in.family) {
    case Family::Sep:
    case Family::SobelRp:
    case Family::Direct:
    case Family::Rank:
    case Family::Bilateral: {
      // Output stores bypass the caches (nt) when the pass streams more than the
      // Infinity Cache holds: then the next pass cannot hit in it anyway (16K RGB
      // frame: gaussian5 0.322 -> 0.319 ms, reference chain 0.239 -> 0.227 ms).  A
      // smaller working set (the 16K x 2K stripe of an 8-GPU run, 8K^2 gray) keeps
      // the default policy so the next iteration reads its input from the cache
      // (8K^2 gray gaussian5: 0.030 ms default vs 0.034 ms nt).
      // The size rule is only the default: the engine passes the policy it tuned
      // (L.nt), and a cache-cold stripe (EngineConfig::cold: a stream of frames, or
      // a working set evicted between steps) streams from HBM however small its
      // pass is -- the data's temperature, not the pass size, is what matters.
      bool nt = in.nt >= 0 ? in.nt != 0 : px * (in.cin + in.cout) > dev::kNtMinBytes;
      if (const int e = env_nt(); e >= 0) nt = e != 0;  // A/B switch
      r.nt_stores = r.streaming = nt;
      // A pass that stays in the Infinity Cache is bound by L2 / fabric traffic: the
      // XCD-contiguous workgroup remap turns the halo rows that vertically adjacent
      // bands share into L2 hits (one N=8 stripe of the 16K RGB frame, gaussian5:
      // 0.0394-0.0401 -> 0.0372 ms at 8-row bands, profiles/r2/xcd_remap_stripe.txt).
      // A pass streaming from HBM gains nothing from it (round 1: FETCH_SIZE 1.40x ->
      // 1.15x of ideal, time unchanged, profiles/fetch_xcd_bands_16k_r1.txt).
      r.nxcd = nt ? 0 : dev::kXcdCount;
      if (env_nxcd() >= 0) r.nxcd = env_nxcd();
      r.cap = stencil_cap(nt, in.wgs, stencil_cap_default(in.family, in.gray_prologue));
      r.cap_applied = r.cap > 0;
      break;
    }
    case Family::ConvSmall: {
      // size rule on the stencil's own channels; PassLaunch::nt is not consulted
      bool nt = px * 2 * in.cmid > dev::kNtMinBytes;
      if (const int e = env_nt(); e >= 0) nt = e != 0;
      r.nt_stores = r.streaming = nt;
      r.nxcd = env_nxcd() >= 0 ? env_nxcd() : 0;  // linear order unless forced
      break;
    }
    case Family::PointwiseChan: {
      // nt stores when the pass streams more than the Infinity Cache (as the
      // stencil kernels; a smaller set is read back from the cache by the next
      // pass) and only for 1-channel output, where one store instruction covers
      // 1 KiB contiguously: the 3-channel store pattern (16 B per lane at a 48 B
      // stride) writes partial lines that nt sends to HBM unmerged (16K RGB
      // invert 0.295 -> 0.322 ms with nt; 16K gray:ref 0.192 -> 0.184 ms)
      r.streaming = px * (in.cin + in.cout) > dev::kNtMinBytes;
      r.nt_stores = in.cout == 1 && r.streaming;
      if (const int e = env_nt(); e >= 0) r.nt_stores = e != 0;  // also for 3-channel output
      r.cap = env_pwg_wgs();
      r.cap_applied = r.cap > 0 && r.streaming;  // by size: not tied to the store policy
      break;
    }
    case Family::PointwiseFlat: {
      r.streaming = px * 2 * in.cin > dev::kNtMinBytes;
      r.nt_stores = r.streaming && env_nt() != 0;  // STRIPE_NT=0 turns nt off; =1 cannot turn it on
      r.cap = env_pw_wgs() != kKnobUnset ? env_pw_wgs() : kPwWgsFlat;
      r.cap_applied = r.cap > 0 && r.nt_stores;
      break;
    }
    case Family::ColorMix: {
      r.streaming = px * 6 > dev::kNtMinBytes;
      r.nt_stores = r.streaming;
      if (const int e = env_nt(); e >= 0) r.nt_stores = e != 0;
      r.cap = env_pw_wgs() >= 0 ? env_pw_wgs() : (in.lut_stage ? kPwWgsMixLut : kPwWgsMix);
      r.cap_applied = r.cap > 0 && r.streaming && r.nt_stores;  // both: the size and the store policy
      break;
    }
    case Family::Combine: {
      // two inputs and one output of cin channels each: 3 bytes move per output byte
      r.streaming = px * 3 * in.cin > dev::kNtMinBytes;
      r.nt_stores = r.streaming;
      if (const int e = env_nt(); e >= 0) r.nt_stores = e != 0;  // overrides either way
      r.cap = env_pw_wgs() != kKnobUnset ? env_pw_wgs() : kPwWgsCombine;
      r.cap_applied = r.cap > 0 && r.streaming && r.nt_stores;
      break;
    }
    case Family::Resize: {
      // one read of the source frame and one write of the destination, cin channels each
      r.streaming = (px + (int64_t)in.rows2 * in.W2) * in.cin > dev::kNtMinBytes;
      r.nt_stores = r.streaming;
      if (const int e = env_nt(); e >= 0) r.nt_stores = e != 0;  // overrides either way
      break;
    }
    case Family::Orient: {
      // one read of the source window (W x rows) and one write of as many pixels, cin channels each
      r.streaming = px * 2 * in.cin > dev::kNtMinBytes;
      r.nt_stores = r.streaming;
      if (const int e = env_nt(); e >= 0) r.nt_stores = e != 0;  // overrides either way
      break;
    }
    case Family::Warp: {
      // the orient family's rule on the pixels of both frames: at most one read of the source
      // (W x rows) and one write of the destination (W2 x rows2), cin channels each
      r.streaming = (px + (int64_t)in.rows2 * in.W2) * in.cin > dev::kNtMinBytes;
      r.nt_stores = r.streaming;
      if (const int e = env_nt(); e >= 0) r.nt_stores = e != 0;  // overrides either way
      break;
    }
    case Family::Remap: {
      // the warp family's rule with the mesh bytes (read once) added to source + destination
      r.streaming = (px + (int64_t)in.rows2 * in.W2) * in.cin + in.mesh_bytes > dev::kNtMinBytes;
      r.nt_stores = r.streaming;
      if (const int e = env_nt(); e >= 0) r.nt_stores = e != 0;  // overrides either way
      break;
    }
    case Family::Blur: {
      // (the engine's memory policy decides for a cache-cold stripe: L.nt = 1)
      // STRIPE_NT is not read; the kernels have no nt-store instances:
      // `streaming` picks the workgroup order and the lsb staging instance
      r.streaming = in.nt >= 0 ? in.nt != 0 : px * 2 * in.cmid > dev::kNtMinBytes;
      r.nxcd = env_nxcd() >= 0 ? env_nxcd() : (r.streaming ? 0 : dev::kXcdCount);
      break;
    }
  }
  return r;
}

// ------------------------------------------------------------------------------
// The LDS reservation behind an occupancy cap
// ------------------------------------------------------------------------------
// Dynamic shared memory that lets `target` workgroups of a kernel with
// `static_lds` bytes of its own fit a CU's LDS, and target + 1 not.
inline int64_t lds_reserve_bytes(int64_t lds_per_cu, int64_t static_lds, int target) {
  if (target <= 0) return 0;
  return std::max<int64_t>(0, lds_per_cu / (target + 1) + 1024 - static_lds);
}

}  // namespace policy
}  // namespace stripe
