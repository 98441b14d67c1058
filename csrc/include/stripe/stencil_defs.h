// Compile-time coefficient sets for the integer stencils.  Usable from host code
// (golden path / catalogue) and device code (kernels instantiate one template per
// filter so every tap is a literal and zero taps vanish; the reference instead
// keeps runtime-indexed private int[5][5] arrays per thread, kernel.cu:71-82,
// which spill to scratch on CDNA).
//
// Weights are correlation weights indexed [dy][dx] (dy = row offset + R).  The
// reference indexes filter[fx][fy] (kernel.cu:86-88) - transposed - but both of
// its filters are symmetric so the result is identical.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define STRIPE_HD __host__ __device__
#else
#define STRIPE_HD
#endif

namespace stripe {
namespace sdef {

struct Emboss3 {
  static constexpr bool BINOM = false;
  static constexpr int K = 3, R = 1, DIV = 1;
  static constexpr bool SEP = false, SOBEL = false;
  static constexpr int RANK = 0, BILATERAL = 0;
  STRIPE_HD static constexpr int w(int dy, int dx) {
    constexpr int t[9] = {-2, -1, 0, -1, 1, 1, 0, 1, 2};  // kernel.cu:71-75
    return t[dy * 3 + dx];
  }
};

struct Emboss5 {
  static constexpr bool BINOM = false;
  static constexpr int K = 5, R = 2, DIV = 1;
  static constexpr bool SEP = false, SOBEL = false;
  static constexpr int RANK = 0, BILATERAL = 0;
  STRIPE_HD static constexpr int w(int dy, int dx) {
    constexpr int d[5] = {4, 4, 1, -4, -4};  // kernel.cu:76-82 (diagonal)
    return dy == dx ? d[dy] : 0;
  }
};

struct Sharpen {
  static constexpr bool BINOM = false;
  static constexpr int K = 3, R = 1, DIV = 1;
  static constexpr bool SEP = false, SOBEL = false;
  static constexpr int RANK = 0, BILATERAL = 0;
  STRIPE_HD static constexpr int w(int dy, int dx) {
    constexpr int t[9] = {0, -1, 0, -1, 5, -1, 0, -1, 0};
    return t[dy * 3 + dx];
  }
};

struct Laplace {
  static constexpr bool BINOM = false;
  static constexpr int K = 3, R = 1, DIV = 1;
  static constexpr bool SEP = false, SOBEL = false;
  static constexpr int RANK = 0, BILATERAL = 0;
  STRIPE_HD static constexpr int w(int dy, int dx) {
    constexpr int t[9] = {0, 1, 0, 1, -4, 1, 0, 1, 0};
    return t[dy * 3 + dx];
  }
};

// Sobel: Gx = [1,2,1]^T (x) [-1,0,1],  Gy = [-1,0,1]^T (x) [1,2,1];  out = sat(|Gx|+|Gy|)
// Both kernels are rank one: the GPU runs it as a separable pair (vertical
// smoothing + difference rows, then horizontal difference + smoothing).
struct Sobel {
  static constexpr bool BINOM = false;
  static constexpr int K = 3, R = 1, DIV = 1;
  static constexpr bool SEP = true, SOBEL = true;
  static constexpr int RANK = 0, BILATERAL = 0;
  STRIPE_HD static constexpr int g(int i) { return i == 1 ? 2 : 1; }
  STRIPE_HD static constexpr int wx(int dy, int dx) {
    constexpr int s[3] = {1, 2, 1}, d[3] = {-1, 0, 1};
    return s[dy] * d[dx];
  }
  STRIPE_HD static constexpr int wy(int dy, int dx) {
    constexpr int s[3] = {1, 2, 1}, d[3] = {-1, 0, 1};
    return d[dy] * s[dx];
  }
  STRIPE_HD static constexpr int w(int dy, int dx) { return wx(dy, dx); }
  static constexpr bool L2 = false;
};

// Sobel gradient magnitude: out = sat(round(sqrt(Gx^2 + Gy^2))), the L2 form of
// SURVEY §2.7's "sobel (|Gx|+|Gy| or L2)".  sqrt of an integer is never a
// half-integer, so the rounding is exact: round = k + (n > k^2 + k), k = isqrt(n).
struct SobelL2 : Sobel {
  static constexpr bool L2 = true;
};

// Separable integer smoothing filters: out = (sum + DIV/2) / DIV, sum >= 0.
struct Gaussian3 {  // binomial: cascade of K-1 two-tap sums
  static constexpr bool BINOM = true;
  static constexpr int K = 3, R = 1, DIV = 16;
  static constexpr bool SEP = true, SOBEL = false;
  static constexpr int RANK = 0, BILATERAL = 0;
  STRIPE_HD static constexpr int g(int i) {
    constexpr int t[3] = {1, 2, 1};
    return t[i];
  }
  STRIPE_HD static constexpr int w(int dy, int dx) { return g(dy) * g(dx); }
};

struct Gaussian5 {  // binomial: cascade of K-1 two-tap sums
  static constexpr bool BINOM = true;
  static constexpr int K = 5, R = 2, DIV = 256;
  static constexpr bool SEP = true, SOBEL = false;
  static constexpr int RANK = 0, BILATERAL = 0;
  STRIPE_HD static constexpr int g(int i) {
    constexpr int t[5] = {1, 4, 6, 4, 1};
    return t[i];
  }
  STRIPE_HD static constexpr int w(int dy, int dx) { return g(dy) * g(dx); }
};

struct Gaussian7 {  // binomial: cascade of K-1 two-tap sums
  static constexpr bool BINOM = true;
  static constexpr int K = 7, R = 3, DIV = 4096;
  static constexpr bool SEP = true, SOBEL = false;
  static constexpr int RANK = 0, BILATERAL = 0;
  STRIPE_HD static constexpr int g(int i) {
    constexpr int t[7] = {1, 6, 15, 20, 15, 6, 1};
    return t[i];
  }
  STRIPE_HD static constexpr int w(int dy, int dx) { return g(dy) * g(dx); }
};

struct Box3 {
  static constexpr bool BINOM = false;
  static constexpr int K = 3, R = 1, DIV = 9;
  static constexpr bool SEP = true, SOBEL = false;
  static constexpr int RANK = 0, BILATERAL = 0;
  STRIPE_HD static constexpr int g(int) { return 1; }
  STRIPE_HD static constexpr int w(int, int) { return 1; }
};

struct Box5 {
  static constexpr bool BINOM = false;
  static constexpr int K = 5, R = 2, DIV = 25;
  static constexpr bool SEP = true, SOBEL = false;
  static constexpr int RANK = 0, BILATERAL = 0;
  STRIPE_HD static constexpr int g(int) { return 1; }
  STRIPE_HD static constexpr int w(int, int) { return 1; }
};

// Rank filters (erode = window minimum, dilate = maximum, median = element
// K*K/2 of the sorted window): no weights, a compile-time rank tag instead.
// The tags mirror stripe::Rank (filters.h).  Every definition carries RANK and
// BILATERAL (0: a weighted stencil); they select the kernel family.
constexpr int kRankMin = 1, kRankMax = 2, kRankMedian = 3;

template <int K_, int RANK_>
struct RankDef {
  static constexpr bool BINOM = false;
  static constexpr int K = K_, R = K_ / 2, DIV = 1;
  static constexpr bool SEP = false, SOBEL = false;
  static constexpr int RANK = RANK_, BILATERAL = 0;
};
struct Median3 : RankDef<3, kRankMedian> {};
struct Median5 : RankDef<5, kRankMedian> {};
struct Erode3 : RankDef<3, kRankMin> {};
struct Erode5 : RankDef<5, kRankMin> {};
struct Dilate3 : RankDef<3, kRankMax> {};
struct Dilate5 : RankDef<5, kRankMax> {};

// Bilateral filters (filters.h): the spatial weights are g (x) g with the
// binomial taps of gaussianK; the range table is run-time data of the pass.  A
// compile-time tag selects the kernel family, as RANK does.
template <class G>
struct BilateralDef {
  static constexpr bool BINOM = false;
  static constexpr int K = G::K, R = G::R, DIV = 1;
  static constexpr bool SEP = false, SOBEL = false;
  static constexpr int RANK = 0, BILATERAL = 1;
  STRIPE_HD static constexpr int g(int i) { return G::g(i); }
  STRIPE_HD static constexpr int w(int dy, int dx) { return G::g(dy) * G::g(dx); }
};
struct Bilateral3 : BilateralDef<Gaussian3> {};
struct Bilateral5 : BilateralDef<Gaussian5> {};

}  // namespace sdef
}  // namespace stripe

// The one list of integer stencils: X(Id, "canonical name", aliases...), Id a
// definition in sdef above.  The order is the StencilId order (filters.h), so
// append.  From it come the enum, the info table and the name lookup
// (filters.cpp), and the launcher's switch and extern templates (stencil.hip);
// a new filter also needs its instantiation line in one stencil_inst_*.hip.
#define STRIPE_STENCILS(X)                        \
  X(Emboss3, "emboss3", "emboss")                 \
  X(Emboss5, "emboss5")                           \
  X(Gaussian3, "gaussian3")                       \
  X(Gaussian5, "gaussian5", "gaussian", "gauss5") \
  X(Gaussian7, "gaussian7")                       \
  X(Box3, "box3")                                 \
  X(Box5, "box5")                                 \
  X(Sharpen, "sharpen")                           \
  X(Laplace, "laplace", "laplacian")              \
  X(Sobel, "sobel", "edge")                       \
  X(SobelL2, "sobel_l2", "magnitude")             \
  X(Median3, "median3", "median")                 \
  X(Median5, "median5")                           \
  X(Erode3, "erode3", "erode")                    \
  X(Erode5, "erode5")                             \
  X(Dilate3, "dilate3", "dilate")                 \
  X(Dilate5, "dilate5")                           \
  X(Bilateral3, "bilateral3")                     \
  X(Bilateral5, "bilateral5", "bilateral")
