// Compare-exchange networks of the median filters, shared by the host executor
// (cpu_exec.cpp: row-wide byte min/max sweeps) and the HIP kernels
// (rank_kernels.h: packed u16 min/max), so both run the same exact selection.
//
// A K x K median is computed in two stages:
//   1. ColSort<K>: every column of the window (K vertically adjacent pixels)
//      is sorted ascending.  Horizontally adjacent windows share K - 1 of
//      their K columns, so this runs once per extended row, not per output.
//   2. Select<K>: a selection network over the K sorted columns.  Wire
//      dx * K + r holds element r (ascending) of column dx; after the network
//      wire kOut holds element K*K/2 of the sorted window.
//
// Step modes: kBoth  (lo, hi) = (min, max) of wires (i, j), i < j;
//             kMin   wire i = min(i, j), wire j is dead afterwards;
//             kMax   wire j = max(i, j), wire i is dead afterwards.
//
// Select<3> is the classic form: the maximum of the columns' minima, the median
// of their medians, the minimum of their maxima, then the median of those three.
// Select<5> is Batcher's odd-even merge sort of 32 wires (window element w on
// wire w, wires 25..31 at +infinity) with every comparator removed that never
// exchanges on sorted columns, then every step removed (or halved to kMin /
// kMax) that the median wire does not depend on: 85 steps, 146 min/max
// operations.  tools/gen_rank_net.py prints the table; tests/test_rank_filters.py
// checks both networks on every 0-1 input with sorted columns, which by the
// 0-1 principle covers every input.
#pragma once

#include "stripe/stencil_defs.h"

namespace stripe {
namespace ranknet {

enum : int { kBoth = 0, kMin = 1, kMax = 2 };

struct Step {
  int i, j, mode;
};

template <int K>
struct ColSort;

template <>
struct ColSort<3> {
  static constexpr int N = 3;
  STRIPE_HD static constexpr Step at(int k) {
    constexpr Step t[N] = {{0, 1, kBoth}, {1, 2, kBoth}, {0, 1, kBoth}};
    return t[k];
  }
};

template <>
struct ColSort<5> {
  static constexpr int N = 9;  // the optimal 5-sorter
  STRIPE_HD static constexpr Step at(int k) {
    constexpr Step t[N] = {{0, 1, kBoth}, {3, 4, kBoth}, {2, 4, kBoth}, {2, 3, kBoth}, {1, 4, kBoth},
                           {0, 3, kBoth}, {0, 2, kBoth}, {1, 3, kBoth}, {1, 2, kBoth}};
    return t[k];
  }
};

template <int K>
struct Select;

template <>
struct Select<3> {
  static constexpr int N = 10, kOut = 4;
  STRIPE_HD static constexpr Step at(int k) {
    constexpr Step t[N] = {
        {0, 3, kMax}, {3, 6, kMax},                 // wire 6: max of the minima
        {5, 8, kMin}, {2, 5, kMin},                 // wire 2: min of the maxima
        {1, 4, kBoth}, {4, 7, kMin}, {1, 4, kMax},  // wire 4: median of the medians
        {4, 6, kBoth}, {2, 6, kMin}, {2, 4, kMax},  // wire 4: median of wires 6, 4, 2
    };
    return t[k];
  }
};

template <>
struct Select<5> {
  static constexpr int N = 85, kOut = 12;
  STRIPE_HD static constexpr Step at(int k) {
    constexpr Step t[N] = {
        {4, 5, 0},   {5, 7, 0},   {5, 6, 0},   {0, 4, 0},   {2, 6, 0},   {2, 4, 0},   {1, 5, 0},   {3, 5, 0},
        {1, 2, 0},   {3, 4, 0},   {5, 6, 0},   {8, 10, 0},  {9, 11, 0},  {9, 10, 0},  {14, 15, 0}, {12, 14, 0},
        {13, 14, 0}, {8, 12, 0},  {10, 14, 0}, {10, 12, 0}, {11, 15, 0}, {11, 13, 0}, {9, 10, 0},  {11, 12, 0},
        {13, 14, 0}, {0, 8, 0},   {4, 12, 0},  {4, 8, 0},   {2, 10, 0},  {6, 14, 0},  {6, 10, 0},  {2, 4, 0},
        {6, 8, 0},   {10, 12, 0}, {1, 9, 0},   {5, 13, 0},  {5, 9, 0},   {3, 11, 0},  {7, 15, 1},  {7, 11, 0},
        {3, 5, 0},   {7, 9, 0},   {11, 13, 0}, {1, 2, 0},   {3, 4, 0},   {5, 6, 0},   {7, 8, 0},   {9, 10, 0},
        {11, 12, 0}, {13, 14, 1}, {16, 20, 0}, {18, 22, 0}, {18, 20, 0}, {17, 21, 0}, {19, 23, 0}, {19, 21, 0},
        {17, 18, 0}, {19, 20, 0}, {21, 22, 0}, {20, 24, 0}, {22, 24, 0}, {21, 22, 0}, {23, 24, 0}, {0, 16, 2},
        {8, 24, 1},  {8, 16, 2},  {4, 20, 2},  {12, 20, 1}, {12, 16, 1}, {2, 18, 2},  {10, 18, 1}, {6, 22, 1},
        {6, 10, 2},  {10, 12, 2}, {1, 17, 2},  {9, 17, 2},  {5, 21, 2},  {13, 21, 1}, {13, 17, 1}, {3, 19, 2},
        {11, 19, 1}, {7, 23, 1},  {7, 11, 2},  {11, 13, 1}, {11, 12, 2},
    };
    return t[k];
  }
};

}  // namespace ranknet
}  // namespace stripe
