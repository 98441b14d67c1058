#!/usr/bin/env python3
"""Print the selection network of the KxK median (csrc/include/stripe/rank_net.h).

The median kernels first sort every column of the window, so the network only
has to select element K*K/2 from K sorted columns.  Construction:

  1. Batcher's odd-even merge sort on the next power of two of wires; window
     element w (= column * K + rank in its column) sits on wire w, the unused
     wires hold +infinity (comparators against them never exchange).
  2. Simulate the network on every 0-1 input with sorted columns (column c
     holds k_c ones at its top ranks: (K + 1)^K inputs, all at once as one big
     integer per wire) and drop every comparator that never exchanges.  By the
     0-1 principle the remaining network still sorts every such input.
  3. Walk backwards from the median wire and drop every step it does not
     depend on; a step with one dead output keeps only its min or max.

Usage: python tools/gen_rank_net.py [K]     (default 5)
Output: the steps as {i, j, mode} rows, mode 0 both, 1 min -> i, 2 max -> j.
"""
from __future__ import annotations

import itertools
import sys


def batcher(n: int) -> list[tuple[int, int]]:
    ces: list[tuple[int, int]] = []

    def merge(lo: int, cnt: int, r: int) -> None:
        step = r * 2
        if step < cnt:
            merge(lo, cnt, step)
            merge(lo + r, cnt, step)
            for i in range(lo + r, lo + cnt - r, step):
                ces.append((i, i + r))
        else:
            ces.append((lo, lo + r))

    def sort(lo: int, cnt: int) -> None:
        if cnt > 1:
            sort(lo, cnt // 2)
            sort(lo + cnt // 2, cnt // 2)
            merge(lo, cnt, 1)

    sort(0, n)
    return ces


def select_network(K: int) -> tuple[list[tuple[int, int, int]], int]:
    N, med = K * K, K * K // 2
    wires = 1
    while wires < N:
        wires *= 2
    inputs = list(itertools.product(range(K + 1), repeat=K))  # ones per column
    full = (1 << len(inputs)) - 1
    state = [full] * wires
    for c in range(K):
        for r in range(K):
            state[c * K + r] = sum(1 << t for t, ks in enumerate(inputs) if r >= K - ks[c])
    kept = []
    for i, j in batcher(wires):
        a, b = state[i], state[j]
        if a & ~b & full:  # some input exchanges here
            kept.append((i, j))
            state[i], state[j] = a & b, a | b
    for t, ks in enumerate(inputs):  # wire `med` holds element `med` of the sorted window
        assert (state[med] >> t) & 1 == (sum(ks) >= N - med)
    live, out = {med}, []
    for i, j in reversed(kept):
        if i in live or j in live:
            out.append((i, j, 0 if i in live and j in live else 1 if i in live else 2))
            live |= {i, j}
    out.reverse()
    assert all(j < N for _, j, _ in out)
    return out, med


def main() -> None:
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    net, out = select_network(K)
    ops = sum(2 if m == 0 else 1 for _, _, m in net)
    print(f"// Select<{K}>: N = {len(net)}, kOut = {out}, {ops} min/max operations")
    for k in range(0, len(net), 8):
        print("        " + " ".join(f"{{{i}, {j}, {m}}}," for i, j, m in net[k:k + 8]))


if __name__ == "__main__":
    main()
