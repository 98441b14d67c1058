#!/usr/bin/env python3
"""Integral-image benchmark: `_C.integral_device` and `_C.window_device` (box at
K = 5, 31 and 255, std, mean and sauvola at K = 31) on cache-cold gray frames,
beside a linear copy of the same source + table + destination bytes, the
chain's `box5` and `threshold:adaptive:5` on the same frames and, for the
4096^2 frame, `scipy.ndimage.uniform_filter` on the host.

Every case rotates over enough (source, destination) buffer pairs that a call's
buffers were last touched pairs-1 calls earlier: pairs * bytes per call >
3 x 256 MiB, so the Infinity Cache holds none of them (the window operations'
own tables, 4 B / pixel each, are one buffer per frame size and window and are
rewritten by every call).  A case is timed with device events around bursts of
`--burst` calls, after one untimed burst; the figure is the median burst's time
per call.  No call synchronises.  The yardstick is `_C.copy_roofline` of a copy
that moves what the call has to: 1 B read + 4 B written per pixel for the
integral; for a window operation 2 B read + 4 B written per table, then 16 B
read per table (four corners) and 1 B read (the thresholds) + 1 B written.

    python tools/integral_bench.py --out profiles/integral/integral_bench.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ("16384x16384", "4096x4096")
# name -> (window operation or None for the integral, K, squared / tables)
OPS = {"integral": (None, 0, 1), "integral_sq": (None, 0, 1), "box5": ("box", 5, 1), "box31": ("box", 31, 1),
       "box255": ("box", 255, 1), "std31": ("std", 31, 2), "mean31": ("mean", 31, 1), "sauvola31": ("sauvola", 31, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES), help="comma list of WxH")
    ap.add_argument("--ops", default=",".join(OPS), help="comma list of " + ", ".join(OPS))
    ap.add_argument("--burst", type=int, default=4, help="calls per timed burst")
    ap.add_argument("--bursts", type=int, default=5, help="timed bursts per case")
    ap.add_argument("--yardsticks", type=int, default=1, help="0: skip the copy roofline, the chain and scipy")
    ap.add_argument("--scipy-max", type=int, default=4096 * 4096, help="largest frame scipy filters on the host")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from mpi_cuda_imagemanipulation_amd import ops
    from mpi_cuda_imagemanipulation_amd._native import C

    stream = torch.cuda.current_stream()
    opi = {name: k for k, name in enumerate(C.WINDOW_OPS)}

    def timed(call, pairs):
        n = [0]

        def burst():
            for _ in range(a.burst):
                call(n[0] % pairs)
                n[0] += 1

        burst()  # untimed: clocks, the cached scratch
        torch.cuda.synchronize()
        times = []
        for _ in range(a.bursts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            burst()
            e1.record(stream)
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / a.burst)
        times.sort()
        return times

    med = lambda t: t[len(t) // 2]
    rows, copy_ms = [], {}

    def copy_of(total):
        if total not in copy_ms:
            half = total // 32 * 16
            copy_ms[total] = C.copy_roofline(0, half, max(2, -(-3 * (256 << 20) // (2 * half))), 20)["burst_ms"]
        return copy_ms[total]

    for shape in a.shapes.split(","):
        W, H = (int(v) for v in shape.split("x"))
        px = W * H
        g = torch.Generator(device="cuda")
        g.manual_seed(1)
        frame = torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=g)
        pairs = max(2, -(-3 * (256 << 20) // (px * 5)))
        pairs8 = max(2, -(-3 * (256 << 20) // (px * 2)))
        srcs = [frame] + [frame.clone() for _ in range(pairs8 - 1)]
        planes = [torch.empty((H + 1, W + 1), dtype=torch.int32, device="cuda") for _ in range(pairs)]
        outs = [torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(pairs8)]
        row = {"shape": shape, "pairs_integral": pairs, "pairs_u8": pairs8}
        for name in a.ops.split(","):
            op, K, tables = OPS[name]
            if op is None:
                sq = name.endswith("_sq")
                call = lambda i: C.integral_device(srcs[i].data_ptr(), W, W, H, sq, planes[i].data_ptr(), W + 1,
                                                   stream.cuda_stream)
                t = timed(call, pairs)
                moved = px * 6  # the source twice, the table once
            else:
                kq = C.window_kq(0.2) if op == "sauvola" else 0
                call = lambda i: C.window_device(srcs[i].data_ptr(), W, W, H, opi[op], K, "reflect101", 0, kq,
                                                 outs[i].data_ptr(), W, stream.cuda_stream)
                t = timed(call, pairs8)
                ext = (W + K - 1) * (H + K - 1)
                moved = ext * (2 + 4 * tables) + px * (16 * tables + 2)
            row[name + "_ms"] = round(med(t), 4)
            row[name + "_ms_min"], row[name + "_ms_max"] = round(t[0], 4), round(t[-1], 4)
            if a.yardsticks:
                row[name + "_copy_ms"] = round(copy_of(moved), 4)
                row[name + "_of_copy"] = round(row[name + "_ms"] / row[name + "_copy_ms"], 2)
        if a.yardsticks:
            row["copy5_ms"] = round(copy_of(px * 5), 4)
            row["copy2_ms"] = round(copy_of(px * 2), 4)
            # the chain's compile-time stencils on the same frames (through ops.apply, its engine cached)
            for chain in ("box5", "threshold:adaptive:5"):
                t = timed(lambda i: ops.apply(srcs[i], chain), pairs8)
                row["chain_" + chain.replace(":", "_") + "_ms"] = round(med(t), 4)
            if px <= a.scipy_max:
                try:
                    from scipy import ndimage

                    host = frame.cpu().numpy()
                    for K in (5, 31):
                        t0 = time.perf_counter()
                        ndimage.uniform_filter(host, K, mode="mirror")
                        row[f"scipy_uniform{K}_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                except ImportError:
                    row["scipy_uniform5_ms"] = None
        del srcs, planes, outs, frame
        torch.cuda.empty_cache()
        ops.clear_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
