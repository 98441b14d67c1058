#!/usr/bin/env python3
"""Resize benchmark: k_resize (`_C.resize_device`) on cache-cold frames beside the
linear copy of the same visit.

Every case rotates over enough (source, destination) buffer pairs that a call's
source was last touched pairs-1 calls earlier: pairs * (src + dst) > 3 x 256 MiB,
so the Infinity Cache holds none of it (as tools/coldbench.py does).  A case is
timed with device events around bursts of `--burst` calls, after one untimed
burst; the figure is the median burst's time per call.  The yardstick is
`_C.copy_roofline` of (src + dst) / 2 bytes, a copy that moves the same
src + dst bytes; `--gaussian5` adds the resident gaussian5 pass on the source
frame for the 2x downscale.

    python tools/resize_bench.py --out profiles/resize/resize_bench.json
    python tools/resize_bench.py --cases 4096x4096x3:8192x8192:bilinear --bursts 3   (under rocprofv3)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULT_CASES = ("16384x16384x3:8192x8192:area,16384x16384x3:4096x4096:area,16384x16384x3:512x512:area,"
                 "16384x16384x1:4096x4096:area,4096x4096x3:8192x8192:bilinear")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma list of WxHxC:W2xH2:mode")
    ap.add_argument("--burst", type=int, default=8, help="calls per timed burst")
    ap.add_argument("--bursts", type=int, default=7, help="timed bursts per case")
    ap.add_argument("--roofline", type=int, default=1, help="0: skip the copy roofline")
    ap.add_argument("--gaussian5", type=int, default=1, help="0: skip gaussian5 on the source of 2x downscales")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from mpi_cuda_imagemanipulation_amd._native import C
    from mpi_cuda_imagemanipulation_amd.models import Pipeline

    stream = torch.cuda.current_stream()
    rows = []
    for case in a.cases.split(","):
        shape, size, mode = case.split(":")
        W, H, Cc = (int(v) for v in shape.split("x"))
        W2, H2 = (int(v) for v in size.split("x"))
        src_b, dst_b = W * H * Cc, W2 * H2 * Cc
        pairs = max(2, -(-3 * (256 << 20) // (src_b + dst_b)))
        srcs = [torch.randint(0, 256, (src_b,), dtype=torch.uint8, device="cuda") for _ in range(pairs)]
        dsts = [torch.empty(dst_b, dtype=torch.uint8, device="cuda") for _ in range(pairs)]
        n = [0]

        def burst():
            for _ in range(a.burst):
                i = n[0] % pairs
                C.resize_device(srcs[i].data_ptr(), W * Cc, W, H, Cc, dsts[i].data_ptr(), W2 * Cc, W2, H2, mode,
                                stream.cuda_stream)
                n[0] += 1

        burst()  # untimed: tables, clocks
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
        ms = times[len(times) // 2]
        row = {"case": case, "pairs": pairs, "ms": round(ms, 4), "ms_min": round(times[0], 4),
               "ms_max": round(times[-1], 4), "src_mb": round(src_b / 2**20, 1), "dst_mb": round(dst_b / 2**20, 1),
               "gb_s": round((src_b + dst_b) / ms / 1e6, 1),
               "policy": C.launch_policy("resize", cin=Cc, W=W, rows=H, W2=W2, rows2=H2)}
        del srcs, dsts
        torch.cuda.empty_cache()
        if a.roofline:
            half = (src_b + dst_b) // 2 // 16 * 16
            r = C.copy_roofline(0, half, max(2, -(-3 * (256 << 20) // (2 * half))), 20)
            row["copy_ms"] = round(r["burst_ms"], 4)
            row["copy_gb_s"] = round(2 * half / r["burst_ms"] / 1e6, 1)
            row["of_copy"] = round(ms / r["burst_ms"], 2)
        if a.gaussian5 and (W, H) == (2 * W2, 2 * H2):
            e = C.Engine(Pipeline("gaussian5").config(W, H, Cc, "device", device=0))
            e.load_synthetic(1)
            e.run(5)
            e.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e.use_external_stream(stream.cuda_stream)
            e0.record(stream)
            e.run(20)
            e1.record(stream)
            torch.cuda.synchronize()
            row["gaussian5_ms"] = round(e0.elapsed_time(e1) / 20, 4)
            del e
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
