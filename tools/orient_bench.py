#!/usr/bin/env python3
"""Orientation benchmark: k_orient (`_C.orient_device`) on cache-cold frames beside
the linear copy and the `invert` pass of the same visit.

Every case rotates over enough (source, destination) buffer pairs that a call's
source was last touched pairs-1 calls earlier: pairs * (src + dst) > 3 x 256 MiB,
so the Infinity Cache holds none of it (as tools/resize_bench.py does).  A case
is timed with device events around bursts of `--burst` calls, after one untimed
burst; the figure is the median burst's time per call.  The yardsticks are
`_C.copy_roofline` of the frame's bytes (a copy that moves the same src + dst
bytes) and, for the non-transposing ops, the resident `invert` pass on a frame
of the same shape (the same bytes in the same memory shape).

    python tools/orient_bench.py --out profiles/orient/orient_bench.json
    python tools/orient_bench.py --cases 4096x4096x3:rot90 --bursts 3 --roofline 0 --invert 0   (under rocprofv3)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPS = ("none", "fliph", "rot180", "transpose", "rot90")
DEFAULT_CASES = ",".join(f"{shape}:{op}" for shape in ("16384x16384x3", "16384x16384x1", "4096x4096x3") for op in OPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma list of WxHxC:op")
    ap.add_argument("--burst", type=int, default=8, help="calls per timed burst")
    ap.add_argument("--bursts", type=int, default=7, help="timed bursts per case")
    ap.add_argument("--roofline", type=int, default=1, help="0: skip the copy roofline")
    ap.add_argument("--invert", type=int, default=1, help="0: skip the invert pass beside the non-transposing ops")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from mpi_cuda_imagemanipulation_amd._native import C
    from mpi_cuda_imagemanipulation_amd.models import Pipeline

    stream = torch.cuda.current_stream()
    rows, copy_ms, invert_ms = [], {}, {}
    for case in a.cases.split(","):
        shape, op = case.split(":")
        W, H, Cc = (int(v) for v in shape.split("x"))
        name, bits = C.parse_orient(op)
        W2, H2 = (H, W) if bits & 4 else (W, H)
        nbytes = W * H * Cc
        pairs = max(2, -(-3 * (256 << 20) // (2 * nbytes)))
        srcs = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda") for _ in range(pairs)]
        dsts = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(pairs)]
        n = [0]

        def burst():
            for _ in range(a.burst):
                i = n[0] % pairs
                C.orient_device(srcs[i].data_ptr(), W * Cc, W, H, Cc, dsts[i].data_ptr(), W2 * Cc, name, None,
                                stream.cuda_stream)
                n[0] += 1

        burst()  # untimed: clocks
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
               "ms_max": round(times[-1], 4), "frame_mb": round(nbytes / 2**20, 1),
               "gb_s": round(2 * nbytes / ms / 1e6, 1), "policy": C.launch_policy("orient", cin=Cc, W=W, rows=H)}
        del srcs, dsts
        torch.cuda.empty_cache()
        if a.roofline:
            if shape not in copy_ms:
                half = nbytes // 16 * 16
                copy_ms[shape] = C.copy_roofline(0, half, max(2, -(-3 * (256 << 20) // (2 * half))), 20)["burst_ms"]
            row["copy_ms"] = round(copy_ms[shape], 4)
            row["of_copy"] = round(ms / copy_ms[shape], 2)
        if a.invert and not bits & 4:
            if shape not in invert_ms:
                e = C.Engine(Pipeline("invert").config(W, H, Cc, "device", device=0))
                e.load_synthetic(1)
                e.run(5)
                e.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e.use_external_stream(stream.cuda_stream)
                e0.record(stream)
                e.run(20)
                e1.record(stream)
                torch.cuda.synchronize()
                invert_ms[shape] = e0.elapsed_time(e1) / 20
                del e
            row["invert_ms"] = round(invert_ms[shape], 4)
            row["of_invert"] = round(ms / invert_ms[shape], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
