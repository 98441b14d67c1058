#!/usr/bin/env python3
"""Affine warp benchmark: k_warp (`_C.warp_device`) on cache-cold frames beside the
linear copy, k_orient and k_resize of the same visit.

Every case rotates over enough (source, destination) buffer pairs that a call's
source was last touched pairs-1 calls earlier: pairs * (src + dst) > 3 x 256 MiB,
so the Infinity Cache holds none of it (as tools/orient_bench.py does).  A case
is timed with device events around bursts of `--burst` calls, after one untimed
burst; the figure is the median burst's time per call.  The yardsticks are
`_C.copy_roofline` of a copy that moves the same src + dst bytes, k_orient's
`rot270` beside `rot:90:fit` (the same pixels) and k_resize's bilinear beside a
scale.

A case is WxHxC:rot:DEG:same|fit:MODE or WxHxC:scale:S:MODE (the frame scaled by
S about its first pixel, destination S*W x S*H), MODE bilinear | nearest; the
border is `constant`.

    python tools/warp_bench.py --out profiles/warp/warp_bench.json
    python tools/warp_bench.py --cases 16384x16384x3:rot:45:same:bilinear --bursts 3 --yardsticks 0   (under rocprofv3)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ("16384x16384x3", "16384x16384x1", "4096x4096x3")
ROTS = ("rot:0:same:bilinear", "rot:1:same:bilinear", "rot:30:same:bilinear", "rot:45:same:bilinear",
        "rot:90:fit:bilinear", "rot:30:same:nearest")
DEFAULT_CASES = ",".join([f"{s}:{r}" for s in SHAPES for r in ROTS] + ["16384x16384x3:scale:0.5:bilinear"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma list of cases")
    ap.add_argument("--burst", type=int, default=8, help="calls per timed burst")
    ap.add_argument("--bursts", type=int, default=7, help="timed bursts per case")
    ap.add_argument("--yardsticks", type=int, default=1, help="0: skip the copy roofline, k_orient and k_resize")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from mpi_cuda_imagemanipulation_amd._native import C

    stream = torch.cuda.current_stream()

    def timed(call, pairs):
        n = [0]

        def burst():
            for _ in range(a.burst):
                call(n[0] % pairs)
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
        return times

    rows, copy_ms = [], {}
    for case in a.cases.split(","):
        f = case.split(":")
        W, H, Cc = (int(v) for v in f[0].split("x"))
        if f[1] == "rot":
            minv, W2, H2 = C.rotate_matrix(float(f[2]), f[3] == "fit", W, H)
            mode = f[4]
        else:
            s = float(f[2])
            minv, W2, H2 = [1 / s, 0, 0, 0, 1 / s, 0], max(1, int(W * s)), max(1, int(H * s))
            mode = f[3]
        q = list(C.warp_quantise(minv, True, W, H, W2, H2)[:6])
        sb, db = W * H * Cc, W2 * H2 * Cc
        pairs = max(2, -(-3 * (256 << 20) // (sb + db)))
        srcs = [torch.randint(0, 256, (sb,), dtype=torch.uint8, device="cuda") for _ in range(pairs)]
        dsts = [torch.empty(db, dtype=torch.uint8, device="cuda") for _ in range(pairs)]
        times = timed(lambda i: C.warp_device(srcs[i].data_ptr(), W * Cc, W, H, Cc, dsts[i].data_ptr(), W2 * Cc, q, W2,
                                              H2, mode, "constant", 0, stream.cuda_stream), pairs)
        ms = times[len(times) // 2]
        row = {"case": case, "plan": C.warp_plan(q), "dst": [W2, H2], "pairs": pairs, "ms": round(ms, 4),
               "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "src_mb": round(sb / 2**20, 1),
               "dst_mb": round(db / 2**20, 1), "gb_s": round((sb + db) / ms / 1e6, 1),
               "policy": C.launch_policy("warp", cin=Cc, W=W, rows=H, W2=W2, rows2=H2)}
        if a.yardsticks:
            if f[1] == "rot" and f[2] == "90" and f[3] == "fit":
                t = timed(lambda i: C.orient_device(srcs[i].data_ptr(), W * Cc, W, H, Cc, dsts[i].data_ptr(), W2 * Cc,
                                                    "rot270", None, stream.cuda_stream), pairs)
                row["orient_rot270_ms"] = round(t[len(t) // 2], 4)
                row["of_orient"] = round(ms / t[len(t) // 2], 2)
            if f[1] == "scale":
                t = timed(lambda i: C.resize_device(srcs[i].data_ptr(), W * Cc, W, H, Cc, dsts[i].data_ptr(), W2 * Cc,
                                                    W2, H2, "bilinear", stream.cuda_stream), pairs)
                row["resize_bilinear_ms"] = round(t[len(t) // 2], 4)
                row["of_resize"] = round(ms / t[len(t) // 2], 2)
        del srcs, dsts
        torch.cuda.empty_cache()
        if a.yardsticks:
            key = (sb, db)
            if key not in copy_ms:
                half = (sb + db) // 32 * 16
                copy_ms[key] = C.copy_roofline(0, half, max(2, -(-3 * (256 << 20) // (2 * half))), 20)["burst_ms"]
            row["copy_ms"] = round(copy_ms[key], 4)
            row["of_copy"] = round(ms / copy_ms[key], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
