#!/usr/bin/env python3
"""Canny benchmark: `_C.canny_device` under both norms, `_C.canny_classes_device`
alone and `_C.hysteresis_device` alone on cache-cold gray frames (seeded noise,
its 5 x 5 box mean, and the `blobs` frame of tools/components_bench.py), beside
a linear copy of the same bytes read and written, the chain's `sobel` on the
same frame and `_C.components_device` on the same class map (the bar the forest
form of the hysteresis should beat: it skips the numbering).

Every case rotates over enough (source, destination) buffer pairs that a call's
buffers were last touched pairs-1 calls earlier: pairs * bytes per call >
3 x 256 MiB, so the Infinity Cache holds none of them (the calls' own class and
forest planes are one buffer per frame size and are rewritten by every call).  A
case is timed with device events around bursts of `--burst` calls, after one
untimed burst; the figure is the median burst's time per call.  canny_device,
hysteresis_device and components_device synchronise the stream once per call
(the read-back of an error word or of N), so their figures include that wait.
The copy yardstick moves 1 B read + 1 B written per pixel.

    python tools/canny_bench.py --out profiles/canny/canny_bench.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ("16384x16384", "4096x4096")
KINDS = ("noise", "blur", "blobs")
LOW, HIGH = 40, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES), help="comma list of WxH")
    ap.add_argument("--kinds", default=",".join(KINDS), help="comma list of " + ", ".join(KINDS))
    ap.add_argument("--burst", type=int, default=4, help="calls per timed burst")
    ap.add_argument("--bursts", type=int, default=5, help="timed bursts per case")
    ap.add_argument("--yardsticks", type=int, default=1, help="0: skip the copy roofline, the chain and the labelling")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from mpi_cuda_imagemanipulation_amd import ops
    from mpi_cuda_imagemanipulation_amd._native import C

    stream = torch.cuda.current_stream()
    s = stream.cuda_stream

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

    rows = []
    for shape in a.shapes.split(","):
        W, H = (int(v) for v in shape.split("x"))
        px = W * H
        pairs = max(2, -(-3 * (256 << 20) // (px * 2)))
        copy_ms = None
        if a.yardsticks:
            half = px // 16 * 16
            copy_ms = C.copy_roofline(0, half, max(2, -(-3 * (256 << 20) // (2 * half))), 20)["burst_ms"]
        for kind in a.kinds.split(","):
            g = torch.Generator(device="cuda")
            g.manual_seed(1)
            frame = torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=g)
            if kind == "blur":
                frame = ops.box_filter(frame, 5)
            elif kind == "blobs":
                frame = ops.apply(frame, "gaussian7,threshold:128")
            elif kind != "noise":
                raise SystemExit(f"unknown kind '{kind}'")
            srcs = [frame] + [frame.clone() for _ in range(pairs - 1)]
            outs = [torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(pairs)]
            row = {"shape": shape, "kind": kind, "pairs": pairs, "low": LOW, "high": HIGH}
            cases = {
                "canny_l1": lambda i: C.canny_device(srcs[i].data_ptr(), W, W, H, LOW, HIGH, "l1", "reflect101",
                                                     outs[i].data_ptr(), W, s),
                "canny_l2": lambda i: C.canny_device(srcs[i].data_ptr(), W, W, H, LOW, HIGH, "l2", "reflect101",
                                                     outs[i].data_ptr(), W, s),
                "classes_l1": lambda i: C.canny_classes_device(srcs[i].data_ptr(), W, W, H, LOW, HIGH, "l1", "reflect101",
                                                               outs[i].data_ptr(), W, s),
                "hysteresis": lambda i: C.hysteresis_device(srcs[i].data_ptr(), W, W, H, LOW, HIGH, 8,
                                                            outs[i].data_ptr(), W, s),
            }
            for name, call in cases.items():
                t = timed(call, pairs)
                row[name + "_ms"] = round(t[len(t) // 2], 4)
                row[name + "_ms_min"], row[name + "_ms_max"] = round(t[0], 4), round(t[-1], 4)
            edges = outs[(a.burst * (a.bursts + 1) - 1) % pairs]
            row["edge_fraction"] = round(float((edges == 255).float().mean().item()), 5)
            if a.yardsticks:
                row["copy_ms"] = round(copy_ms, 4)
                t = timed(lambda i: ops.apply(srcs[i], "sobel"), pairs)
                row["chain_sobel_ms"] = round(t[len(t) // 2], 4)
                # the labelling of the same class map (class != 0 is foreground)
                cls = ops.canny_classes(frame, LOW, HIGH)
                row["class_fraction"] = round(float((cls != 0).float().mean().item()), 5)
                clss = [cls] + [cls.clone() for _ in range(pairs - 1)]
                labels = torch.empty((H, W), dtype=torch.int32, device="cuda")
                t = timed(lambda i: C.components_device(clss[i].data_ptr(), W, W, H, 8, labels.data_ptr(), W, s), pairs)
                row["components_on_classes_ms"] = round(t[len(t) // 2], 4)
                # and the hysteresis of the same map: the class plane as pixels, thresholds 0 / 1
                t = timed(lambda i: C.hysteresis_device(clss[i].data_ptr(), W, W, H, 0, 1, 8, outs[i].data_ptr(), W, s), pairs)
                row["hysteresis_on_classes_ms"] = round(t[len(t) // 2], 4)
                del clss, labels, cls
            del srcs, outs, frame
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
