#!/usr/bin/env python3
"""Distance-transform benchmark: `_C.distance_device` (squared, u8) and
`_C.disk_morph_device` (erode at two radii, open) on cache-cold masks, beside a
linear copy of the same bytes, the `erode5` chain for the erosion of radius 2
and, for the 4096^2 frame, `scipy.ndimage.distance_transform_edt` on the host.

Every case rotates over enough (mask, destination) buffer pairs that a call's
buffers were last touched pairs-1 calls earlier: pairs * bytes per call >
3 x 256 MiB, so the Infinity Cache holds none of them (the transform's own
scratch, 2 B / pixel of g, is one buffer per frame size and is rewritten by
every call).  A case is timed with device events around bursts of `--burst`
calls, after one untimed burst; the figure is the median burst's time per call.
No call synchronises.  The yardstick is `_C.copy_roofline` of a copy that moves
1 byte read + 4 bytes written per pixel (squared) or 1 + 1 (the u8 results).

A case is WxH:KIND:
  background   all zero
  foreground   all 255 (to the background: a frame without any site)
  random0.5    seeded noise at density 0.5
  blobs        gaussian7 of noise, thresholded at 128
  hole_tl      all foreground but the pixel (0, 0)
  disc         a foreground disc of radius min(W, H) / 2 - 1

    python tools/distance_bench.py --out profiles/distance/distance_bench.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ("16384x16384", "4096x4096")
KINDS = ("background", "foreground", "random0.5", "blobs", "hole_tl", "disc")
DEFAULT_CASES = ",".join(f"{s}:{k}" for s in SHAPES for k in KINDS)
# name -> (entry point, argument): the transform's stored form, or the disc operation and its radius
OPS = {"squared": ("distance", 0), "u8": ("distance", 1), "erode2": ("erode", 2.0), "erode40": ("erode", 40.0),
       "open8": ("open", 8.0)}


def make_mask(torch, ops, kind, W, H, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    if kind == "background":
        return torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    if kind == "foreground":
        return torch.full((H, W), 255, dtype=torch.uint8, device="cuda")
    if kind.startswith("random"):
        d = float(kind[len("random"):])
        return (torch.rand((H, W), device="cuda", generator=g) < d).to(torch.uint8) * 255
    if kind == "blobs":
        noise = torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda", generator=g)
        return ops.apply(noise, "gaussian7,threshold:128")
    if kind == "hole_tl":
        m = torch.full((H, W), 255, dtype=torch.uint8, device="cuda")
        m[0, 0] = 0
        return m
    if kind == "disc":
        yy = torch.arange(H, device="cuda")[:, None] - H // 2
        xx = torch.arange(W, device="cuda")[None, :] - W // 2
        r = min(W, H) / 2 - 1
        return ((yy * yy + xx * xx) <= r * r).to(torch.uint8) * 255
    raise SystemExit(f"unknown case kind '{kind}'")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma list of cases")
    ap.add_argument("--ops", default=",".join(OPS), help="comma list of " + ", ".join(OPS))
    ap.add_argument("--burst", type=int, default=4, help="calls per timed burst")
    ap.add_argument("--bursts", type=int, default=5, help="timed bursts per case")
    ap.add_argument("--yardsticks", type=int, default=1, help="0: skip the copy roofline, the erode5 chain and scipy")
    ap.add_argument("--scipy-max", type=int, default=4096 * 4096, help="largest frame scipy transforms on the host")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from mpi_cuda_imagemanipulation_amd import ops
    from mpi_cuda_imagemanipulation_amd._native import C

    stream = torch.cuda.current_stream()

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

    for case in a.cases.split(","):
        f = case.split(":")
        W, H = (int(v) for v in f[0].split("x"))
        kind = f[1]
        px = W * H
        pairs = max(2, -(-3 * (256 << 20) // (px * 5)))
        pairs8 = max(2, -(-3 * (256 << 20) // (px * 2)))
        mask = make_mask(torch, ops, kind, W, H, 1)
        srcs = [mask] + [mask.clone() for _ in range(pairs8 - 1)]
        planes = [torch.empty((H, W), dtype=torch.int32, device="cuda") for _ in range(pairs)]
        outs = [torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(pairs8)]
        row = {"case": case, "pairs_squared": pairs, "pairs_u8": pairs8}
        for name in a.ops.split(","):
            entry, arg = OPS[name]
            if name == "squared":
                call = lambda i: C.distance_device(srcs[i].data_ptr(), W, W, H, False, 0, 0, planes[i].data_ptr(), W,
                                                   stream.cuda_stream)
                t = timed(call, pairs)
            elif name == "u8":
                call = lambda i: C.distance_device(srcs[i].data_ptr(), W, W, H, False, 1, 0, outs[i].data_ptr(), W,
                                                   stream.cuda_stream)
                t = timed(call, pairs8)
            else:
                thr = C.check_radius(arg)
                call = lambda i: C.disk_morph_device(srcs[i].data_ptr(), W, W, H, entry, thr, outs[i].data_ptr(), W,
                                                     stream.cuda_stream)
                t = timed(call, pairs8)
            row[name + "_ms"] = round(med(t), 4)
            row[name + "_ms_min"], row[name + "_ms_max"] = round(t[0], 4), round(t[-1], 4)
        if "squared_ms" in row:
            row["mpx_s"] = round(px / row["squared_ms"] / 1e3, 1)
            d2 = planes[0]
            finite = d2[d2 != C.DISTANCE_NONE]
            row["max_d2"] = int(finite.max()) if finite.numel() else None
        if a.yardsticks:
            row["copy5_ms"] = round(copy_of(px * 5), 4)
            row["copy2_ms"] = round(copy_of(px * 2), 4)
            if "squared_ms" in row:
                row["squared_of_copy"] = round(row["squared_ms"] / row["copy5_ms"], 1)
            if "u8_ms" in row:
                row["u8_of_copy"] = round(row["u8_ms"] / row["copy2_ms"], 1)
            # the 5 x 5 square erosion of the chain on the same masks (through ops.apply, its engine cached)
            t = timed(lambda i: ops.apply(srcs[i], "erode5"), pairs8)
            row["erode5_chain_ms"] = round(med(t), 4)
            if px <= a.scipy_max and kind != "foreground":
                try:
                    from scipy import ndimage

                    host = mask.cpu().numpy()
                    t0 = time.perf_counter()
                    ndimage.distance_transform_edt(host)
                    row["scipy_edt_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                except ImportError:
                    row["scipy_edt_ms"] = None
        del srcs, planes, outs, mask
        torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    ops.clear_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
