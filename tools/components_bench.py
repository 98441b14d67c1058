#!/usr/bin/env python3
"""Connected-component benchmark: `_C.components_device` (label) and label +
`_C.component_stats_device` (stats) on cache-cold masks, beside a linear copy of
the same bytes and, for the 4096^2 frame, `scipy.ndimage.label` on the host.

Every case rotates over enough (mask, label plane) buffer pairs that a call's
buffers were last touched pairs-1 calls earlier: pairs * (W * H * 5 bytes) >
3 x 256 MiB, so the Infinity Cache holds none of them.  A case is timed with
device events around bursts of `--burst` calls, after one untimed burst; the
figure is the median burst's time per call.  A call ends with its own host
synchronisation (the read-back of N), which the bursts therefore include.  The
yardstick is `_C.copy_roofline` of a copy that moves 1 byte read + 4 bytes
written per pixel.

A case is WxH:KIND[:CONN], CONN 4 | 8 (default 8):
  background   all zero
  foreground   all 255
  random0.5    seeded noise at density 0.5
  random0.593  seeded noise at density 0.593 (the site-percolation threshold of 4-connectivity)
  blobs        gaussian7 of noise, thresholded at 128

    python tools/components_bench.py --out profiles/components/components_bench.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ("16384x16384", "4096x4096")
KINDS = ("background", "foreground", "random0.5", "random0.593", "blobs")
DEFAULT_CASES = ",".join(f"{s}:{k}" for s in SHAPES for k in KINDS)


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
    raise SystemExit(f"unknown case kind '{kind}'")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma list of cases")
    ap.add_argument("--burst", type=int, default=4, help="calls per timed burst")
    ap.add_argument("--bursts", type=int, default=5, help="timed bursts per case")
    ap.add_argument("--yardsticks", type=int, default=1, help="0: skip the copy roofline and scipy")
    ap.add_argument("--scipy-max", type=int, default=4096 * 4096, help="largest frame scipy labels on the host")
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

        burst()  # untimed: clocks, the cached temporaries
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
        W, H = (int(v) for v in f[0].split("x"))
        kind = f[1]
        conn = int(f[2]) if len(f) > 2 else 8
        total = W * H * 5
        pairs = max(2, -(-3 * (256 << 20) // total))
        mask = make_mask(torch, ops, kind, W, H, 1)
        srcs = [mask] + [mask.clone() for _ in range(pairs - 1)]
        labs = [torch.empty((H, W), dtype=torch.int32, device="cuda") for _ in range(pairs)]
        n_of = [0]

        def label(i):
            n_of[0] = C.components_device(srcs[i].data_ptr(), W, W, H, conn, labs[i].data_ptr(), W, stream.cuda_stream)

        label(0)
        n = n_of[0]
        table = torch.empty((n + 1, 7), dtype=torch.int64, device="cuda")

        def label_stats(i):
            label(i)
            C.component_stats_device(labs[i].data_ptr(), W, W, H, n, table.data_ptr(), stream.cuda_stream)

        def stats_only(i):
            C.component_stats_device(labs[i].data_ptr(), W, W, H, n, table.data_ptr(), stream.cuda_stream)

        t_label = timed(label, pairs)
        t_both = timed(label_stats, pairs)
        t_stats = timed(stats_only, pairs)
        med = lambda t: t[len(t) // 2]
        row = {"case": case, "connectivity": conn, "n": n, "pairs": pairs, "label_ms": round(med(t_label), 4),
               "label_ms_min": round(t_label[0], 4), "label_ms_max": round(t_label[-1], 4),
               "label_stats_ms": round(med(t_both), 4), "label_stats_ms_min": round(t_both[0], 4),
               "label_stats_ms_max": round(t_both[-1], 4), "stats_ms": round(med(t_stats), 4),
               "mpx_s": round(W * H / med(t_label) / 1e3, 1)}
        if a.yardsticks:
            if total not in copy_ms:
                half = total // 32 * 16
                copy_ms[total] = C.copy_roofline(0, half, max(2, -(-3 * (256 << 20) // (2 * half))), 20)["burst_ms"]
            row["copy_ms"] = round(copy_ms[total], 4)
            row["label_of_copy"] = round(med(t_label) / copy_ms[total], 1)
            if W * H <= a.scipy_max:
                try:
                    import numpy as np
                    from scipy import ndimage

                    host = mask.cpu().numpy()
                    st = ndimage.generate_binary_structure(2, 1) if conn == 4 else np.ones((3, 3), int)
                    t0 = time.perf_counter()
                    _, sn = ndimage.label(host, structure=st)
                    row["scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    row["scipy_n"] = int(sn)
                except ImportError:
                    row["scipy_ms"] = None
        del srcs, labs, mask, table
        torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
