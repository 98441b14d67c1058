#!/usr/bin/env python3
"""Mesh warp benchmark: k_remap (`_C.remap_device`) on cache-cold frames beside the
linear copy and, for the rotation, k_warp on the same map, buffers and visit.

Every case rotates over enough (source, destination) buffer pairs that a call's
source was last touched pairs-1 calls earlier: pairs * (src + dst) > 3 x 256 MiB,
so the Infinity Cache holds none of it (as tools/warp_bench.py does).  The mesh
is one buffer (a small one is meant to stay cached; a full map of spacing 1 is
larger than the cache itself).  A case is timed with device events around bursts
of `--burst` calls, after one untimed burst; the figure is the median burst's
time per call.  The yardstick is `_C.copy_roofline` of a copy that moves the same
src + dst + mesh bytes.

A case is WxHxC:KIND[:MODE], MODE bilinear | nearest, the border `constant`:
  rot30     a rotation by 30 degrees about the centre as a mesh of spacing 64, and
            k_warp on the same inverse matrix (the mesh path's cost over the affine kernel)
  keystone  a perspective map (w varies by about 5 % over the frame) at its automatic spacing
  barrel    radial undistortion, k1 = -0.05, at its automatic spacing
  full      the rotation as a full map of spacing 1 (what ops.remap runs)
  minify    a 2x minification at spacing 64: every tile gathers from global memory

    python tools/remap_bench.py --out profiles/remap/remap_bench.json
    python tools/remap_bench.py --cases 16384x16384x3:rot30 --bursts 3 --yardsticks 0   (under rocprofv3)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ("16384x16384x3", "16384x16384x1", "4096x4096x3", "4096x4096x1")
KINDS = ("rot30", "keystone", "barrel", "full", "minify")
DEFAULT_CASES = ",".join(f"{s}:{k}" for s in SHAPES for k in KINDS)


def full_rotation_mesh(torch, minv, W2, H2):
    """The inverse matrix at every pixel, quantised on the device: the mesh of spacing 1 (one row and column
    of padding)."""
    x = torch.arange(W2 + 1, dtype=torch.float64, device="cuda")[None, :]
    y = torch.arange(H2 + 1, dtype=torch.float64, device="cuda")[:, None]
    mesh = torch.empty((H2 + 1, W2 + 1, 2), dtype=torch.int32, device="cuda")
    for c in range(2):
        mesh[:, :, c] = torch.round(4096.0 * (minv[3 * c] * x + minv[3 * c + 1] * y + minv[3 * c + 2])).to(torch.int32)
    return mesh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES, help="comma list of cases")
    ap.add_argument("--burst", type=int, default=8, help="calls per timed burst")
    ap.add_argument("--bursts", type=int, default=7, help="timed bursts per case")
    ap.add_argument("--yardsticks", type=int, default=1, help="0: skip the copy roofline and k_warp")
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
        kind = f[1]
        mode = f[2] if len(f) > 2 else "bilinear"
        W2, H2 = W, H
        minv = None
        if kind in ("rot30", "full"):
            minv, W2, H2 = C.rotate_matrix(30.0, False, W, H)
            if kind == "rot30":
                mesh, S = C.perspective_mesh(list(minv) + [0.0, 0.0, 1.0], True, W, H, W2, H2, 64)
                dm = torch.from_numpy(mesh).cuda()
            else:
                S, dm = 1, full_rotation_mesh(torch, minv, W2, H2)
        elif kind == "keystone":
            k = 16384.0 / max(W, H)
            mesh, S = C.perspective_mesh([1.0, 0.02, 0.0, 0.01, 1.0, 0.0, 2e-6 * k, 1e-6 * k, 1.0], True, W, H, W2, H2)
            dm = torch.from_numpy(mesh).cuda()
        elif kind == "barrel":
            mesh, S = C.radial_mesh(-0.05, 0.0, None, None, W, H)
            dm = torch.from_numpy(mesh).cuda()
        elif kind == "minify":
            W2, H2 = W // 2, H // 2
            mesh, S = C.perspective_mesh([2.0, 0.0, 0.5, 0.0, 2.0, 0.5, 0.0, 0.0, 1.0], True, W, H, W2, H2, 64)
            dm = torch.from_numpy(mesh).cuda()
        else:
            raise SystemExit(f"unknown case kind '{kind}'")
        sb, db, mb = W * H * Cc, W2 * H2 * Cc, dm.numel() * 4
        pairs = max(2, -(-3 * (256 << 20) // (sb + db)))
        srcs = [torch.randint(0, 256, (sb,), dtype=torch.uint8, device="cuda") for _ in range(pairs)]
        dsts = [torch.empty(db, dtype=torch.uint8, device="cuda") for _ in range(pairs)]
        times = timed(lambda i: C.remap_device(srcs[i].data_ptr(), W * Cc, W, H, Cc, dsts[i].data_ptr(), W2 * Cc,
                                               dm.data_ptr(), dm.numel(), S, W2, H2, mode, "constant", 0,
                                               stream.cuda_stream), pairs)
        ms = times[len(times) // 2]
        row = {"case": case, "spacing": S, "dst": [W2, H2], "pairs": pairs, "ms": round(ms, 4),
               "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "src_mb": round(sb / 2**20, 1),
               "dst_mb": round(db / 2**20, 1), "mesh_mb": round(mb / 2**20, 2), "gb_s": round((sb + db + mb) / ms / 1e6, 1),
               "policy": C.launch_policy("remap", cin=Cc, W=W, rows=H, W2=W2, rows2=H2, mesh_bytes=mb)}
        if a.yardsticks and kind == "rot30":
            q = list(C.warp_quantise(minv, True, W, H, W2, H2)[:6])
            t = timed(lambda i: C.warp_device(srcs[i].data_ptr(), W * Cc, W, H, Cc, dsts[i].data_ptr(), W2 * Cc, q, W2,
                                              H2, mode, "constant", 0, stream.cuda_stream), pairs)
            row["warp_ms"] = round(t[len(t) // 2], 4)
            row["of_warp"] = round(ms / t[len(t) // 2], 3)
        del srcs, dsts, dm
        torch.cuda.empty_cache()
        if a.yardsticks:
            key = sb + db + mb
            if key not in copy_ms:
                half = key // 32 * 16
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
