"""`python -m mpi_cuda_imagemanipulation_amd` - Python front end of the native
engine for any image format Pillow reads (the native `bin/stripe` CLI is
PNM-only).  The reference's single command (kernel.cu main: load, distribute,
gray -> contrast -> emboss, gather, write) is `run --preset ref-gpu`.

  python -m mpi_cuda_imagemanipulation_amd run --input in.jpg --output out.png \\
      --chain gray:ref,contrast:3.5,emboss3 --ranks 4 --backend local
  python -m mpi_cuda_imagemanipulation_amd run --input in.jpg --output out.png --resize 1920x1080 --chain sharpen
  python -m mpi_cuda_imagemanipulation_amd run --input phone.jpg --output out.png --orient auto --crop 800x600+40+0
  python -m mpi_cuda_imagemanipulation_amd convert in.jpg out.ppm
  python -m mpi_cuda_imagemanipulation_amd filters

One process per rank, like the reference's `mpiexec -n N kernel.exe`
(kernel.cu:104-137 Init/Bcast/Scatter, :223-225 Gather): under torchrun,
`--backend rccl` (one GPU per process, RCCL over xGMI) or `--backend gloo`
(CPU golden engine) - rank 0 reads the image, broadcasts its shape (the
reference's 4-int metadata Bcast), scatters the stripes, every rank filters
its stripe with halo exchange, rank 0 gathers and writes:

  torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m mpi_cuda_imagemanipulation_amd \\
      run --input in.jpg --output out.png --preset ref-gpu --backend rccl
"""
from __future__ import annotations

import argparse
import json
import sys
import time


def main(argv=None) -> int:
    from . import models, ops, utils
    from ._native import C

    ap = argparse.ArgumentParser(prog="python -m mpi_cuda_imagemanipulation_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run", help="filter an image (distributed over in-process ranks)")
    r.add_argument("--input", required=True)
    r.add_argument("--output", required=True)
    r.add_argument("--chain", default=None)
    r.add_argument("--preset", default=None, choices=sorted(models.PRESETS))
    r.add_argument("--ranks", type=int, default=1)
    r.add_argument("--backend", default="auto", choices=["auto", "local", "host", "rccl", "gloo", "gloo-gpu"],
                   help="local: N logical ranks on this process's GPU; host: CPU golden engine; "
                        "rccl / gloo / gloo-gpu: one process per rank under torchrun (RANK / WORLD_SIZE env; "
                        "gloo-gpu: GPU engines sharing GPUs, gloo transport through pinned host memory)")
    r.add_argument("--border", default=None)
    r.add_argument("--iterations", type=int, default=1)
    r.add_argument("--dist-chunks", type=int, default=0,
                   help="> 1 ranks, one iteration, single-pass chains: ship / filter / gather the "
                        "stripes in this many overlapped row chunks (bit-identical)")
    r.add_argument("--row-weights", default=None,
                   help="comma list, one share per rank (weighted split, e.g. a larger root share for "
                        "--dist-chunks); default: even rows")
    r.add_argument("--resize", default=None, metavar="WxH[:mode]",
                   help="resize the loaded frame before the chain (mode: auto | nearest | bilinear | area); "
                        "on the GPU for GPU backends, on the host executor for host / gloo")
    r.add_argument("--orient", default=None, metavar="OP|auto",
                   help="orient the loaded frame before --resize and the chain: none | fliph | rot180 | flipv | "
                        "transpose | rot90 (cw) | transverse | rot270 (ccw) | exif:N | auto (the Exif Orientation "
                        "of a JPEG input, none for any other format); without it the stored pixels are used")
    r.add_argument("--crop", default=None, metavar="WxH+X+Y",
                   help="a window of the oriented frame, cut in the same pass")
    w = r.add_mutually_exclusive_group()
    w.add_argument("--rotate", default=None, metavar="DEG[:same|fit]",
                   help="rotate the frame counter-clockwise about its centre, after --orient / --crop and before "
                        "--resize (fit: the frame grows to hold the turn); use --rotate=-30 for a negative angle")
    w.add_argument("--warp", default=None, metavar="a;b;c;d;e;f[:WxH]",
                   help="warp the frame by the forward 2x3 matrix (source -> destination, like cv2.warpAffine); "
                        "WxH: the destination size (default: the source's)")
    w.add_argument("--perspective", default=None, metavar="h00;...;h22[:WxH]",
                   help="warp the frame by the forward 3x3 matrix (source -> destination, like cv2.warpPerspective), in "
                        "the slot of --rotate / --warp")
    w.add_argument("--quad", default=None, metavar="x0,y0;x1,y1;x2,y2;x3,y3[:WxH]",
                   help="straighten the source quadrilateral TL TR BR BL to a rectangle (default size: its longer sides)")
    w.add_argument("--undistort", default=None, metavar="k1[;k2[;f[;cx;cy]]]",
                   help="radial lens undistortion (f default: half the diagonal; centre default: the frame's); use "
                        "--undistort=-0.1 for a negative k1")
    r.add_argument("--warp-mode", default=None, choices=["bilinear", "nearest"])
    r.add_argument("--warp-border", default=None, metavar="constant[:V]|replicate",
                   help="taps outside the frame: the fill value V (default 0) or the clamped pixel")
    r.add_argument("--verbose", "-v", action="store_true", help="rank-prefixed progress log on stderr")
    c = sub.add_parser("convert", help="convert between image formats")
    c.add_argument("src")
    c.add_argument("dst")
    sub.add_parser("filters", help="list the filter syntax")
    a = ap.parse_args(argv)

    if a.cmd == "filters":
        for k, v in ops.FILTERS.items():
            print(f"{k:24s} {v}")
        return 0
    if a.cmd == "convert":
        utils.write_image(a.dst, utils.read_image(a.src))
        return 0
    if a.preset:
        pipe = models.Pipeline.preset(a.preset)
    else:
        pipe = models.Pipeline(a.chain or "gaussian5", border=a.border or "reflect101")
    pipe.dist_chunks = a.dist_chunks
    weights = [float(v) for v in a.row_weights.split(",")] if a.row_weights else None
    if a.verbose:
        import os

        os.environ["STRIPE_LOG"] = "INFO"
    if a.backend in ("rccl", "gloo", "gloo-gpu"):
        return _run_per_process(a, pipe)
    img = utils.read_image(a.input)
    backend = a.backend
    if backend == "auto":
        import torch

        backend = "local" if torch.cuda.is_available() else "host"
    img, oriented = _orient_input(a, img, backend != "host")
    img, warped = _warp_input(a, img, backend != "host")
    oriented = {**oriented, **warped}
    img, resized_from = _resize_input(a, img, backend != "host")
    t0 = time.perf_counter()
    log = utils.get_logger("cli", 0)
    log.info("run %s on %s, %d ranks (%s)", pipe.spec.chain, img.shape, a.ranks, backend)
    out = pipe.run_distributed(img, a.ranks, backend=backend, iterations=a.iterations, row_weights=weights)
    ms = (time.perf_counter() - t0) * 1e3
    utils.write_image(a.output, out)
    print(json.dumps({"cmd": "run", "input": a.input, "output": a.output, "shape": list(img.shape),
                      "chain": pipe.spec.chain, "ranks": a.ranks, "backend": backend, "wall_ms": round(ms, 3),
                      **oriented, **({"resized_from": resized_from} if resized_from else {})}))
    return 0


def _orient_input(a, img, on_gpu):
    """--orient OP|auto and --crop WxH+X+Y on the loaded frame, one pass: (frame, JSON members)."""
    if not a.orient and not a.crop:
        return img, {}
    import numpy as np

    from . import ops
    from ._native import C

    token = a.orient or "none"
    if token == "auto":
        token = f"exif:{ops.exif_orientation(a.input)}"
    name = C.parse_orient(token)[0]
    H, W = img.shape[:2]
    crop = None
    if a.crop:
        ow, oh = (H, W) if C.parse_orient(name)[1] & 4 else (W, H)
        crop = C.parse_crop_spec(a.crop, ow, oh)
    if on_gpu:
        import torch

        out = ops.orient(torch.from_numpy(np.ascontiguousarray(img)).cuda(), name, crop).cpu().numpy()
    else:
        out = ops.orient(np.ascontiguousarray(img), name, crop)
    return out, {"oriented": name, "cropped_from": [int(W), int(H)]}


def _warp_input(a, img, on_gpu):
    """--rotate DEG[:same|fit], --warp a;b;c;d;e;f[:WxH], --perspective, --quad or --undistort on the loaded frame:
    (frame, JSON members)."""
    if not (a.rotate or a.warp or a.perspective or a.quad or a.undistort):
        if a.warp_mode or a.warp_border:
            raise SystemExit("--warp-mode and --warp-border need --rotate or --warp (or --perspective, --quad, "
                             "--undistort)")
        return img, {}
    import numpy as np

    from . import ops
    from ._native import C

    H, W = img.shape[:2]
    border, fill = C.parse_warp_border(a.warp_border or "constant")
    kw = dict(mode=C.parse_warp_mode(a.warp_mode or "bilinear"), border=border, fill=fill)
    x = np.ascontiguousarray(img)
    if on_gpu:
        import torch

        x = torch.from_numpy(x).cuda()
    extra = {}
    if a.perspective or a.quad or a.undistort:
        # the mesh is built here so that its spacing can be reported; ops.mesh_warp runs it
        if a.perspective:
            Hm, W2, H2 = C.parse_perspective_spec(a.perspective)
            W2, H2 = W2 or W, H2 or H
            token = C.perspective_token(Hm, W2, H2)
            mesh, spacing = C.perspective_mesh(Hm, False, W, H, W2, H2, 0, a.perspective)
        elif a.quad:
            pts, W2, H2 = C.parse_quad_spec(a.quad)
            token = C.quad_token(pts, W2, H2)
            mesh, spacing = C.perspective_mesh(C.quad_matrix(pts, W2, H2)[0], False, W, H, W2, H2, 0, a.quad)
        else:
            k1, k2, f, centre = C.parse_undistort_spec(a.undistort)
            W2, H2 = W, H
            token = C.undistort_token(a.undistort, W, H)
            mesh, spacing = C.radial_mesh(k1, k2, f, centre, W, H, 0, a.undistort)
        out = ops.mesh_warp(x, mesh, spacing, size=(H2, W2), **kw)
        extra = {"mesh_spacing": int(spacing)}
    elif a.rotate:
        deg, fit, token = C.parse_rotate_spec(a.rotate)
        out = ops.rotate(x, deg, expand=fit, **kw)
    else:
        M, W2, H2 = C.parse_warp_spec(a.warp)
        W2, H2 = W2 or W, H2 or H
        token = C.warp_token(M, W2, H2)
        out = ops.warp_affine(x, M, size=(H2, W2), **kw)
    if on_gpu:
        out = out.cpu().numpy()
    return out, {"warped_from": [int(W), int(H)], "warp": token, **extra}


def _resize_input(a, img, on_gpu):
    """--resize WxH[:mode] on the loaded frame: (frame, [W, H] it had, or None)."""
    if not a.resize:
        return img, None
    import numpy as np

    from . import ops
    from ._native import C

    W2, H2, mode = C.parse_resize_spec(a.resize)
    from_wh = [int(img.shape[1]), int(img.shape[0])]
    if on_gpu:
        import torch

        out = ops.resize(torch.from_numpy(np.ascontiguousarray(img)).cuda(), size=(H2, W2), mode=mode).cpu().numpy()
    else:
        out = ops.resize(np.ascontiguousarray(img), size=(H2, W2), mode=mode)
    return out, from_wh


def _run_per_process(a, pipe) -> int:
    """One rank per process (torchrun env): root load -> metadata broadcast ->
    scatter -> per-stripe chain with halo exchange -> gather -> root write."""
    import numpy as np
    import torch.distributed as dist

    from . import parallel, utils

    ctx = parallel.init(a.backend)
    log = utils.get_logger("cli", ctx.rank)
    img = utils.read_image(a.input) if ctx.rank == 0 else None
    resized_from = None
    oriented = {}
    if ctx.rank == 0:  # rank 0 orients, crops and resizes before it broadcasts the geometry
        img, oriented = _orient_input(a, img, a.backend in ("rccl", "gloo-gpu"))
        img, warped = _warp_input(a, img, a.backend in ("rccl", "gloo-gpu"))
        oriented = {**oriented, **warped}
        img, resized_from = _resize_input(a, img, a.backend in ("rccl", "gloo-gpu"))
    meta = [None if img is None else tuple(img.shape)]
    if ctx.world > 1:
        dist.broadcast_object_list(meta, src=0)
    shape = meta[0]
    H, W = shape[:2]
    Cc = 1 if len(shape) == 2 else shape[2]
    weights = [float(v) for v in a.row_weights.split(",")] if a.row_weights else None
    dp = parallel.DistributedPipeline(ctx, pipe, W, H, Cc, root_buffers=True, row_weights=weights)
    log.info("stripe rows %s of %dx%dx%d, chain %s", dp.stripe, W, H, Cc, pipe.spec.chain)
    dp.load_root(img)
    if ctx.world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    if a.iterations == 1 and dp.engine.dist_chunks(a.dist_chunks) > 0:
        dp.engine.run_dist(a.dist_chunks)
    else:
        dp.scatter()
        dp.run(a.iterations)
        dp.gather()
    dp.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    log.info("dist step %.3f ms", ms)
    if ctx.rank == 0:
        out = dp.result_root()
        utils.write_image(a.output, np.ascontiguousarray(out))
        print(json.dumps({"cmd": "run", "input": a.input, "output": a.output, "shape": list(shape),
                          "chain": pipe.spec.chain, "ranks": ctx.world, "backend": a.backend,
                          "stripe_rows": dp.stripe[1], "dist_ms": round(ms, 3),
                          **oriented, **({"resized_from": resized_from} if resized_from else {})}))
    if ctx.world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
