"""k_remap (csrc/hip/remap.hip) on the GPU, bit-exact against golden_remap: the
mirror test's shapes, spacings, modes and borders; identity, translation,
rotation, keystone and barrel meshes; a minification whose tiles all gather from
global memory; a mesh whose left tiles fit the staged box and whose right tiles
do not; a mesh wholly outside the frame; seeded random meshes near the identity
and anywhere in +-2^18 pixels; unaligned pitched views with guard bytes; a
source that ends its tensor; both store policies; a second stream; the torch
front end; the launch checks; the CLI.  Frames stay within 200 pixels a side."""
import json
import os
import subprocess

import numpy as np
import pytest

import mpi_cuda_imagemanipulation_amd as m
import np_remap as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = m._C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPE = os.path.join(ROOT, "bin", "stripe")
TILE = C.remap_tile()
T = TILE["tile"]
BORDERS = (("constant", 0), ("constant", 200), ("replicate", 0))
MODES = ("bilinear", "nearest")


def frame(W, H, ch):
    shape = (H, W) if ch == 1 else (H, W, ch)
    return np.random.default_rng(W * 7919 + H * 31 + ch).integers(0, 256, shape, dtype=np.uint8)


def device_remap(x, dm, S, W2, H2, mode, border, fill):
    """k_remap on a contiguous CUDA tensor and a CUDA mesh through the raw binding."""
    H, W = x.shape[:2]
    ch = 1 if x.ndim == 2 else x.shape[2]
    out = torch.empty((H2, W2) + tuple(x.shape[2:]), dtype=torch.uint8, device="cuda")
    C.remap_device(x.data_ptr(), W * ch, W, H, ch, out.data_ptr(), W2 * ch, dm.data_ptr(), dm.numel(), S, W2, H2, mode,
                   border, fill, torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()


def check(a, mesh, S, W2, H2, modes=MODES, borders=BORDERS, what=None):
    x = torch.from_numpy(a).cuda()
    dm = torch.from_numpy(np.ascontiguousarray(mesh)).cuda()
    for mode in modes:
        for border, fill in borders:
            ref = C.golden_remap(a, mesh, S, W2, H2, mode, border, fill)
            got = device_remap(x, dm, S, W2, H2, mode, border, fill)
            assert got.shape == ref.shape
            assert (got == ref).all(), (what, a.shape, S, W2, H2, mode, border, fill, int((got != ref).sum()))


def test_tile_constants():
    assert TILE == dict(tile=64, box=92, lds_spacing=4, nodes=17, node_bytes=2312, reduce_bytes=64,
                        lds_gray=8464 + 2312 + 64, lds_rgb=25392 + 2312 + 64)
    assert TILE["box"] == C.warp_tile()["box"] and TILE["tile"] == C.warp_tile()["tile"]


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("S", R.SPACINGS)
def test_mirror_shapes(ch, S):
    a = frame(90, 70, ch)
    for W2, H2 in ((63, 65), (64, 64), (65, 63), (131, 9), (9, 131), (1, 1)):
        check(a, R.random_mesh(S, W2, H2, seed=S * 1000 + W2, spread=40), S, W2, H2, what="near")
    one = frame(1, 1, ch)
    check(one, R.random_mesh(S, 9, 7, seed=3, spread=2), S, 9, 7, what="1x1 source")
    check(one, R.identity_mesh(S, 1, 1), S, 1, 1, what="1x1 both")


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("S", R.SPACINGS)
def test_named_meshes(ch, S):
    W, H = 150, 131
    a = frame(W, H, ch)
    x = torch.from_numpy(a).cuda()
    ident = R.identity_mesh(S, W, H)
    got = device_remap(x, torch.from_numpy(ident).cuda(), S, W, H, "bilinear", "constant", 0)
    assert (got == a).all()
    check(a, ident, S, W, H, what="identity")
    check(a, R.translation_mesh(S, W, H, 3, -5), S, W, H, what="translation")
    check(a, R.rotation_mesh(S, W, H, 30.0, (W - 1) / 2, (H - 1) / 2), S, W, H, what="rot30")
    check(a, C.perspective_mesh(R.KEYSTONE_MILD, True, W, H, W + 7, H - 3, S)[0], S, W + 7, H - 3, what="keystone")
    check(a, C.radial_mesh(-0.15, 0.02, None, None, W, H, S)[0], S, W, H, what="barrel")


@pytest.mark.parametrize("ch", [1, 3])
def test_minification_where_every_tile_goes_direct(ch):
    # 4x: a 64-pixel tile spans 253 source pixels, far beyond the staged box
    a = frame(200, 200, ch)
    for S in (4, 16, 64, 1):
        mesh = R.mesh_of(lambda x, y: (4 * x + 1.5, 4 * y + 0.25), S, 50 + T, 49)
        check(a, mesh, S, 50 + T, 49, borders=BORDERS[1:], what="minify4")


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("S", [4, 8, 32, 64])
def test_both_paths_in_one_launch(ch, S):
    # the left tile column is a translation (its box fits), from x = 64 on the map stretches 3x (it does not)
    a = frame(200, 150, ch)
    fn = lambda x, y: (np.where(x <= 64, x + 2.25, 66.25 + 3 * (x - 64)), y + 0.5 + 0 * x)  # noqa: E731
    mesh = R.mesh_of(fn, S, 2 * T + 5, T + 9)
    # (the statement about the boxes, from the nodes themselves)
    left = mesh[:, :64 // S + 1, 0]
    right = mesh[:, 64 // S:2 * 64 // S + 1, 0]
    assert (left.max() - left.min()) >> 12 < TILE["box"] - 3 and (right.max() - right.min()) >> 12 > TILE["box"]
    check(a, mesh, S, 2 * T + 5, T + 9, what="both paths")


@pytest.mark.parametrize("ch", [1, 3])
def test_mesh_wholly_outside_the_frame(ch):
    a = frame(40, 30, ch)
    for S in (1, 8, 64):
        for dx, dy in ((-500, 0), (500, 0), (0, -500), (0, 500), (4000, 4000), (-262000, 262000)):
            mesh = R.translation_mesh(S, T + 3, T + 2, dx, dy)
            check(a, mesh, S, T + 3, T + 2, what=("outside", dx, dy))
            x = torch.from_numpy(a).cuda()
            got = device_remap(x, torch.from_numpy(mesh).cuda(), S, T + 3, T + 2, "bilinear", "constant", 200)
            assert (got == 200).all()
    # a small source in the middle of 3 x 3 tiles: the corner tiles' boxes miss the frame
    mesh = R.translation_mesh(8, 3 * T - 5, 3 * T - 9, -70, -80)
    check(a, mesh, 8, 3 * T - 5, 3 * T - 9, what="middle")


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("S", R.SPACINGS)
def test_random_meshes(ch, S):
    a = frame(200, 180, ch)
    W2, H2 = 2 * T + 3, T + 1
    check(a, R.random_mesh(S, W2, H2, seed=S + 17, spread=40), S, W2, H2, what="near")
    check(a, R.random_mesh(S, W2, H2, seed=S + 18), S, W2, H2, borders=BORDERS[1:], what="anywhere")
    # the extremes of the node range
    lim = (1 << 30) - 1
    mesh = R.random_mesh(S, W2, H2, seed=S + 19)
    mesh[::2] = lim
    mesh[1::3] = -lim
    check(a, mesh, S, W2, H2, borders=BORDERS[1:], what="extremes")


def device_bytes(n, fill):
    return torch.full((n,), fill, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("off", [1, 7, 15])
def test_unaligned_pitched_views(ch, off):
    stream = torch.cuda.current_stream().cuda_stream
    for (W, H) in ((131, 19), (37, 133), (16, 5), (T + 1, T + 1)):
        a = frame(W, H, ch)
        E = W * ch
        sp = (E + 5) | 1  # odd pitches: every row has its own misalignment
        src = device_bytes(off + sp * H + 64, 0x5A)
        src[off:off + sp * H].view(H, sp)[:, :E] = torch.from_numpy(a.reshape(H, E)).cuda()
        for S, W2, H2, fn in ((8, W + 3, H + 2, lambda x, y: (0.9 * x + 0.3 * y - 2.5, -0.3 * x + 0.9 * y + 4.25)),
                              (1, 2 * W - 3, 2 * H - 1, lambda x, y: (0.5 * x + 0.25, 0.5 * y + 0.75)),
                              (16, W // 3 + 1, H // 3 + 1, lambda x, y: (3 * x + 0.5 * y, -0.5 * x + 3 * y + 1))):
            mesh = R.mesh_of(fn, S, W2, H2)
            # the mesh at an offset of one node (8 bytes) into its buffer
            dmb = torch.zeros(mesh.size + 2, dtype=torch.int32, device="cuda")
            dmb[2:] = torch.from_numpy(mesh.reshape(-1)).cuda()
            E2 = W2 * ch
            dp = (E2 + 13) | 1
            for mode in MODES:
                for border, fill in BORDERS[1:]:
                    ref = C.golden_remap(a, mesh, S, W2, H2, mode, border, fill)
                    dst = device_bytes(off + dp * H2 + 64, 0xA5)
                    C.remap_device(src.data_ptr() + off, sp, W, H, ch, dst.data_ptr() + off, dp, dmb.data_ptr() + 8,
                                   mesh.size, S, W2, H2, mode, border, fill, stream)
                    torch.cuda.synchronize()
                    d = dst.cpu().numpy()
                    body = d[off:off + dp * H2].reshape(H2, dp)
                    assert (body[:, :E2] == ref.reshape(H2, E2)).all(), (W, H, S, W2, H2, mode, border)
                    # the bytes around the destination and its pitch padding are untouched
                    assert (d[:off] == 0xA5).all() and (body[:, E2:] == 0xA5).all() and (d[off + dp * H2:] == 0xA5).all()


@pytest.mark.parametrize("ch", [1, 3])
def test_source_at_the_end_of_its_tensor(ch):
    # the last pixel of the source is the tensor's last byte; the maps read its last rows and columns
    for (W, H) in ((133, 11), (17, 140), (T + 3, 9)):
        a = frame(W, H, ch)
        n = a.size
        big = torch.empty(n + 37, dtype=torch.uint8, device="cuda")
        big[37:] = torch.from_numpy(a.reshape(-1)).cuda()
        x = big[37:].view(a.shape)
        assert x.data_ptr() + n == big.data_ptr() + big.numel()
        for S in (1, 2, 8):
            for fn in (lambda x, y: (x + 0.5, y + 0.5), lambda x, y: (W - 1 - x + 0.25, H - 1 - y + 0.25),
                       lambda x, y: (0.2 * x + W - 20, 0.2 * y + H - 8)):
                mesh = R.mesh_of(fn, S, W, H)
                dm = torch.from_numpy(mesh).cuda()
                for border in ("constant", "replicate"):
                    got = m.ops.mesh_warp(x, dm, S, border=border, fill=3).cpu().numpy()
                    assert (got == m.ops.remap_reference(a, mesh, S, border=border, fill=3)).all(), (S, border)


@pytest.mark.parametrize("nt", ["0", "1"])
def test_both_store_policies(monkeypatch, nt):
    monkeypatch.setenv("STRIPE_NT", nt)
    assert C.launch_policy("remap", cin=3, W=100, rows=100, W2=100, rows2=100, mesh_bytes=800)["nt_stores"] == (nt == "1")
    for ch in (1, 3):
        a = frame(T + 37, T + 5, ch)
        for S in (1, 2, 16):
            check(a, R.rotation_mesh(S, T + 30, T + 9, 30.0, 50, 34), S, T + 30, T + 9, borders=BORDERS[1:])
            check(a, R.mesh_of(lambda x, y: (4 * x, 4 * y), S, 33, 21), S, 33, 21, borders=BORDERS[1:])


def test_second_stream():
    a = frame(200, 160, 3)
    Hinv = np.asarray(R.KEYSTONE_MILD).reshape(3, 3)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.from_numpy(a).cuda()
        y = m.ops.warp_perspective(x, Hinv, size=(150, 190), inverse=True)
        z = m.ops.undistort(y, -0.1, mode="nearest")
    s.synchronize()
    ref = m.ops.warp_perspective(a, Hinv, size=(150, 190), inverse=True)
    assert (y.cpu().numpy() == ref).all()
    assert (z.cpu().numpy() == m.ops.undistort(ref, -0.1, mode="nearest")).all()


def test_front_end_on_tensors():
    a = frame(150, 90, 3)
    x = torch.from_numpy(a).cuda()
    Hinv = np.asarray(R.KEYSTONE_STRONG).reshape(3, 3)
    got = m.ops.warp_perspective(x, Hinv, size=(80, 140), fill=9, inverse=True)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (80, 140, 3)
    assert (got.cpu().numpy() == m.ops.warp_perspective(a, Hinv, size=(80, 140), fill=9, inverse=True)).all()
    g = x[:, :, 1]  # non-contiguous gray view: made contiguous
    assert not g.is_contiguous()
    assert (m.ops.undistort(g, -0.1).cpu().numpy() == m.ops.undistort(np.ascontiguousarray(a[:, :, 1]), -0.1)).all()
    t = x.transpose(0, 1)  # non-contiguous RGB
    assert (m.ops.undistort(t, 0.07).cpu().numpy() == m.ops.undistort(np.ascontiguousarray(a.transpose(1, 0, 2)), 0.07)).all()
    v = x[10:70, 20:101]  # a strided window with packed pixels: read in place
    assert not v.is_contiguous()
    quad = [(3, 2), (70, 6), (75, 55), (1, 50)]
    for border in ("constant", "replicate"):
        assert (m.ops.rectify_quad(v, quad, border=border).cpu().numpy() ==
                m.ops.rectify_quad(np.ascontiguousarray(a[10:70, 20:101]), quad, border=border)).all()
    b = torch.stack([x, 255 - x, x.flip(0)])
    out = m.ops.undistort(b, -0.12, 0.01)
    assert (out.cpu().numpy() == m.ops.undistort(b.cpu().numpy(), -0.12, 0.01)).all()
    assert m.ops.undistort(b[:0], -0.12).shape == (0,) + tuple(out.shape[1:])
    assert m.ops.undistort(x[:, :, :1], -0.1).shape == (90, 150, 1)
    # device maps are quantised on the device, like host maps on the host
    yy, xx = np.mgrid[0:70, 0:120].astype(np.float64)
    map_x, map_y = 1.2 * xx + 3 * np.sin(yy / 5.0) + 0.37, 0.9 * yy + 0.1 * xx - 2.11
    ref = m.ops.remap(a, map_x, map_y, border="replicate")
    got = m.ops.remap(x, torch.from_numpy(map_x).cuda(), torch.from_numpy(map_y).cuda(), border="replicate")
    assert got.is_cuda and (got.cpu().numpy() == ref).all()
    assert (m.ops.remap(x, map_x, map_y, border="replicate").cpu().numpy() == ref).all()  # host maps, device frame
    fx, fy = map_x.astype(np.float32), map_y.astype(np.float32)
    assert (m.ops.remap(x, torch.from_numpy(fx).cuda(), torch.from_numpy(fy).cuda(), mode="nearest").cpu().numpy() ==
            m.ops.remap(a, fx, fy, mode="nearest")).all()
    # a device mesh
    mesh, S = C.perspective_mesh(R.KEYSTONE_MILD, True, 150, 90, 150, 90)
    assert (m.ops.mesh_warp(x, torch.from_numpy(mesh).cuda(), S).cpu().numpy() == m.ops.remap_reference(a, mesh, S)).all()
    with pytest.raises(TypeError, match="uint8"):
        m.ops.undistort(x.float(), 0.1)
    with pytest.raises(ValueError, match=r"beyond 2\^18"):
        m.ops.mesh_warp(x, torch.full((3, 4, 2), 1 << 30, dtype=torch.int32, device="cuda"), 64)
    with pytest.raises(ValueError, match="non-finite"):
        m.ops.remap(x, torch.full((4, 5), float("nan"), device="cuda"), torch.zeros((4, 5), device="cuda"))


def test_launch_checks():
    x = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    mesh = torch.zeros(2 * 2 * 2, dtype=torch.int32, device="cuda")
    p, q = x.data_ptr(), mesh.data_ptr()
    for args, msg in (((p, 63, 64, 64, 1, p, 64, q, 8, 64, 64, 64), "src_pitch 63 < row bytes 64"),
                      ((p, 64, 64, 32, 1, p, 31, q, 8, 64, 32, 64), "dst_pitch 31 < row bytes 32"),
                      ((p, 64, 64, 64, 2, p, 64, q, 8, 64, 64, 64), "1 or 3 channels"),
                      ((p, 64, 64, 64, 1, 0, 64, q, 8, 64, 64, 64), "null src or dst"),
                      ((p, 64, 64, 64, 1, p, 64, 0, 8, 64, 64, 64), "null mesh"),
                      ((p, 64, 0, 64, 1, p, 64, q, 8, 64, 64, 64), r"source size 0x64 outside 1\.\.65535"),
                      ((p, 64, 64, 64, 1, p, 64, q, 8, 64, 64, 65536), r"destination size 64x65536 outside 1\.\.65535"),
                      ((p, 64, 64, 64, 1, p, 64, q, 8, 48, 64, 64), "spacing 48 is not a power of two"),
                      ((p, 64, 64, 64, 1, p, 64, q, 8, 32, 64, 64), r"has shape 3x3x2 \(18 integers\), got 8"),
                      ((p, 64, 64, 64, 1, p, 64, q + 2, 8, 64, 64, 64), "aligned to 4 bytes"),
                      ((p, 64, 64, 64, 1, p, 64, q, 8, 64, 64, 64, "cubic"), "unknown mode 'cubic'"),
                      ((p, 64, 64, 64, 1, p, 64, q, 8, 64, 64, 64, "nearest", "wrap"), "unknown border 'wrap'")):
        with pytest.raises(RuntimeError, match=msg):
            C.remap_device(*args)


@pytest.mark.skipif(not os.path.exists(STRIPE), reason="bin/stripe not built")
def test_cli_device_equals_host(tmp_path):
    a = frame(200, 160, 3)
    src = str(tmp_path / "a.ppm")
    C.write_pnm(src, a)
    spec = "1.05;0.08;-4;0.02;1.1;-3;0.0004;0.0002;1:180x150"
    outs = {}
    for backend in ("local", "host"):
        dst = str(tmp_path / f"{backend}.ppm")
        args = ["run", "--input", src, "--output", dst, "--orient", "fliph", "--perspective", spec, "--warp-border",
                "constant:40", "--resize", "90x75:bilinear", "--chain", "gaussian5"]
        if backend == "host":
            args += ["--backend", "host"]  # (the default is the device backend where a GPU is present)
        r = subprocess.run([STRIPE, *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        j = json.loads(r.stdout.strip().splitlines()[-1])
        assert j["warp"] == "perspective:" + spec and j["warped_from"] == [200, 160] and j["backend"] == backend
        assert (j["W"], j["H"]) == (90, 75)
        outs[backend] = C.read_pnm(dst)
    assert (outs["local"] == outs["host"]).all()
    Hm = C.parse_perspective_spec(spec)[0]
    mesh, S = C.perspective_mesh(Hm, False, 200, 160, 180, 150)
    assert j["mesh_spacing"] == S
    ref = C.golden_remap(C.golden_orient(a, "fliph"), mesh, S, 180, 150, "bilinear", "constant", 40)
    ref = C.golden_resize(ref, 90, 75, "bilinear")
    assert (outs["host"] == C.golden_apply(ref, "gaussian5", "reflect101", True)).all()
