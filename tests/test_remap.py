"""The mesh warp rule on the CPU (csrc/include/stripe/remap.h): golden_remap ==
the numpy mirror == cpu_remap at 1, 2 and 7 threads over every spacing, both
modes, both borders, gray and RGB; the fixed points that follow from the rule;
the builders' accuracy at every pixel and their automatic spacing; the pixel
bounds against float64 sampling at the exact map; scipy's map_coordinates as
the third-party check on `ops.remap`; perspective_from_points; --quad of a
rectangle against the crop; the refusals; the front end; the CLIs on the host
backend."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mpi_cuda_imagemanipulation_amd as m
import np_remap as R

C = m._C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPE = os.path.join(ROOT, "bin", "stripe")
BORDERS = (("constant", 0), ("constant", 200), ("replicate", 0))
MODES = ("bilinear", "nearest")
SIDES = (63, 64, 65, 131)


def frame(W, H, ch):
    shape = (H, W) if ch == 1 else (H, W, ch)
    return np.random.default_rng(W * 7919 + H * 31 + ch).integers(0, 256, shape, dtype=np.uint8)


def all_layers(a, mesh, S, W2, H2, modes=MODES, borders=BORDERS, what=None):
    for mode in modes:
        for border, fill in borders:
            g = C.golden_remap(a, mesh, S, W2, H2, mode, border, fill)
            assert g.shape[:2] == (H2, W2)
            assert (g == R.np_remap(a, mesh, S, W2, H2, mode, border, fill)).all(), (what, S, W2, H2, mode, border)
            for threads in (1, 2, 7):
                assert (g == C.cpu_remap(a, mesh, S, W2, H2, mode, border, fill, threads)).all(), (what, S, mode, border)


def shapes():
    """Destination sizes: each side in SIDES on one axis at least, a 1 x 1 destination."""
    return [(63, 65), (64, 64), (65, 63), (131, 9), (9, 131), (1, 1)]


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("S", R.SPACINGS)
def test_golden_mirror_and_host_executor_agree(ch, S):
    a = frame(90, 70, ch)
    for W2, H2 in shapes():
        all_layers(a, R.random_mesh(S, W2, H2, seed=S * 1000 + W2, spread=40), S, W2, H2, what="near")
    W2, H2 = 65, 63
    all_layers(a, R.rotation_mesh(S, W2, H2, 30.0, 44.5, 34.5), S, W2, H2, what="rot30")
    all_layers(a, R.random_mesh(S, W2, H2, seed=S), S, W2, H2, what="anywhere")
    # a 1 x 1 source
    one = frame(1, 1, ch)
    all_layers(one, R.random_mesh(S, 9, 7, seed=3, spread=2), S, 9, 7, what="1x1 source")
    all_layers(one, R.identity_mesh(S, 1, 1), S, 1, 1, what="1x1 both")
    assert (C.golden_remap(one, R.identity_mesh(S, 1, 1), S, 1, 1) == one).all()


def test_host_executor_threads_on_a_frame_large_enough_to_split():
    a = frame(300, 290, 3)
    mesh, S = C.perspective_mesh(R.KEYSTONE_MILD, True, 300, 290, 310, 280)
    for mode in MODES:
        g = C.golden_remap(a, mesh, S, 310, 280, mode, "constant", 7)
        for threads in (1, 2, 7):
            assert (g == C.cpu_remap(a, mesh, S, 310, 280, mode, "constant", 7, threads)).all()


@pytest.mark.parametrize("ch", [1, 3])
def test_fixed_points(ch):
    a = frame(131, 65, ch)
    W, H = 131, 65
    for S in R.SPACINGS:
        # the identity mesh is the identity at every spacing
        for mode in MODES:
            for border, fill in BORDERS:
                assert (C.golden_remap(a, R.identity_mesh(S, W, H), S, W, H, mode, border, fill) == a).all(), (S, mode)
        # integer translations are exact: out(x, y) = in(x + 3, y - 5), the fill outside
        for mode in MODES:
            g = C.golden_remap(a, R.translation_mesh(S, W, H, 3, -5), S, W, H, mode, "constant", 77)
            ref = np.full_like(a, 77)
            ref[5:, :W - 3] = a[:H - 5, 3:]
            assert (g == ref).all(), (S, mode)
        # flat images are fixed points under replicate, whatever the mesh
        flat = np.full_like(a, 93)
        for mode in MODES:
            assert (C.golden_remap(flat, R.random_mesh(S, 70, 67, seed=S), S, 70, 67, mode, "replicate", 0) == 93).all()
    # at S = 1 nothing is interpolated: every pixel depends on its own node only
    mesh = R.random_mesh(1, 40, 30, seed=9, spread=20)
    g = C.golden_remap(a, mesh, 1, 40, 30)
    other = mesh.copy()
    other[7, 11] = (5 * 4096 + 100, 9 * 4096 + 3000)
    g2 = C.golden_remap(a, other, 1, 40, 30)
    diff = np.argwhere((g != g2).reshape(30, 40, -1).any(axis=2))
    assert len(diff) <= 1 and all(tuple(d) == (7, 11) for d in diff)
    # and the last row and column of the mesh are never read
    other = mesh.copy()
    other[-1, :] = 12345
    other[:, -1] = -54321
    assert (C.golden_remap(a, other, 1, 40, 30) == g).all()


PERSPECTIVES = (("mild", R.KEYSTONE_MILD, lambda S: S > 1), ("strong", R.KEYSTONE_STRONG, lambda S: S <= 4),
                ("affine", R.AFFINE_H, lambda S: S == 64))


@pytest.mark.parametrize("name,Hinv,spacing_ok", PERSPECTIVES, ids=[p[0] for p in PERSPECTIVES])
def test_perspective_builder_accuracy_and_pixels(name, Hinv, spacing_ok):
    W, H, W2, H2 = 90, 70, 131, 65
    mesh, S = C.perspective_mesh(Hinv, True, W, H, W2, H2)
    assert spacing_ok(S), (name, S)
    assert mesh.shape == (R.grid(H2, S), R.grid(W2, S), 2) and mesh.dtype == np.int32
    sx, sy = R.mesh_positions(mesh, S, W2, H2)
    ex, ey = R.perspective_positions(Hinv, W2, H2)
    assert np.abs(sx - ex).max() <= R.POSITION_BOUND and np.abs(sy - ey).max() <= R.POSITION_BOUND, (name, S)
    # the forward matrix gives the same mesh as its inverse, up to the node rounding of a double inversion
    fwd = np.linalg.inv(np.asarray(Hinv).reshape(3, 3)).reshape(-1)
    mesh2, S2 = C.perspective_mesh(list(fwd), False, W, H, W2, H2, S)
    assert S2 == S and np.abs(mesh2.astype(np.int64) - mesh).max() <= 1
    # a scaled or negated matrix is the same map
    mesh3, _ = C.perspective_mesh([-3.0 * v for v in Hinv], True, W, H, W2, H2, S)
    assert np.abs(mesh3.astype(np.int64) - mesh).max() <= 1
    for ch in (1, 3):
        a = frame(W, H, ch)
        for border, fill in BORDERS:
            g = C.golden_remap(a, mesh, S, W2, H2, "bilinear", border, fill)
            err = np.abs(g.astype(np.float64) - R.float_sample(a, ex, ey, border, fill)).max()
            assert err <= R.bound(S), (name, border, err)
    # every explicit spacing is honoured; the rule's own bound holds for those at or below the automatic one
    for S1 in R.SPACINGS:
        me, s1 = C.perspective_mesh(Hinv, True, W, H, W2, H2, S1)
        assert s1 == S1
        if S1 <= S:
            px, py = R.mesh_positions(me, S1, W2, H2)
            assert max(np.abs(px - ex).max(), np.abs(py - ey).max()) <= R.POSITION_BOUND


@pytest.mark.parametrize("name,k1,k2", [("barrel", -0.12, 0.01), ("pincushion", 0.08, 0.0), ("slight", -2e-3, 0.0)])
def test_radial_builder_accuracy_and_pixels(name, k1, k2):
    W, H = 131, 65
    mesh, S = C.radial_mesh(k1, k2, None, None, W, H)
    if name == "slight":
        assert S > 1
    f, cx, cy = 0.5 * np.hypot(W, H), (W - 1) / 2, (H - 1) / 2
    ex, ey = R.radial_positions(k1, k2, f, cx, cy, W, H)
    sx, sy = R.mesh_positions(mesh, S, W, H)
    assert np.abs(sx - ex).max() <= R.POSITION_BOUND and np.abs(sy - ey).max() <= R.POSITION_BOUND, (name, S)
    a = frame(W, H, 3)
    for border, fill in BORDERS:
        g = C.golden_remap(a, mesh, S, W, H, "bilinear", border, fill)
        err = np.abs(g.astype(np.float64) - R.float_sample(a, ex, ey, border, fill)).max()
        assert err <= R.bound(S), (name, border, err)
    # explicit f and centre
    mesh2, S2 = C.radial_mesh(k1, k2, 80.0, (60.25, 30.5), W, H)
    ex, ey = R.radial_positions(k1, k2, 80.0, 60.25, 30.5, W, H)
    sx, sy = R.mesh_positions(mesh2, S2, W, H)
    assert np.abs(sx - ex).max() <= R.POSITION_BOUND and np.abs(sy - ey).max() <= R.POSITION_BOUND
    # k1 = k2 = 0 is the identity at spacing 64
    mesh0, S0 = C.radial_mesh(0.0, 0.0, None, None, W, H)
    assert S0 == 64 and (mesh0 == R.identity_mesh(64, W, H)).all()


def test_remap_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    W, H, W2, H2 = 90, 70, 77, 66
    a = frame(W, H, 3)
    yy, xx = np.mgrid[0:H2, 0:W2].astype(np.float64)
    map_x = 1.1 * xx - 0.2 * yy + 3.0 + 4.0 * np.sin(yy / 9.0) + rng.uniform(-0.5, 0.5, xx.shape)
    map_y = 0.15 * xx + 0.95 * yy - 6.0 + 3.0 * np.cos(xx / 7.0)
    for border, smode in (("constant", "grid-constant"), ("replicate", "nearest")):
        got = m.ops.remap(a, map_x, map_y, border=border, fill=50)
        assert got.shape == (H2, W2, 3) and got.dtype == np.uint8
        ref = np.stack([ndi.map_coordinates(a[:, :, c].astype(np.float64), [map_y, map_x], order=1, mode=smode, cval=50.0)
                        for c in range(3)], axis=2)
        err = np.abs(got.astype(np.float64) - ref).max()
        assert err <= R.bound(1), (border, err)
    # float32 maps are taken as they are; nearest picks the rounded position
    got = m.ops.remap(a[:, :, 0], np.rint(map_x).astype(np.float32), np.rint(map_y).astype(np.float32), mode="nearest",
                      border="replicate")
    ix, iy = np.clip(np.rint(map_x).astype(int), 0, W - 1), np.clip(np.rint(map_y).astype(int), 0, H - 1)
    assert (got == a[iy, ix, 0]).all()


def test_perspective_from_points():
    src = [(10.5, 20.25), (80.0, 25.0), (85.75, 60.0), (5.0, 66.5)]
    dst = [(0.0, 0.0), (99.0, 3.0), (97.0, 49.0), (-2.0, 51.0)]
    Hm = m.ops.perspective_from_points(src, dst)
    assert Hm.shape == (3, 3) and Hm[2, 2] == 1.0
    for (x, y), (u, v) in zip(src, dst):
        p = Hm @ np.array([x, y, 1.0])
        scale = max(1.0, abs(u), abs(v))
        assert abs(p[0] / p[2] - u) <= 1e-9 * scale and abs(p[1] / p[2] - v) <= 1e-9 * scale
    # a pure affine set gives an affine matrix
    Hm = m.ops.perspective_from_points([(0, 0), (1, 0), (1, 1), (0, 1)], [(3, 4), (5, 4), (5, 7), (3, 7)])
    assert np.allclose(Hm, [[2, 0, 3], [0, 3, 4], [0, 0, 1]], atol=1e-12)


@pytest.mark.parametrize("ch", [1, 3])
def test_quad_of_a_rectangle_is_the_crop(ch):
    a = frame(90, 70, ch)
    out = m.ops.rectify_quad(a, [(10, 5), (40, 5), (40, 30), (10, 30)])
    assert (out == a[5:31, 10:41]).all()
    assert (out == m.ops.crop(a, 10, 5, 31, 26)).all()
    pts, W2, H2 = C.parse_quad_spec("10,5;40,5;40,30;10,30")
    assert (W2, H2) == (31, 26) and pts == [10, 5, 40, 5, 40, 30, 10, 30]
    assert C.parse_quad_spec("0,0;9.6,0;9,4.4;0,5:20x10")[1:] == (20, 10)
    assert C.parse_quad_spec("0,0;9.6,0;9,4.4;0,5")[1:] == (11, 6)  # rint(9.6) + 1, rint(5) + 1
    # with a size the rectangle is scaled onto the corners
    out = m.ops.rectify_quad(a, [(10, 5), (40, 5), (40, 30), (10, 30)], size=(51, 61))
    assert out.shape[:2] == (51, 61) and (out[::2, ::2] == a[5:31, 10:41]).all()


REFUSALS = [
    (lambda: C.perspective_mesh([1, 0, 0, 0, 1, 0, 0, 0, float("nan")], True, 9, 9, 9, 9), "non-finite number"),
    (lambda: C.perspective_mesh([1, 2, 3, 2, 4, 6, 0, 0, 1], False, 9, 9, 9, 9, 0, "tok"), r"remap 'tok': singular matrix"),
    (lambda: C.perspective_mesh([1, 0, 0, 0, 1, 0, -0.05, 0, 1], True, 90, 70, 90, 70, 0, "hz"),
     r"remap 'hz': the horizon crosses the destination"),
    (lambda: C.perspective_mesh([1, 0, 0, 0, 1, 0, -0.05, 0, 1], True, 90, 70, 90, 70, 64), "the horizon crosses the destination"),
    (lambda: C.perspective_mesh([1, 0, 3e5, 0, 1, 0, 0, 0, 1], True, 9, 9, 9, 9, 0, "far"),
     r"remap 'far': a node at .* lies at or beyond 2\^18 pixels"),
    (lambda: C.perspective_mesh(R.AFFINE_H, True, 9, 9, 0 + 65536, 9), r"destination size 65536x9 outside 1\.\.65535"),
    (lambda: C.perspective_mesh(R.AFFINE_H, True, 0, 9, 9, 9), r"source size 0x9 outside 1\.\.65535"),
    (lambda: C.perspective_mesh(R.AFFINE_H, True, 9, 9, 9, 9, 3, "sp"), r"remap 'sp': spacing 3 is not a power of two in 1\.\.64"),
    (lambda: C.perspective_mesh(R.AFFINE_H, True, 9, 9, 9, 9, 128), "spacing 128 is not a power of two"),
    (lambda: C.perspective_mesh([1, 0, 0, 0, 1, 0], True, 9, 9, 9, 9), "nine numbers"),
    (lambda: C.radial_mesh(0.1, 0.0, 0.0, None, 9, 9), "the focal length must be positive"),
    (lambda: C.radial_mesh(0.1, 0.0, -5.0, None, 9, 9, 0, "u"), r"remap 'u': the focal length must be positive"),
    (lambda: C.radial_mesh(float("inf"), 0.0, None, None, 9, 9), "non-finite number"),
    (lambda: C.radial_mesh(1e9, 0.0, 1.0, None, 99, 99), r"lies at or beyond 2\^18 pixels"),
    (lambda: C.perspective_from_points([0, 0, 1, 1, 2, 2, 0, 5], [0, 0, 9, 0, 9, 9, 0, 9]), "degenerate point set"),
    (lambda: C.perspective_from_points([0, 0, 1, 0, 1, 0, 0, 5], [0, 0, 9, 0, 9, 9, 0, 9]), "degenerate point set"),
    (lambda: C.perspective_from_points([0, 0, 1, 0, 1, 1, 0, float("nan")], [0, 0, 9, 0, 9, 9, 0, 9]), "non-finite number"),
    (lambda: C.parse_quad_spec("0,0;1,0;1,1"), r"quad spec '0,0;1,0;1,1': expected four points"),
    (lambda: C.parse_quad_spec("0,0;1,0;1,1;0,inf"), "non-finite number"),
    (lambda: C.parse_quad_spec("0,0;1,0;1,1;0,1:0x5"), r"destination size outside 1\.\.65535"),
    (lambda: C.parse_quad_spec("0,0;1e6,0;1e6,1;0,1"), r"outside 1\.\.65535"),
    (lambda: C.parse_perspective_spec("1;0;0;0;1;0;0;0"), "expected nine numbers"),
    (lambda: C.parse_perspective_spec("1;0;0;0;1;0;0;0;nan"), "non-finite number"),
    (lambda: C.parse_undistort_spec(""), "expected k1"),
    (lambda: C.parse_undistort_spec("0.1;0;100;5"), "expected k1"),
    (lambda: C.golden_remap(np.zeros((9, 9), np.uint8), np.zeros((3, 4, 2), np.int32), 8, 9, 9), "has shape 3x3x2"),
    (lambda: C.golden_remap(np.zeros((9, 9), np.uint8), np.zeros((3, 3, 2), np.int32), 5, 9, 9), "spacing 5 is not a power of two"),
    (lambda: C.golden_remap(np.zeros((9, 9), np.uint8), np.zeros((3, 3, 2), np.int64), 8, 9, 9), "must be an int32 array"),
    (lambda: C.golden_remap(np.zeros((9, 9), np.uint8), np.full((3, 3, 2), 1 << 30, np.int32), 8, 9, 9),
     r"lies at or beyond 2\^18 pixels"),
    (lambda: C.cpu_remap(np.zeros((9, 9), np.uint8), np.full((3, 3, 2), -(1 << 30), np.int32), 8, 9, 9),
     r"lies at or beyond 2\^18 pixels"),
    (lambda: C.cpu_remap(np.zeros((9, 9, 3), np.uint8), np.zeros((10, 10, 2), np.int32), 1, 9, 9, "cubic"), "unknown mode 'cubic'"),
    (lambda: C.cpu_remap(np.zeros((9, 9, 3), np.uint8), np.zeros((10, 10, 2), np.int32), 1, 9, 9, "nearest", "wrap"),
     "unknown border 'wrap'"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals(i):
    fn, msg = REFUSALS[i]
    with pytest.raises(RuntimeError, match=msg):
        fn()


def test_front_end_on_arrays():
    a = frame(90, 70, 3)
    Hinv = np.asarray(R.KEYSTONE_MILD).reshape(3, 3)
    mesh, S = C.perspective_mesh(R.KEYSTONE_MILD, True, 90, 70, 100, 60)
    ref = C.golden_remap(a, mesh, S, 100, 60, "bilinear", "constant", 9)
    got = m.ops.warp_perspective(a, Hinv, size=(60, 100), fill=9, inverse=True)
    assert got.dtype == np.uint8 and (got == ref).all()
    assert (m.ops.mesh_warp(a, mesh, S, size=(60, 100), fill=9) == ref).all()
    assert (m.ops.remap_reference(a, mesh, S, size=(60, 100), fill=9) == ref).all()
    fwd = np.linalg.inv(Hinv)
    assert np.abs(m.ops.warp_perspective(a, fwd, size=(60, 100), fill=9).astype(int) - ref).max() <= 2
    # an affine homography equals warp_affine's float64 reference within both rules' bounds
    g = m.ops.warp_perspective(a, [[1, 0, 3], [0, 1, -5], [0, 0, 1]])
    assert (g == m.ops.warp_affine(a, [[1, 0, 3], [0, 1, -5]])).all()
    # gray H x W x 1, batches, an empty batch, tensors on the CPU
    assert m.ops.undistort(a[:, :, :1], -0.1).shape == (70, 90, 1)
    b = np.stack([a, 255 - a])
    out = m.ops.undistort(b, -0.1, border="replicate")
    assert out.shape == b.shape and (out[1] == m.ops.undistort(255 - a, -0.1, border="replicate")).all()
    assert m.ops.warp_perspective(b[:0], fwd, size=(60, 100)).shape == (0, 60, 100, 3)
    torch = pytest.importorskip("torch")
    t = m.ops.warp_perspective(torch.from_numpy(a), Hinv, size=(60, 100), fill=9, inverse=True)
    assert isinstance(t, torch.Tensor) and (t.numpy() == ref).all()
    tm = m.ops.remap(torch.from_numpy(a), torch.full((5, 6), 2.5), torch.full((5, 6), 3.0, dtype=torch.float64))
    assert (tm.numpy() == m.ops.remap(a, np.full((5, 6), 2.5), np.full((5, 6), 3.0))).all()
    # undistort's defaults and explicit values
    meshu, Su = C.radial_mesh(-0.1, 0.02, None, None, 90, 70)
    assert (m.ops.undistort(a, -0.1, 0.02) == C.golden_remap(a, meshu, Su, 90, 70)).all()
    meshu, Su = C.radial_mesh(-0.1, 0.0, 50.0, (40.0, 30.0), 90, 70)
    assert (m.ops.undistort(a, -0.1, f=50, center=(40, 30)) == C.golden_remap(a, meshu, Su, 90, 70)).all()
    for name in ("warp_perspective", "perspective_from_points", "rectify_quad", "undistort", "remap", "mesh_warp",
                 "remap_reference"):
        assert name in m.ops.__all__ and callable(getattr(m.ops, name))
    for fn, exc, msg in (
            (lambda: m.ops.warp_perspective(a, [[1, 2, 3], [2, 4, 6], [0, 0, 1]]), ValueError, "singular"),
            (lambda: m.ops.warp_perspective(a, [[1, 0, 0], [0, 1, 0], [-0.05, 0, 1]], inverse=True), ValueError, "horizon"),
            (lambda: m.ops.warp_perspective(a, [[1, 0], [0, 1]]), ValueError, "3x3"),
            (lambda: m.ops.warp_perspective(a, fwd, mode="cubic"), ValueError, "unknown mode"),
            (lambda: m.ops.warp_perspective(a, fwd, size=(0, 5)), ValueError, r"outside 1\.\.65535"),
            (lambda: m.ops.mesh_warp(a, mesh, 3, size=(60, 100)), ValueError, "power of two"),
            (lambda: m.ops.undistort(a, 0.1, f=0), ValueError, "focal length"),
            (lambda: m.ops.mesh_warp(a, mesh, 4, size=(60, 100)), ValueError, "has shape"),
            (lambda: m.ops.mesh_warp(a, mesh.astype(np.int64), S, size=(60, 100)), TypeError, "int32"),
            (lambda: m.ops.mesh_warp(a, np.full_like(mesh, 1 << 30), S, size=(60, 100)), ValueError, r"beyond 2\^18"),
            (lambda: m.ops.remap(a, np.zeros((4, 5)), np.zeros((5, 4))), ValueError, "two H2 x W2 maps"),
            (lambda: m.ops.remap(a, np.zeros((4, 5), np.int32), np.zeros((4, 5))), TypeError, "floating point"),
            (lambda: m.ops.remap(a, np.full((4, 5), np.nan), np.zeros((4, 5))), ValueError, "non-finite"),
            (lambda: m.ops.remap(a, np.full((4, 5), 3e5), np.zeros((4, 5))), ValueError, r"beyond 2\^18"),
            (lambda: m.ops.rectify_quad(a, [(0, 0), (1, 1), (2, 2), (3, 3)]), ValueError, "degenerate"),
            (lambda: m.ops.warp_perspective(a.astype(np.float32), fwd), TypeError, "uint8")):
        with pytest.raises(exc, match=msg):
            fn()


def run_cli(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


KEYSTONE_FWD = "1.05;0.08;-4;0.02;1.1;-3;0.0004;0.0002;1"


@pytest.mark.skipif(not os.path.exists(STRIPE), reason="bin/stripe not built")
def test_cli_on_the_host_backend(tmp_path):
    a = frame(120, 80, 3)
    src, dst = str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm")
    C.write_pnm(src, a)
    base = [STRIPE, "run", "--input", src, "--output", dst, "--backend", "host", "--chain", "invert"]
    # --perspective, with mode and border, in front of --resize
    r = run_cli(base + ["--perspective", KEYSTONE_FWD + ":100x90", "--warp-border", "constant:40", "--resize", "50x45:area"])
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    Hm, W2, H2 = C.parse_perspective_spec(KEYSTONE_FWD + ":100x90")
    assert j["warped_from"] == [120, 80] and j["warp"] == "perspective:" + KEYSTONE_FWD + ":100x90"
    assert (j["W"], j["H"]) == (50, 45)
    mesh, S = C.perspective_mesh(Hm, False, 120, 80, 100, 90)
    assert j["mesh_spacing"] == S
    ref = C.golden_resize(C.golden_remap(a, mesh, S, 100, 90, "bilinear", "constant", 40), 50, 45, "area")
    assert (C.read_pnm(dst) == 255 - ref).all()
    # --quad of an axis-aligned rectangle is the crop, bit for bit (after --orient)
    r = run_cli(base + ["--orient", "fliph", "--quad", "10,5;40,5;40,30;10,30"])
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["warp"] == "quad:10,5;40,5;40,30;10,30:31x26" and j["mesh_spacing"] == 64
    assert (C.read_pnm(dst) == 255 - a[:, ::-1][5:31, 10:41]).all()
    # --undistort with nearest and replicate; the token carries the resolved defaults
    r = run_cli(base + ["--undistort", "-0.1;0.01", "--warp-mode", "nearest", "--warp-border", "replicate"])
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["warp"] == C.undistort_token("-0.1;0.01", 120, 80) and j["warp"].startswith("undistort:-0.1;0.01;")
    assert j["warp"].endswith(";59.5;39.5") and j["warped_from"] == [120, 80]
    mesh, S = C.radial_mesh(-0.1, 0.01, None, None, 120, 80)
    assert j["mesh_spacing"] == S
    assert (C.read_pnm(dst) == 255 - C.golden_remap(a, mesh, S, 120, 80, "nearest", "replicate", 0)).all()
    # --held gets the same map
    held = str(tmp_path / "h.ppm")
    C.write_pnm(held, 255 - a)
    r = run_cli([STRIPE, "run", "--input", src, "--held", held, "--output", dst, "--backend", "host", "--chain", "add",
                 "--undistort", "0.05", "--warp-border", "replicate"])
    assert r.returncode == 0, r.stderr
    assert (C.read_pnm(dst) == 255).all()
    # convert takes the flags too
    r = run_cli([STRIPE, "convert", "--input", src, "--output", dst, "--backend", "host", "--quad", "10,5;40,5;40,30;10,30"])
    assert r.returncode == 0, r.stderr
    assert (C.read_pnm(dst) == a[5:31, 10:41]).all()
    # without the flags nothing changes
    r = run_cli(base)
    assert r.returncode == 0 and "warp" not in r.stdout and "mesh_spacing" not in r.stdout
    for extra, msg in ((["--rotate", "3", "--perspective", KEYSTONE_FWD], "mutually exclusive"),
                       (["--quad", "0,0;9,0;9,9;0,9", "--undistort", "0.1"], "mutually exclusive"),
                       (["--warp", "1;0;0;0;1;0", "--undistort", "0.1"], "mutually exclusive"),
                       (["--perspective", KEYSTONE_FWD, "--quad", "0,0;9,0;9,9;0,9"], "mutually exclusive"),
                       (["--warp-mode", "nearest"], "need --rotate or --warp"),
                       (["--perspective", "1;2;3;2;4;6;0;0;1"], "remap '1;2;3;2;4;6;0;0;1': singular matrix"),
                       (["--perspective", "1;0;0;0;1;0;0.05;0;-1"], "the horizon crosses the destination"),
                       (["--quad", "0,0;5,5;9,9;2,2"], "degenerate point set"),
                       (["--undistort", "0.1;0;0"], "the focal length must be positive"),
                       (["--undistort", "0.1;0;x"], "undistort spec '0.1;0;x'")):
        r = run_cli(base + extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)


def test_python_cli_on_the_host_backend(tmp_path):
    a = frame(64, 48, 3)
    src, dst = str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm")
    C.write_pnm(src, a)
    base = [sys.executable, "-m", "mpi_cuda_imagemanipulation_amd", "run", "--input", src, "--output", dst, "--backend",
            "host", "--chain", "invert"]
    r = run_cli(base + ["--undistort=-0.08", "--warp-border", "replicate"])
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    mesh, S = C.radial_mesh(-0.08, 0.0, None, None, 64, 48)
    assert j["warped_from"] == [64, 48] and j["warp"] == C.undistort_token("-0.08", 64, 48) and j["mesh_spacing"] == S
    assert (C.read_pnm(dst) == 255 - C.golden_remap(a, mesh, S, 64, 48, "bilinear", "replicate", 0)).all()
    r = run_cli(base + ["--perspective", KEYSTONE_FWD + ":50x40"])
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    Hm = C.parse_perspective_spec(KEYSTONE_FWD)[0]
    mesh, S = C.perspective_mesh(Hm, False, 64, 48, 50, 40)
    assert j["warp"] == "perspective:" + KEYSTONE_FWD + ":50x40" and j["mesh_spacing"] == S
    assert (C.read_pnm(dst) == 255 - C.golden_remap(a, mesh, S, 50, 40)).all()
    r = run_cli(base + ["--quad", "10,5;40,5;40,30;10,30"])
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["warp"] == "quad:10,5;40,5;40,30;10,30:31x26"
    assert (C.read_pnm(dst) == 255 - a[5:31, 10:41]).all()
    r = run_cli(base + ["--quad", "10,5;40,5;40,30;10,30", "--rotate", "3"])
    assert r.returncode != 0 and "not allowed with" in r.stderr
    r = run_cli(base + ["--warp-border", "replicate"])
    assert r.returncode != 0 and "need --rotate or --warp" in r.stderr
