"""Distance transform on the host: the golden two-step definition against the
literal minimum over all site pixels and against scipy's
distance_transform_edt (in integers), the threaded executor against the golden
plane, the derived forms (u8, float, masks) against their numpy definitions,
disc morphology against scipy's binary erosion / dilation with the explicit
disc, the ops front end, its refusals and the `stripe distance` subcommand.
All comparisons are exact."""
import os
import subprocess

import numpy as np
import pytest

import distance_cases as D
import mpi_cuda_imagemanipulation_amd as m

C = m._C
ops = m.ops
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPE = os.path.join(ROOT, "bin", "stripe")
THREADS = (1, 2, 3, 7)
# test_components.py's shapes plus a short and a narrow frame
SHAPES = ((1, 1), (1, 37), (37, 1), (7, 9), (21, 23), (39, 35), (3, 70), (70, 3))
RADII = (0, 1, 1.5, 2, 3.7, 10)
BIG = (1000, 1049)


def all_cases():
    for H, W in SHAPES:
        for name, a in D.cases(H, W):
            yield f"{H}x{W}-{name}", a


CASES = list(all_cases())


@pytest.fixture(scope="module")
def golden():
    return {(name, to): C.golden_distance(a, to == "foreground") for name, a in CASES for to in D.TOS}


def test_constants():
    assert C.DISTANCE_NONE == D.NONE == ops.DISTANCE_NONE and C.DISTANCE_MAX_SIDE == 32767
    assert 2 * (C.DISTANCE_MAX_SIDE - 1) ** 2 < C.DISTANCE_NONE


def test_golden_equals_brute_force(golden):
    for name, a in CASES:
        for to in D.TOS:
            got = golden[(name, to)]
            assert got.dtype == np.int32 and got.shape == a.shape
            assert (got == D.brute_d2(a, to)).all(), (name, to)


def test_golden_equals_scipy(golden):
    pytest.importorskip("scipy")
    checked = 0
    for name, a in CASES:
        for to in D.TOS:
            if not D.has_site(a, to):
                continue
            assert (golden[(name, to)] == D.scipy_d2(a, to)).all(), (name, to)
            checked += 1
    assert checked > len(CASES)


def test_frames_without_a_site_are_none(golden):
    seen = 0
    for name, a in CASES:
        for to in D.TOS:
            if not D.has_site(a, to):
                assert (golden[(name, to)] == C.DISTANCE_NONE).all(), (name, to)
                seen += 1
    assert seen >= 2 * len(SHAPES)


def test_known_values():
    a = np.full((5, 7), 255, np.uint8)
    a[1, 2] = 0
    yy, xx = np.mgrid[0:5, 0:7]
    assert (C.golden_distance(a) == (yy - 1) ** 2 + (xx - 2) ** 2).all()
    assert (C.golden_distance(a, True) == (a == 0)).all()  # every pixel but the hole is a site; the hole is 1 away
    assert C.golden_distance(np.array([[0, 9, 9, 9, 0]], np.uint8)).tolist() == [[0, 1, 4, 1, 0]]


@pytest.mark.parametrize("threads", THREADS)
def test_cpu_distance_equals_golden(golden, threads):
    for name, a in CASES:
        for to in D.TOS:
            got = C.cpu_distance(a, to == "foreground", threads)
            assert got.dtype == np.int32 and (got == golden[(name, to)]).all(), (name, to, threads)


@pytest.mark.parametrize("name", ("hole_tl", "disc", "sparse", "random0.5"))
def test_cpu_distance_equals_scipy_on_a_million_pixels(name):
    pytest.importorskip("scipy")
    a = dict(D.cases(*BIG))[name]
    for to in D.TOS:
        assert (C.cpu_distance(a, to == "foreground") == D.scipy_d2(a, to)).all(), (name, to)


def test_derived_forms(golden):
    for name, a in CASES:
        for to in D.TOS:
            d2, fg = golden[(name, to)], to == "foreground"
            u8 = D.numpy_u8(d2)
            assert (C.golden_distance_u8(a, fg) == u8).all() and (C.cpu_distance_u8(a, fg, 3) == u8).all(), (name, to)
            assert (ops.distance_transform(a, to, "u8") == u8).all(), (name, to)
            f = ops.distance_transform(a, to, "float")
            ref = D.numpy_float(d2)
            assert f.dtype == np.float32 and f.tobytes() == ref.tobytes(), (name, to)
            assert ops.distance_transform_reference(a, to, "float").tobytes() == ref.tobytes()
            for t in (0, 2, 50):
                for above in (True, False):
                    want = D.numpy_mask(d2, t, above)
                    assert (C.golden_distance_mask(a, fg, t, above) == want).all(), (name, to, t, above)
                    assert (C.cpu_distance_mask(a, fg, t, above, 2) == want).all(), (name, to, t, above)
    # the exact integer root at the squares and either side of them, and the clamp
    d2 = np.array([[0, 1, 2, 3, 4, 8, 9, 10, 15, 16, 17, 254 ** 2 - 1, 254 ** 2, 255 ** 2 - 1, 255 ** 2, 10 ** 9, D.NONE]], np.int32)
    assert D.numpy_u8(d2).tolist() == [[0, 1, 1, 1, 2, 2, 3, 3, 3, 4, 4, 253, 254, 254, 255, 255, 255]]
    row = np.full((1, 300), 255, np.uint8)
    row[0, 0] = 0
    assert ops.distance_transform(row, output="u8")[0].tolist() == [min(x, 255) for x in range(300)]


def test_disk_erode_and_dilate_equal_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, a in CASES:
        for r in RADII:
            se = D.disc(r)
            want_e = ndimage.binary_erosion(a != 0, structure=se, border_value=1)
            want_d = ndimage.binary_dilation(a != 0, structure=se)
            for fn in (C.golden_disk_morph, C.cpu_disk_morph):
                assert (fn(a, "erode", r) == want_e * 255).all(), (name, r, fn.__name__)
                assert (fn(a, "dilate", r) == want_d * 255).all(), (name, r, fn.__name__)


def test_disk_open_close_are_compositions_and_r1_is_the_cross():
    ndimage = pytest.importorskip("scipy.ndimage")
    cross = ndimage.generate_binary_structure(2, 1)
    for name, a in CASES:
        for r in RADII:
            for fn in (C.golden_disk_morph, C.cpu_disk_morph):
                assert (fn(a, "open", r) == fn(fn(a, "erode", r), "dilate", r)).all(), (name, r)
                assert (fn(a, "close", r) == fn(fn(a, "dilate", r), "erode", r)).all(), (name, r)
        assert (C.golden_disk_morph(a, "erode", 1) == ndimage.binary_erosion(a != 0, cross, border_value=1) * 255).all()
        assert (ops.erode_disk(a, 0) == (a != 0) * 255).all() and (ops.dilate_disk(a, 0) == (a != 0) * 255).all()
        assert (ops.open_disk(a, 0) == (a != 0) * 255).all() and (ops.close_disk(a, 0) == (a != 0) * 255).all()


def test_ops_containers_and_shapes():
    torch = pytest.importorskip("torch")
    a = D.K.random_mask(21, 23, 0.7, 5, value=128)
    ref = C.golden_distance(a)
    d = ops.distance_transform(a)
    assert isinstance(d, np.ndarray) and d.dtype == np.int32 and (d == ref).all()
    d = ops.distance_transform(torch.from_numpy(a), to="foreground")
    assert isinstance(d, torch.Tensor) and d.dtype == torch.int32 and (d.numpy() == C.golden_distance(a, True)).all()
    d = ops.distance_transform(a[:, :, None], output="u8")
    assert d.shape == a.shape and d.dtype == np.uint8 and (d == D.numpy_u8(ref)).all()
    f = ops.distance_transform(torch.from_numpy(a), output="float")
    assert isinstance(f, torch.Tensor) and f.dtype == torch.float32 and (f.numpy() == D.numpy_float(ref)).all()
    assert (ops.distance_transform_reference(a) == ref).all()
    assert (ops.distance_transform_reference(torch.from_numpy(a), "foreground", "u8") == C.golden_distance_u8(a, True)).all()
    z = np.zeros((3, 4), np.uint8)
    assert np.isinf(ops.distance_transform(z, "foreground", "float")).all()
    assert (ops.distance_transform(z, "foreground") == ops.DISTANCE_NONE).all()
    assert (ops.distance_transform(z, "foreground", "u8") == 255).all()
    # the disc operations keep shape, dtype and container
    for x in (a, a[:, :, None], torch.from_numpy(a), torch.from_numpy(a[:, :, None].copy())):
        for fn, op in ((ops.erode_disk, "erode"), (ops.dilate_disk, "dilate"), (ops.open_disk, "open"), (ops.close_disk, "close")):
            y = fn(x, 2.5)
            assert type(y) is type(x) and y.shape == x.shape and y.dtype == x.dtype
            assert (np.asarray(y).reshape(a.shape) == C.golden_disk_morph(a, op, 2.5)).all(), op
    for name in ("distance_transform", "distance_transform_reference", "erode_disk", "dilate_disk", "open_disk", "close_disk"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    ops.clear_cache()


def test_refusals():
    a = np.zeros((6, 7), np.uint8)
    with pytest.raises(ValueError, match=r"needs a 1-channel image, got C = 3; convert first \(gray, threshold"):
        ops.distance_transform(np.zeros((6, 7, 3), np.uint8))
    with pytest.raises(RuntimeError, match=r"needs a 1-channel image, got C = 3; convert first"):
        C.golden_distance(np.zeros((6, 7, 3), np.uint8))
    with pytest.raises(RuntimeError, match=r"needs a 1-channel image, got C = 3; convert first"):
        C.cpu_disk_morph(np.zeros((6, 7, 3), np.uint8), "erode", 1.0)
    with pytest.raises(TypeError, match="uint8"):
        ops.distance_transform(a.astype(np.int32))
    with pytest.raises(TypeError, match="uint8"):
        ops.erode_disk(a.astype(np.float32), 1)
    with pytest.raises(ValueError, match="one frame at a time"):
        ops.distance_transform(np.zeros((2, 6, 7, 1), np.uint8))
    with pytest.raises(ValueError, match="HxW or HxWx1"):
        ops.dilate_disk(np.zeros((6, 7, 2), np.uint8), 1)
    with pytest.raises(ValueError, match="radius must be finite and not negative, got -1"):
        ops.erode_disk(a, -1)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius must be finite and not negative"):
            ops.open_disk(a, bad)
    with pytest.raises(ValueError, match="radius must be a number"):
        ops.close_disk(a, "3")
    with pytest.raises(RuntimeError, match="radius must be finite and not negative"):
        C.golden_disk_morph(a, "erode", -0.5)
    with pytest.raises(RuntimeError, match="erode, dilate, open or close, got 'shrink'"):
        C.golden_disk_morph(a, "shrink", 1.0)
    with pytest.raises(ValueError, match="32768x1 has a side above 32767"):
        ops.distance_transform(np.zeros((1, 32768), np.uint8))
    with pytest.raises(RuntimeError, match="1x32768 has a side above 32767"):
        C.cpu_distance(np.zeros((32768, 1), np.uint8))
    with pytest.raises(ValueError, match="to must be background or foreground, got 'edge'"):
        ops.distance_transform(a, to="edge")
    with pytest.raises(ValueError, match="output must be one of squared, float, u8, got 'f64'"):
        ops.distance_transform(a, output="f64")
    with pytest.raises(RuntimeError, match="threshold must lie in"):
        C.golden_distance_mask(a, False, -1, True)
    assert C.check_radius(3.7) == 13 and C.check_radius(0) == 0 and C.check_radius(1e9) == 2 ** 31 - 2
    # the limit itself is accepted
    d = ops.distance_transform(np.zeros((1, 32767), np.uint8), "foreground")
    assert d.shape == (1, 32767) and (d == ops.DISTANCE_NONE).all()


def run_cli(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


@pytest.mark.skipif(not os.path.exists(STRIPE), reason="bin/stripe not built")
def test_cli_distance_on_the_host_backend(tmp_path):
    a = np.random.default_rng(4).integers(0, 256, (40, 52), dtype=np.uint8)
    a[8:32, 5:30] = 250  # one thick object among the noise
    src, dst = str(tmp_path / "a.pgm"), str(tmp_path / "d.pgm")
    C.write_pnm(src, a)
    chain = "threshold:128,open3"
    mask = ops.apply(a, chain)
    r = run_cli([STRIPE, "distance", "--input", src, "--chain", chain, "--backend", "host", "--output", dst])
    assert r.returncode == 0, r.stderr
    d2 = ops.distance_transform(mask)
    assert r.stdout.strip() == str(int(d2.max())) and d2.max() >= 100
    assert (C.read_pnm(dst) == ops.distance_transform(mask, output="u8")).all()
    r = run_cli([STRIPE, "distance", "--input", src, "--chain", chain, "--backend", "host", "--to", "foreground",
                 "--output", dst])
    assert r.returncode == 0 and r.stdout.strip() == str(int(ops.distance_transform(mask, "foreground").max())), r.stderr
    assert (C.read_pnm(dst) == ops.distance_transform(mask, "foreground", "u8")).all()
    for flag, fn in (("--erode", ops.erode_disk), ("--dilate", ops.dilate_disk), ("--open", ops.open_disk),
                     ("--close", ops.close_disk)):
        r = run_cli([STRIPE, "distance", "--input", src, "--chain", chain, "--backend", "host", flag, "3.5",
                     "--output", dst])
        assert r.returncode == 0, r.stderr
        assert (C.read_pnm(dst) == fn(mask, 3.5)).all(), flag
        assert r.stdout.strip() == str(int(d2.max()))
    # a frame without a site
    full = str(tmp_path / "full.pgm")
    C.write_pnm(full, np.full((5, 6), 200, np.uint8))
    r = run_cli([STRIPE, "distance", "--input", full, "--backend", "host", "--output", dst])
    assert r.returncode == 0 and r.stdout.strip() == "none" and (C.read_pnm(dst) == 255).all(), r.stderr
    # refusals: an RGB input without a conversion, a bad radius, two operations, a bad polarity
    rgb = str(tmp_path / "c.ppm")
    C.write_pnm(rgb, np.dstack([a, a, a]))
    r = run_cli([STRIPE, "distance", "--input", rgb, "--chain", "invert", "--backend", "host"])
    assert r.returncode != 0 and "convert first" in r.stderr
    r = run_cli([STRIPE, "distance", "--input", src, "--backend", "host", "--erode", "-2"])
    assert r.returncode != 0 and "radius must be finite and not negative" in r.stderr
    r = run_cli([STRIPE, "distance", "--input", src, "--backend", "host", "--erode", "2", "--open", "2"])
    assert r.returncode != 0 and "at most one of" in r.stderr
    r = run_cli([STRIPE, "distance", "--input", src, "--backend", "host", "--to", "edge"])
    assert r.returncode != 0 and "background or foreground" in r.stderr
