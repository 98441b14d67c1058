"""Resize on the host (csrc/core/resize.cpp, cpu_resize): the tap tables, the
golden loop and the threaded executor against the numpy mirror of the rule
(tests/np_resize.py), the accuracy bound against the float64 geometry, torch's
interpolate and Pillow's BOX, the refusals, `ops.resize` and the CLI.  No GPU.

The shape list carries 330x330 -> 10x11: its 330 -> 10 axis is a factor of 33,
which the rule refuses for area.  That shape runs under bilinear and nearest
and is expected to be refused under auto / area; 330x330 -> 11x11 stands in
for it under area.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import mpi_cuda_imagemanipulation_amd as m
import np_resize as R

C = m._C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPE = os.path.join(ROOT, "bin", "stripe")
MODES = ("auto", "nearest", "bilinear", "area")

AXES = [(1, 1), (1, 5), (5, 1), (2, 3), (7, 3), (131, 65), (131, 262), (330, 11), (16383, 512), (16384, 512),
        (65535, 2048)]


def legal(n_in, n_out, mode):
    return mode != "area" or (n_out <= n_in and n_in <= 32 * n_out)


@pytest.mark.parametrize("n_in,n_out", AXES)
@pytest.mark.parametrize("mode", MODES)
def test_taps(n_in, n_out, mode):
    if not legal(n_in, n_out, mode):
        with pytest.raises(RuntimeError, match="area"):
            C.resize_taps(n_in, n_out, mode)
        return
    first, count, w = C.resize_taps(n_in, n_out, mode)
    assert first.shape == count.shape == (n_out,) and w.shape == (count.sum(),)
    assert (count >= 1).all() and (w >= 0).all() and (w <= 32768).all()
    off = np.concatenate([[0], np.cumsum(count)])
    assert (np.add.reduceat(w, off[:-1]) == 32768).all()  # every output's weights sum to one
    assert (first >= 0).all() and (first + count <= n_in).all()
    assert (np.diff(first) >= 0).all()
    f2, c2, w2 = R.taps(n_in, n_out, mode)
    assert (first == f2).all() and (count == c2).all() and (w == np.concatenate(w2)).all()
    if R.resolve(n_in, n_out, mode) == "area":
        assert count.max() <= 33
        # coverage: the spans tile [0, n_in) (adjacent cells share at most one pixel)
        assert first[0] == 0 and first[-1] + count[-1] == n_in
        nxt = first[1:] - (first[:-1] + count[:-1])
        assert ((nxt == 0) | (nxt == -1)).all()


def frames(W, H):
    """random, 0/255 noise, and only the last pixel non-zero; gray and RGB"""
    rng = np.random.default_rng(W * 1000 + H)
    for shape in ((H, W), (H, W, 3)):
        yield "random", rng.integers(0, 256, shape, dtype=np.uint8)
        yield "checker", (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8)
        last = np.zeros(shape, np.uint8)
        last[-1, -1] = 255
        yield "last", last


# (W, H) -> (W2, H2), mode
SHAPES = [
    (67, 131, 33, 65, "bilinear"), (67, 131, 67, 131, "bilinear"), (67, 131, 1, 1, "bilinear"),
    (67, 131, 134, 262, "bilinear"), (67, 131, 100, 57, "bilinear"), (67, 131, 20, 40, "bilinear"),
    (67, 131, 33, 65, "auto"), (67, 131, 67, 131, "auto"), (67, 131, 134, 262, "auto"), (67, 131, 100, 57, "auto"),
    (67, 131, 20, 40, "auto"), (67, 131, 1, 1, "nearest"), (67, 131, 33, 65, "nearest"), (67, 131, 134, 262, "nearest"),
    (64, 96, 16, 32, "auto"), (64, 96, 16, 32, "area"),
    (97, 203, 13, 7, "auto"),
    (330, 330, 10, 11, "bilinear"), (330, 330, 10, 11, "nearest"), (330, 330, 11, 11, "area"),
    (5, 7, 5, 3, "auto"),
    (3, 2, 17, 9, "auto"), (3, 2, 17, 9, "nearest"),
    (1, 1, 4, 5, "auto"),
    (1280, 40, 40, 40, "auto"),
]


@pytest.mark.parametrize("W,H,W2,H2,mode", SHAPES)
def test_golden_is_the_mirror_and_cpu_is_golden(W, H, W2, H2, mode):
    tx, ty = C.resize_taps(W, W2, mode)[1].max(), C.resize_taps(H, H2, mode)[1].max()
    for name, a in frames(W, H):
        g = C.golden_resize(a, W2, H2, mode)
        assert g.shape == (H2, W2) + a.shape[2:]
        assert (g == R.resize(a, W2, H2, mode)).all(), name
        for t in (1, 2, 7):
            assert (C.cpu_resize(a, W2, H2, mode, t) == g).all(), (name, t)
        # against the same geometry in float64 with real-valued weights
        err = np.abs(g.astype(np.float64) - R.resize_real(a, W2, H2, mode)).max()
        assert err <= R.bound(tx, ty), (name, err)


def test_threads_split_a_frame_large_enough_to_split():
    # cpu_resize only splits frames above a work threshold: this one is split at 2 and 7 threads
    a = np.random.default_rng(5).integers(0, 256, (1500, 1100, 3), dtype=np.uint8)
    for W2, H2, mode in ((367, 501, "auto"), (1400, 1700, "auto"), (1100, 700, "nearest")):
        g = C.cpu_resize(a, W2, H2, mode, 1)
        for t in (2, 7):
            assert (C.cpu_resize(a, W2, H2, mode, t) == g).all(), (W2, H2, mode, t)
    s = a[:260, :240]
    assert (C.golden_resize(s, 77, 91, "auto") == C.cpu_resize(s, 77, 91, "auto", 3)).all()


def test_factor_33_shape_is_refused_under_area():
    a = np.zeros((330, 330), np.uint8)
    for mode in ("auto", "area"):
        with pytest.raises(RuntimeError, match=r"330 / 10 exceeds the limit of 32.*two steps"):
            C.golden_resize(a, 10, 11, mode)


@pytest.mark.parametrize("mode", MODES)
def test_flat_frames_are_fixed_points_and_same_size_is_identity(mode):
    rng = np.random.default_rng(1)
    for v in (0, 1, 127, 254, 255):
        for W2, H2 in ((23, 31), (67, 131), (9, 70)) + (((140, 300),) if mode != "area" else ()):
            if mode == "area" and (W2 > 67 or H2 > 131 or 67 > 32 * W2 or 131 > 32 * H2):
                continue
            flat = np.full((131, 67, 3), v, np.uint8)
            assert (C.cpu_resize(flat, W2, H2, mode) == v).all()
            assert (C.golden_resize(flat[:, :, 0], W2, H2, mode) == v).all()
    a = rng.integers(0, 256, (57, 100, 3), dtype=np.uint8)
    assert (C.cpu_resize(a, 100, 57, mode) == a).all() and (C.golden_resize(a, 100, 57, mode) == a).all()


def test_bilinear_against_torch_float64():
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    rng = np.random.default_rng(2)
    for (W, H, W2, H2) in ((67, 131, 134, 262), (67, 131, 100, 57), (67, 131, 20, 40), (3, 2, 17, 9), (97, 203, 13, 7)):
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        t = torch.from_numpy(a).permute(2, 0, 1)[None].to(torch.float64)
        ref = F.interpolate(t, size=(H2, W2), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
        got = C.cpu_resize(a, W2, H2, "bilinear").astype(np.float64)
        assert np.abs(got - ref).max() <= R.bound(2, 2)


def test_area_at_integer_factors_is_the_block_mean():
    rng = np.random.default_rng(3)
    for fx, fy in ((2, 2), (3, 5), (32, 1), (1, 4), (7, 32)):
        W2, H2 = 9, 6
        a = rng.integers(0, 256, (H2 * fy, W2 * fx, 3), dtype=np.uint8)
        mean = a.reshape(H2, fy, W2, fx, 3).astype(np.float64).mean(axis=(1, 3))
        got = C.cpu_resize(a, W2, H2, "area")
        _, cx, _ = C.resize_taps(W2 * fx, W2, "area")
        _, cy, _ = C.resize_taps(H2 * fy, H2, "area")
        assert cx.max() == fx and cy.max() == fy
        assert np.abs(got - mean).max() <= R.bound(fx, fy)
        torch = pytest.importorskip("torch")
        t = torch.from_numpy(a).permute(2, 0, 1)[None].to(torch.float64)
        ref = torch.nn.functional.interpolate(t, size=(H2, W2), mode="area")[0].permute(1, 2, 0).numpy()
        assert np.abs(got - ref).max() <= R.bound(fx, fy)


def test_pillow_box_at_integer_factors():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(4)
    for fx, fy in ((2, 2), (3, 5), (4, 1)):
        a = rng.integers(0, 256, (12 * fy, 10 * fx, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(a).resize((10, 12), Image.BOX)).astype(int)
        assert np.abs(C.cpu_resize(a, 10, 12, "area").astype(int) - ref).max() <= 1


def test_refusals_name_the_argument():
    a = np.zeros((40, 66, 3), np.uint8)
    with pytest.raises(RuntimeError, match=r"area cannot grow an axis \(n_in 66 -> n_out 67\)"):
        C.cpu_resize(a, 67, 40, "area")
    with pytest.raises(RuntimeError, match=r"n_in / n_out = 66 / 2 exceeds the limit of 32.*two steps"):
        C.cpu_resize(a, 2, 40, "auto")
    with pytest.raises(RuntimeError, match=r"n_in / n_out = 66 / 2 exceeds"):
        C.resize_taps(66, 2, "area")
    assert C.resize_taps(64, 2, "area")[1].max() == 32  # the cap itself is allowed
    for fn in (C.golden_resize, C.cpu_resize):
        with pytest.raises(RuntimeError, match=r"(n_out 0|size 0x40) outside 1\.\.65535"):
            fn(a, 0, 40, "auto")
        with pytest.raises(RuntimeError, match=r"(n_out 65536|size 10x65536) outside 1\.\.65535"):
            fn(a, 10, 65536, "nearest")
        with pytest.raises(RuntimeError, match="unknown mode 'cubic'"):
            fn(a, 10, 10, "cubic")
        with pytest.raises(RuntimeError, match="1 or 3 channels"):
            fn(np.zeros((4, 4, 2), np.uint8), 2, 2, "auto")
    with pytest.raises(ValueError, match="HxW or HxWx3"):
        m.ops.resize(np.zeros((4, 4, 2), np.uint8), size=(2, 2))
    with pytest.raises(ValueError, match=r"size must lie in 1\.\.65535"):
        m.ops.resize(a, size=(0, 5))
    with pytest.raises(ValueError, match="mode must be one of"):
        m.ops.resize(a, size=(5, 5), mode="lanczos")
    with pytest.raises(ValueError, match="exactly one of size"):
        m.ops.resize(a)
    with pytest.raises(ValueError, match="exactly one of size"):
        m.ops.resize(a, size=(3, 3), scale=2)
    with pytest.raises(TypeError, match="uint8"):
        m.ops.resize(a.astype(np.float32), size=(3, 3))


@pytest.mark.parametrize("spec", ["40", "40x", "x30", "0x30", "40x0", "40x30x3", "-4x30", "4.5x30", "65536x3",
                                  "40x30:cubic", "40x30:", "axb", ""])
def test_malformed_specs_name_the_token(spec):
    with pytest.raises(RuntimeError) as e:
        C.parse_resize_spec(spec)
    assert f"resize spec '{spec}'" in str(e.value)


def test_specs():
    assert C.parse_resize_spec("40x30") == (40, 30, "auto")
    assert C.parse_resize_spec("1x65535:area") == (1, 65535, "area")
    assert C.parse_resize_spec("640x480:bilinear") == (640, 480, "bilinear")
    assert C.parse_resize_spec("8x8:nearest") == (8, 8, "nearest")


def test_ops_resize_on_numpy():
    rng = np.random.default_rng(6)
    a = rng.integers(0, 256, (57, 100, 3), dtype=np.uint8)
    assert (m.ops.resize(a, size=(30, 40)) == C.golden_resize(a, 40, 30, "auto")).all()
    assert (m.ops.resize(a, size=(30, 40), mode="nearest") == C.golden_resize(a, 40, 30, "nearest")).all()
    assert (m.ops.resize_reference(a, size=(30, 40)) == C.golden_resize(a, 40, 30, "auto")).all()
    # n_out = max(1, rint(n * s)): 57 * 0.5 = 28.5 -> 28 (rint rounds to even), 100 * 0.5 = 50
    assert m.ops.resize(a, scale=0.5).shape == (28, 50, 3)
    assert (m.ops.resize(a, scale=0.5) == C.golden_resize(a, 50, 28, "auto")).all()
    assert (m.ops.resize(a, scale=(2, 0.25)) == C.golden_resize(a, 25, 114, "auto")).all()
    assert m.ops.resize(a, scale=0.001, mode="nearest").shape == (1, 1, 3)
    g = a[:, :, 0]
    assert (m.ops.resize(g, size=(60, 99)) == C.golden_resize(g, 99, 60, "auto")).all()
    assert m.ops.resize(g[:, :, None], size=(60, 99)).shape == (60, 99, 1)
    b = np.stack([a, a[::-1], 255 - a])
    out = m.ops.resize(b, size=(20, 33))
    assert out.shape == (3, 20, 33, 3)
    for i in range(3):
        assert (out[i] == C.golden_resize(np.ascontiguousarray(b[i]), 33, 20, "auto")).all()
    assert m.ops.resize(b[:0], size=(20, 33)).shape == (0, 20, 33, 3)
    torch = pytest.importorskip("torch")
    t = m.ops.resize(torch.from_numpy(a), size=(30, 40))
    assert isinstance(t, torch.Tensor) and (t.numpy() == C.golden_resize(a, 40, 30, "auto")).all()
    assert "resize" not in " ".join(m.ops.FILTERS)  # not a chain token


def run_cli(*args):
    r = subprocess.run([STRIPE, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.skipif(not os.path.exists(STRIPE), reason="bin/stripe not built")
def test_cli_host_resize(tmp_path):
    a = np.random.default_rng(7).integers(0, 256, (57, 100, 3), dtype=np.uint8)
    src, dst = str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm")
    C.write_pnm(src, a)
    j = run_cli("run", "--backend", "host", "--input", src, "--output", dst, "--resize", "40x30:area", "--chain",
                "invert")
    assert j["resized_from"] == [100, 57] and (j["W"], j["H"]) == (40, 30)
    assert (C.read_pnm(dst) == 255 - C.golden_resize(a, 40, 30, "area")).all()
    # without the flag nothing changes, and the JSON line has no such member
    j = run_cli("run", "--backend", "host", "--input", src, "--output", dst, "--chain", "invert")
    assert "resized_from" not in j and (C.read_pnm(dst) == 255 - a).all()
    # --held is resized the same way
    h = np.random.default_rng(8).integers(0, 256, (57, 100, 3), dtype=np.uint8)
    held = str(tmp_path / "h.ppm")
    C.write_pnm(held, h)
    j = run_cli("run", "--backend", "host", "--input", src, "--held", held, "--output", dst, "--resize", "150x80",
                "--chain", "absdiff")
    assert j["resized_from"] == [100, 57]
    ga, gh = C.golden_resize(a, 150, 80, "auto").astype(int), C.golden_resize(h, 150, 80, "auto").astype(int)
    assert (C.read_pnm(dst) == np.abs(ga - gh)).all()
    j = run_cli("convert", "--backend", "host", "--input", src, "--output", dst, "--resize", "33x20:nearest")
    assert j["resized_from"] == [100, 57] and (j["W"], j["H"]) == (33, 20)
    assert (C.read_pnm(dst) == C.golden_resize(a, 33, 20, "nearest")).all()
    r = subprocess.run([STRIPE, "convert", "--backend", "host", "--input", src, "--output", dst, "--resize", "33by20"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "resize spec '33by20'" in r.stderr


def test_python_cli_host_resize(tmp_path):
    from mpi_cuda_imagemanipulation_amd.__main__ import main

    a = np.random.default_rng(9).integers(0, 256, (57, 100, 3), dtype=np.uint8)
    src, dst = str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm")
    C.write_pnm(src, a)
    assert main(["run", "--backend", "host", "--input", src, "--output", dst, "--resize", "40x30:area", "--chain",
                 "invert"]) == 0
    assert (C.read_pnm(dst) == 255 - C.golden_resize(a, 40, 30, "area")).all()
