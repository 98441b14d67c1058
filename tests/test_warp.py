"""The affine warp rule on the CPU (csrc/include/stripe/warp.h): golden_warp ==
the numpy mirror == cpu_warp at 1, 3 and 8 threads over gray / RGB x both modes
x both borders; the float64 bound on the bilinear cases; the fixed points; the
quantiser's integers; the `fit` sizes; the parsers and their refusals; the CLI
on the host backend."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mpi_cuda_imagemanipulation_amd as m
from np_warp import ANGLES, bound, float_warp, invert, maps, np_warp, quantise

C = m._C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPE = os.path.join(ROOT, "bin", "stripe")
ONE = 1 << 24
BORDERS = (("constant", 0), ("constant", 200), ("replicate", 0))
SIZES = ((90, 70), (1, 1), (2, 300), (300, 2))


def frame(W, H, ch):
    shape = (H, W) if ch == 1 else (H, W, ch)
    return np.random.default_rng(W * 7919 + H * 31 + ch).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_golden_mirror_and_host_executor_agree(ch, size):
    W, H = size
    a = frame(W, H, ch)
    for name, minv, W2, H2 in maps(C, W, H):
        q = quantise(C, minv, W, H, W2, H2)
        for mode in ("bilinear", "nearest"):
            for border, fill in BORDERS:
                g = C.golden_warp(a, q, W2, H2, mode, border, fill)
                assert g.shape[:2] == (H2, W2)
                assert (g == np_warp(a, q, W2, H2, mode, border, fill)).all(), (name, mode, border)
                for threads in (1, 3, 8):
                    assert (g == C.cpu_warp(a, q, W2, H2, mode, border, fill, threads)).all(), (name, mode, border)
                if mode == "bilinear":
                    err = np.abs(g.astype(np.float64) - float_warp(a, minv, W2, H2, border, fill)).max()
                    assert err <= bound(W2, H2), (name, border, err)
        if name == "all-outside":
            assert (C.golden_warp(a, q, W2, H2, "bilinear", "constant", 200) == 200).all()


def test_host_executor_threads_on_a_frame_large_enough_to_split():
    a = frame(300, 290, 3)
    minv, W2, H2 = C.rotate_matrix(30.0, True, 300, 290)
    q = quantise(C, minv, 300, 290, W2, H2)
    for mode in ("bilinear", "nearest"):
        g = C.golden_warp(a, q, W2, H2, mode, "constant", 7)
        for threads in (1, 3, 8):
            assert (g == C.cpu_warp(a, q, W2, H2, mode, "constant", 7, threads)).all()


@pytest.mark.parametrize("ch", [1, 3])
def test_quarter_turns_are_exact(ch):
    for (W, H) in ((90, 70), (33, 34), (1, 5)):
        a = frame(W, H, ch)
        for k, op in ((0, "none"), (1, "rot270"), (2, "rot180"), (3, "rot90")):
            minv, W2, H2 = C.rotate_matrix(90.0 * k, True, W, H)
            q = quantise(C, minv, W, H, W2, H2)
            for mode in ("bilinear", "nearest"):
                g = C.golden_warp(a, q, W2, H2, mode, "constant", 0)
                assert (g == np.rot90(a, k)).all() and (g == C.golden_orient(a, op)).all(), (k, mode)
        # 180 keeps the size without `fit` too
        minv, W2, H2 = C.rotate_matrix(180.0, False, W, H)
        assert (C.golden_warp(a, quantise(C, minv, W, H, W2, H2), W2, H2) == np.rot90(a, 2)).all()


def test_fixed_points():
    for ch in (1, 3):
        a = frame(64, 48, ch)
        flat = np.full_like(a, 137)
        for name, minv, W2, H2 in maps(C, 64, 48):
            q = quantise(C, minv, 64, 48, W2, H2)
            for mode in ("bilinear", "nearest"):
                assert (C.golden_warp(flat, q, W2, H2, mode, "replicate", 0) == 137).all(), name
        for mode in ("bilinear", "nearest"):
            for border, fill in BORDERS:
                assert (C.golden_warp(a, [ONE, 0, 0, 0, ONE, 0], 64, 48, mode, border, fill) == a).all()
                # an integer translation: out[y, x] = a[y + 5, x - 3] where that exists
                q = quantise(C, invert([1, 0, 3, 0, 1, -5]), 64, 48, 64, 48)
                g = C.golden_warp(a, q, 64, 48, mode, border, fill)
                assert (g[:43, 3:] == a[5:, :61]).all()
                if border == "constant":
                    assert (g[43:] == fill).all() and (g[:, :3] == fill).all()
                else:
                    assert (g[43:, 3:] == a[47:, :61]).all() and (g[:43, :3] == a[5:, :1]).all()


def test_quantiser_integers():
    Q = lambda M, inverse=False, **kw: C.warp_quantise([float(v) for v in M], inverse, 10, 8, **kw)
    assert Q([1, 0, 0, 0, 1, 0]) == (ONE, 0, 0, 0, ONE, 0, 10, 8)
    assert Q([2, 0, 0, 0, 4, 0], W2=20, H2=32) == (ONE // 2, 0, 0, 0, ONE // 4, 0, 20, 32)
    assert Q([1, 0, 3, 0, 1, -2]) == (ONE, 0, -3 * ONE, 0, ONE, 2 * ONE, 10, 8)
    assert Q([1, 0, 0.5, 0, 1, 1.25], True) == (ONE, 0, ONE // 2, 0, ONE, ONE + ONE // 4, 10, 8)
    # x' = -y + 5, y' = x + 7  <=>  x = y' - 7, y = -x' + 5
    assert Q([0, -1, 5, 1, 0, 7]) == (0, ONE, -7 * ONE, -ONE, 0, 5 * ONE, 10, 8)
    # rounding to nearest: 1/3 = 0x555555.55..; the largest coefficients and offsets
    assert Q([3, 0, 0, 0, -3, 0])[:6] == (5592405, 0, 0, 0, -5592405, 0)
    assert Q([63.9, 0, 1048575.5, 0, -63.9, -1048575.5], True)[:6] == (
        round(63.9 * ONE), 0, 1048575 * ONE + ONE // 2, 0, -round(63.9 * ONE), -1048575 * ONE - ONE // 2)
    # forward and inverse forms of one map give the same integers
    for M in ([2, 0, 6, 0, 0.5, -3], [0, -1, 5, 1, 0, 7], [1, 0.5, 0, 0, 1, 0], [4, 0, 1, 0, 4, 3]):
        assert Q(M) == Q(invert(M), True), M


def test_fit_sizes_and_rotation_matrix():
    size = lambda deg, fit=True: tuple(C.rotate_matrix(float(deg), fit, 100, 50)[1:])
    assert size(0) == (100, 50) and size(90) == (50, 100) and size(180) == (100, 50) and size(270) == (50, 100)
    assert size(30) == (112, 94)    # 100 * 0.8660 + 50 * 0.5 = 111.60; 100 * 0.5 + 50 * 0.8660 = 93.30
    assert size(45) == (107, 107)   # 150 * 0.70711 = 106.07
    assert size(30, False) == (100, 50) and size(450) == (50, 100) and size(-90) == (50, 100)
    assert tuple(C.rotate_matrix(45.0, True, 1, 1)[1:]) == (2, 2)
    # multiples of 90 use exact cosines; the centre maps to the centre
    assert C.rotate_matrix(90.0, True, 4, 3)[0] == [0.0, -1.0, 3.0, 1.0, 0.0, 0.0]
    assert C.rotate_matrix(-270.0, True, 4, 3)[0] == [0.0, -1.0, 3.0, 1.0, 0.0, 0.0]
    for deg in ANGLES:
        minv, W2, H2 = C.rotate_matrix(float(deg), True, 31, 18)
        t = np.deg2rad(deg % 360)
        assert np.allclose(minv[:2] + minv[3:5], [np.cos(t), -np.sin(t), np.sin(t), np.cos(t)], atol=1e-15)
        cx, cy = (W2 - 1) / 2, (H2 - 1) / 2
        assert abs(minv[0] * cx + minv[1] * cy + minv[2] - 15.0) < 1e-9
        assert abs(minv[3] * cx + minv[4] * cy + minv[5] - 8.5) < 1e-9
    # counter-clockwise as seen: the top-right corner of a square goes to the top-left
    a = np.zeros((9, 9), np.uint8)
    a[0, 8] = 255
    assert m.ops.rotate(a, 90)[0, 0] == 255 and m.ops.rotate(a, 90).sum() == 255


def test_parsers_round_trip():
    assert C.parse_warp_spec("1;0;2.5;0;1;-3") == ([1.0, 0.0, 2.5, 0.0, 1.0, -3.0], 0, 0)
    assert C.parse_warp_spec("0.5;-1e-3;2.5;.25;1;-3:40x30") == ([0.5, -0.001, 2.5, 0.25, 1.0, -3.0], 40, 30)
    for M in ([1, 0, 2.5, 0, 1, -3], [0.1, 1 / 3, -7e-5, 2 ** 0.5, 63.9, 1e5]):
        token = C.warp_token([float(v) for v in M], 40, 30)
        assert token.startswith("affine:") and token.endswith(":40x30")
        assert C.parse_warp_spec(token[len("affine:"):]) == ([float(v) for v in M], 40, 30)
    assert C.warp_token([1.0, 0.0, 2.5, 0.0, 1.0, -3.0], 40, 30) == "affine:1;0;2.5;0;1;-3:40x30"
    assert C.parse_rotate_spec("30") == (30.0, False, "rotate:30:same")
    assert C.parse_rotate_spec("-77.7:fit") == (-77.7, True, "rotate:-77.7:fit")
    assert C.parse_rotate_spec("1e1:same") == (10.0, False, "rotate:10:same")
    assert C.parse_warp_border("constant") == ("constant", 0) and C.parse_warp_border("constant:200") == ("constant", 200)
    assert C.parse_warp_border("replicate") == ("replicate", 0)
    assert C.parse_warp_mode("nearest") == "nearest" and C.parse_warp_mode("bilinear") == "bilinear"
    # the forward matrix of a spec and its inverse give one map
    M, W2, H2 = C.parse_warp_spec("2;0;6;0;0.5;-3:20x4")
    assert C.warp_quantise(M, False, 10, 8, W2, H2) == C.warp_quantise(invert(M), True, 10, 8, W2, H2)


REFUSALS = [
    (lambda: C.parse_warp_spec("nan;0;0;0;1;0"), "warp spec 'nan;0;0;0;1;0': non-finite"),
    (lambda: C.parse_warp_spec("1;0;inf;0;1;0"), "warp spec '1;0;inf;0;1;0': non-finite"),
    (lambda: C.parse_warp_spec("1;0;0;0;1"), "warp spec '1;0;0;0;1': expected six numbers"),
    (lambda: C.parse_warp_spec("1;0;0;0;1;0;0"), "expected six numbers"),
    (lambda: C.parse_warp_spec("1;0;0;0;1;x"), "expected six numbers"),
    (lambda: C.parse_warp_spec("1;0;0;0;1;0:0x5"), r"warp spec '1;0;0;0;1;0:0x5': destination size outside 1\.\.65535"),
    (lambda: C.parse_warp_spec("1;0;0;0;1;0:70000x5"), r"destination size outside 1\.\.65535"),
    (lambda: C.parse_warp_spec("1;0;0;0;1;0:40"), "expected a size WxH"),
    (lambda: C.warp_quantise([1.0, 2, 0, 2, 4, 0], False, 5, 5, 5, 5, "T"), "warp 'T': singular matrix"),
    (lambda: C.warp_quantise([0.0, 0, 0, 0, 0, 0], True, 5, 5, 5, 5, "T"), "warp 'T': singular matrix"),
    (lambda: C.warp_quantise([float("nan"), 0, 0, 0, 1, 0], False, 5, 5, 5, 5, "T"), "warp 'T': non-finite"),
    (lambda: C.warp_quantise([0.01, 0, 0, 0, 1, 0], False, 5, 5, 5, 5, "T"),
     r"warp 'T': inverse map coefficient 100 outside \(-64, 64\)"),
    (lambda: C.warp_quantise([64.0, 0, 0, 0, 1, 0], True, 5, 5, 5, 5, "T"), r"coefficient 64 outside \(-64, 64\)"),
    # values that pass |v| < 64 (|v| < 2^20) and round to 2^30 (2^44) are refused here, by name
    (lambda: C.warp_quantise([64 - 2.0 ** -30, 0, 0, 0, 1, 0], True, 5, 5, 5, 5, "T"),
     r"warp 'T': inverse map coefficient 64 outside \(-64, 64\)"),
    (lambda: C.warp_quantise([1.0, 0, 0, 0, 1, -(2.0 ** 20 - 2.0 ** -30)], True, 5, 5, 5, 5, "T"),
     r"warp 'T': inverse map offset -1\.04858e\+06 outside \(-2\^20, 2\^20\)"),
    (lambda: C.parse_warp_spec("0x1p0;0;0;0;1;0"), "expected six numbers"),
    (lambda: C.parse_warp_spec(" 1;0;0;0;1;0"), "expected six numbers"),
    (lambda: C.warp_quantise([1.0, 0, 2.0 ** 20, 0, 1, 0], False, 5, 5, 5, 5, "T"),
     r"warp 'T': inverse map offset -1\.04858e\+06 outside \(-2\^20, 2\^20\)"),
    (lambda: C.warp_quantise([1.0, 0, 0, 0, 1, 0], False, 0, 5, 5, 5, "T"), r"warp 'T': source size 0x5 outside 1\.\.65535"),
    (lambda: C.warp_quantise([1.0, 0, 0, 0, 1, 0], False, 5, 5, 5, 65536, "T"),
     r"warp 'T': destination size 5x65536 outside 1\.\.65535"),
    (lambda: C.parse_rotate_spec("nan"), "rotate spec 'nan': non-finite angle"),
    (lambda: C.parse_rotate_spec("30:bogus"), r"rotate spec '30:bogus': expected DEG\[:same\|fit\]"),
    (lambda: C.parse_rotate_spec("thirty"), "rotate spec 'thirty': expected DEG"),
    (lambda: C.rotate_matrix(30.0, True, 0, 4), r"rotate: size 0x4 outside 1\.\.65535"),
    (lambda: C.rotate_matrix(float("inf"), True, 4, 4), "rotate: non-finite angle"),
    (lambda: C.parse_warp_mode("cubic"), r"warp: unknown mode 'cubic' \(bilinear \| nearest\)"),
    (lambda: C.parse_warp_border("wrap"), r"warp: unknown border 'wrap' \(constant\[:V\] \| replicate\)"),
    (lambda: C.parse_warp_border("constant:256"), "warp border 'constant:256': the fill value must be an integer in 0..255"),
    (lambda: C.golden_warp(np.zeros((4, 4, 2), np.uint8), [ONE, 0, 0, 0, ONE, 0], 4, 4), "1 or 3 channels"),
    (lambda: C.golden_warp(np.zeros((4, 4), np.uint8), [ONE, 0, 0, 0, ONE, 0], 0, 4), r"destination size 0x4 outside"),
    (lambda: C.cpu_warp(np.zeros((4, 4), np.uint8), [ONE, 0, 0, 0, ONE, 0], 4, 70000), r"destination size 4x70000 outside"),
    (lambda: C.golden_warp(np.zeros((4, 4), np.uint8), [64 * ONE, 0, 0, 0, ONE, 0], 4, 4), r"coefficient outside \(-64, 64\)"),
    (lambda: C.golden_warp(np.zeros((4, 4), np.uint8), [ONE, 0, 0, 0, ONE], 4, 4), "six integers"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals(i):
    call, msg = REFUSALS[i]
    with pytest.raises(RuntimeError, match=msg):
        call()


def test_front_end_on_arrays():
    a = frame(60, 40, 3)
    M = [[0.9, 0.2, 3], [-0.2, 0.9, 5]]
    q = list(C.warp_quantise([0.9, 0.2, 3, -0.2, 0.9, 5], False, 60, 40, 50, 45)[:6])
    ref = C.golden_warp(a, q, 50, 45, "bilinear", "constant", 9)
    assert (m.ops.warp_affine(a, M, size=(45, 50), fill=9) == ref).all()
    assert (m.ops.warp_reference(a, np.array(M), size=(45, 50), fill=9) == ref).all()
    assert (m.ops.warp_affine(a, invert(np.ravel(M)), size=(45, 50), fill=9, inverse=True) ==
            m.ops.warp_reference(a, invert(np.ravel(M)), size=(45, 50), fill=9, inverse=True)).all()
    assert m.ops.warp_affine(a[:, :, :1], M).shape == (40, 60, 1)
    assert (m.ops.warp_affine(a[:, :, 0], M, mode="nearest", border="replicate") ==
            m.ops.warp_reference(a[:, :, 0], M, mode="nearest", border="replicate")).all()
    b = np.stack([a, 255 - a])
    out = m.ops.rotate(b, 30, expand=True)
    minv, W2, H2 = C.rotate_matrix(30.0, True, 60, 40)
    assert out.shape == (2, H2, W2, 3)
    assert (out[1] == C.golden_warp(255 - a, quantise(C, minv, 60, 40, W2, H2), W2, H2)).all()
    assert m.ops.rotate(b[:0], 30, expand=True).shape == (0, H2, W2, 3)
    for k in range(4):
        assert (m.ops.rotate(a, 90 * k, expand=True) == np.rot90(a, k)).all()
    with pytest.raises(TypeError, match="uint8"):
        m.ops.rotate(a.astype(np.float32), 3)
    with pytest.raises(ValueError, match="singular"):
        m.ops.warp_affine(a, [[1, 2, 0], [2, 4, 0]])
    with pytest.raises(ValueError, match="2x3"):
        m.ops.warp_affine(a, [[1, 0], [0, 1]])
    with pytest.raises(ValueError, match="unknown mode"):
        m.ops.rotate(a, 3, mode="cubic")
    with pytest.raises(ValueError, match="unknown border"):
        m.ops.rotate(a, 3, border="wrap")
    with pytest.raises(ValueError, match="fill"):
        m.ops.rotate(a, 3, fill=256)
    with pytest.raises(ValueError, match="non-finite"):
        m.ops.rotate(a, float("nan"))
    with pytest.raises(ValueError, match="outside 1..65535"):
        m.ops.warp_affine(a, M, size=(0, 5))


def run_cli(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


@pytest.mark.skipif(not os.path.exists(STRIPE), reason="bin/stripe not built")
def test_cli_on_the_host_backend(tmp_path):
    a = frame(120, 80, 3)
    src, dst = str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm")
    C.write_pnm(src, a)
    base = [STRIPE, "run", "--input", src, "--output", dst, "--backend", "host", "--chain", "gaussian5"]
    r = run_cli(base + ["--rotate", "-30:fit", "--warp-border", "constant:77"])
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    minv, W2, H2 = C.rotate_matrix(-30.0, True, 120, 80)
    assert j["warped_from"] == [120, 80] and j["warp"] == "rotate:-30:fit" and (j["W"], j["H"]) == (W2, H2)
    ref = C.golden_warp(a, quantise(C, minv, 120, 80, W2, H2), W2, H2, "bilinear", "constant", 77)
    assert (C.read_pnm(dst) == C.golden_apply(ref, "gaussian5", "reflect101", True)).all()
    # a matrix, after --orient and before --resize
    spec = "0.8;0.1;4;-0.1;0.8;9:100x90"
    r = run_cli(base + ["--orient", "rot90", "--warp", spec, "--warp-mode", "nearest", "--warp-border", "replicate",
                        "--resize", "50x45:nearest"])
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["oriented"] == "rot90" and j["warped_from"] == [80, 120] and j["resized_from"] == [100, 90]
    assert j["warp"] == "affine:0.8;0.1;4;-0.1;0.8;9:100x90"
    o = C.golden_orient(a, "rot90")
    q = list(C.warp_quantise([0.8, 0.1, 4, -0.1, 0.8, 9], False, 80, 120, 100, 90)[:6])
    ref = C.golden_resize(C.golden_warp(o, q, 100, 90, "nearest", "replicate", 0), 50, 45, "nearest")
    assert (C.read_pnm(dst) == C.golden_apply(ref, "gaussian5", "reflect101", True)).all()
    # convert takes the same flags; without them the JSON line has no new member
    r = run_cli([STRIPE, "convert", "--input", src, "--output", dst, "--backend", "host", "--rotate", "90:fit"])
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["warp"] == "rotate:90:fit"
    assert (C.read_pnm(dst) == np.rot90(a, 1)).all()
    r = run_cli(base)
    assert r.returncode == 0 and "warp" not in r.stdout
    for extra, msg in ((["--rotate", "3", "--warp", "1;0;0;0;1;0"], "mutually exclusive"),
                       (["--warp-mode", "nearest"], "need --rotate or --warp"),
                       (["--warp", "1;2;0;2;4;0"], "singular matrix"),
                       (["--rotate", "3:big"], "rotate spec '3:big'")):
        r = run_cli(base + extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)


def test_python_cli_on_the_host_backend(tmp_path):
    a = frame(64, 48, 3)
    src, dst = str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm")
    C.write_pnm(src, a)
    r = run_cli([sys.executable, "-m", "mpi_cuda_imagemanipulation_amd", "run", "--input", src, "--output", dst,
                 "--backend", "host", "--chain", "invert", "--rotate=-12.5", "--warp-border", "replicate"])
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["warped_from"] == [64, 48] and j["warp"] == "rotate:-12.5:same"
    minv, W2, H2 = C.rotate_matrix(-12.5, False, 64, 48)
    ref = C.golden_warp(a, quantise(C, minv, 64, 48, W2, H2), W2, H2, "bilinear", "replicate", 0)
    assert (C.read_pnm(dst) == 255 - ref).all()
