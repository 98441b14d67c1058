"""Canny edges and hysteresis thresholding on the host: the golden class plane
and edge map against an independent numpy reference (tests/np_canny.py: shifted
slices, vectorised sector tests, scipy.ndimage.label), the threaded executor
against golden at 1, 3 and 8 threads, on every frame of canny_cases under every
border and norm at four threshold pairs and five shapes; pitched views with
guard bytes; the spiral and staircase masks through the hysteresis stage alone;
every refusal; the ops front end; `stripe edges`.  All comparisons are exact.

The suite must exercise the hysteresis: over the frames of the 65 x 257 shape
the reference has weak pixels that are kept and weak pixels that are dropped
(test_the_frames_exercise_the_hysteresis)."""
import os
import subprocess

import numpy as np
import pytest

import canny_cases as CC
import mpi_cuda_imagemanipulation_amd as m
import np_canny as NC

pytest.importorskip("scipy")

C = m._C
ops = m.ops
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPE = os.path.join(ROOT, "bin", "stripe")
THREADS = (1, 3, 8)
SHAPES = ((1, 1), (1, 9), (9, 1), (17, 70), (65, 257))
THRESHOLDS = ((40, 100), (100, 300), (0, 0), (2040, 2040))
BIG = (300, 420)  # large enough for the executor to split the rows into several blocks

_frames = {}


def frames(shape):
    if shape not in _frames:
        _frames[shape] = CC.frames(*shape)
    return _frames[shape]


def test_constants():
    assert C.CANNY_MAX_THRESHOLD == ops.CANNY_MAX_THRESHOLD == 2040 == 2 * 4 * 255
    assert C.HYSTERESIS_MAX_THRESHOLD == 255
    assert tuple(C.CANNY_NORMS) == NC.NORMS == ops.CANNY_NORMS
    # every term of the sector tests and the l2 magnitude fit their types
    assert (1020 << 15) < 2 ** 31 and 1020 * NC.TAN + (1020 << 16) < 2 ** 31
    assert 2 * 1020 ** 2 == 2080800 < 2 ** 21 and 2040 ** 2 < 2 ** 32


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_golden_numpy_and_the_host_executor_agree(shape):
    for name, a in frames(shape):
        for border in NC.BORDERS:
            for norm in NC.NORMS:
                for low, high in THRESHOLDS:
                    key = (shape, name, border, norm, low, high)
                    cls = NC.classes(a, low, high, norm, border)
                    want = NC.hysteresis(cls, 8)
                    assert (C.golden_canny_classes(a, low, high, norm, border) == cls).all(), key
                    assert (C.golden_canny(a, low, high, norm, border) == want).all(), key
                    for t in THREADS:
                        assert (C.cpu_canny_classes(a, low, high, norm, border, t) == cls).all(), key + (t,)
                        assert (C.cpu_canny(a, low, high, norm, border, t) == want).all(), key + (t,)


def test_row_blocks_of_a_larger_frame():
    for name, a in frames(BIG):
        if name not in ("blur_random", "blur_text", "ring", "step45up"):
            continue
        for border in NC.BORDERS:
            for norm in NC.NORMS:
                cls = NC.classes(a, 40, 100, norm, border)
                want = NC.hysteresis(cls, 8)
                for t in THREADS + (16,):
                    assert (C.cpu_canny_classes(a, 40, 100, norm, border, t) == cls).all(), (name, border, norm, t)
                    assert (C.cpu_canny(a, 40, 100, norm, border, t) == want).all(), (name, border, norm, t)


def test_the_frames_exercise_the_hysteresis():
    """Counted from the reference: weak pixels that are kept and weak pixels that are dropped both occur."""
    kept = dropped = strong = 0
    per_frame = {}
    for name, a in frames((65, 257)):
        cls = C.golden_canny_classes(a, 40, 100, "l1", "reflect101")
        edge = C.golden_canny(a, 40, 100, "l1", "reflect101")
        assert (edge[cls == 2] == 255).all() and (edge[cls == 0] == 0).all()
        k, d = int(((cls == 1) & (edge == 255)).sum()), int(((cls == 1) & (edge == 0)).sum())
        per_frame[name] = (int((cls == 2).sum()), k, d)
        strong, kept, dropped = strong + per_frame[name][0], kept + k, dropped + d
    print("strong, weak kept, weak dropped per frame:", per_frame)
    assert kept > 0 and dropped > 0 and strong > 0, per_frame
    for name in ("blur_random", "blur_text"):
        assert per_frame[name][1] > 0 and per_frame[name][2] > 0, (name, per_frame[name])


def test_two_pixel_plateaus_keep_exactly_one_pixel():
    """A step's Sobel response is two pixels wide at equal magnitude: the asymmetric > / >= keeps the first."""
    H, W = 17, 70
    f = dict(frames((H, W)))
    for pol in ("up", "down"):
        cls = C.golden_canny_classes(f[f"step90{pol}"], 40, 100, "l1", "replicate")
        assert (cls[:, W // 2 - 1] == 2).all() and (cls.sum(axis=1) == 2).all(), pol  # the left column only
        cls = C.golden_canny_classes(f[f"step0{pol}"], 40, 100, "l1", "replicate")
        assert (cls[H // 2 - 1, :] == 2).all() and (cls.sum(axis=0) == 2).all(), pol  # the upper row only


def test_pitched_views_with_guard_bytes():
    H, W = 17, 70
    a = dict(frames((H, W)))["blur_random"]
    wide = np.full((H, W + 9), 0xA5, np.uint8)
    src = wide[:, 3:3 + W]
    src[...] = a
    assert not src.flags.c_contiguous
    for fn, args, want in ((C.cpu_canny, (40, 100, "l2", "replicate", 3), NC.canny(a, 40, 100, "l2", "replicate")),
                           (C.cpu_canny_classes, (40, 100, "l1", "constant", 3), NC.classes(a, 40, 100, "l1", "constant")),
                           (C.cpu_hysteresis_threshold, (100, 180, 4, 3), NC.hysteresis_threshold(a, 100, 180, 4))):
        plane = np.full((H, W + 5), 77, np.uint8)
        out = plane[:, 2:2 + W]
        got = fn(src, *args, out)
        assert (out == want).all() and (got == want).all(), fn
        assert (plane[:, :2] == 77).all() and (plane[:, 2 + W:] == 77).all()
        assert (fn(src, *args) == want).all()
    assert (wide[:, :3] == 0xA5).all() and (wide[:, 3 + W:] == 0xA5).all() and (src == a).all()
    with pytest.raises(RuntimeError, match="must be packed"):
        C.cpu_canny(wide[:, ::2], 1, 2)
    with pytest.raises(RuntimeError, match=f"out must be {H}x{W}"):
        C.cpu_canny(src, 1, 2, "l1", "reflect101", 1, np.zeros((H, W + 1), np.uint8))


@pytest.mark.parametrize("shape", ((41, 41), (40, 57), (200, 200)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_spirals(shape):
    H, W = shape
    on = lambda path: {p for p in path}  # noqa: E731
    for conn in (4, 8):
        a, path, _ = CC.spiral(H, W)
        assert len(path) > (H * W) // 3  # the spiral crosses the whole frame
        want = np.where(a > 0, 255, 0).astype(np.uint8)  # one strong pixel at the inner end keeps all of it
        b, _, _ = CC.spiral(H, W, strong=False)
        g, gpath, k = CC.spiral(H, W, gap=True)
        want_gap = np.zeros((H, W), np.uint8)
        for y, x in gpath[k + 1:]:
            want_gap[y, x] = 255  # only the strong pixel's side of the gap
        assert 0 < int((want_gap == 255).sum()) < int((want == 255).sum()) - 1
        for fn in (lambda x: C.golden_hysteresis_threshold(x, 50, 150, conn), lambda x: NC.hysteresis_threshold(x, 50, 150, conn),
                   lambda x: C.cpu_hysteresis_threshold(x, 50, 150, conn, 1), lambda x: C.cpu_hysteresis_threshold(x, 50, 150, conn, 8),
                   lambda x: ops.hysteresis_threshold(x, 50, 150, conn)):
            assert (fn(a) == want).all(), (shape, conn)
            assert not fn(b).any(), (shape, conn)
            assert (fn(g) == want_gap).all(), (shape, conn)
    assert on(path) == on(gpath)


def test_staircase_tells_the_connectivities_apart():
    a = CC.staircase(23, 31)
    only_first = np.zeros_like(a)
    only_first[0, 0] = 255
    for t in THREADS:
        assert (C.cpu_hysteresis_threshold(a, 50, 150, 8, t) == np.where(a > 0, 255, 0)).all()
        assert (C.cpu_hysteresis_threshold(a, 50, 150, 4, t) == only_first).all()
    assert (C.golden_hysteresis_threshold(a, 50, 150, 8) == NC.hysteresis_threshold(a, 50, 150, 8)).all()
    assert (C.golden_hysteresis_threshold(a, 50, 150, 4) == only_first).all()


def test_hysteresis_threshold_on_every_frame():
    for shape in SHAPES:
        for name, a in frames(shape):
            for low, high in ((0, 0), (40, 100), (100, 254), (255, 255), (0, 255)):
                for conn in (4, 8):
                    want = NC.hysteresis_threshold(a, low, high, conn)
                    assert (C.golden_hysteresis_threshold(a, low, high, conn) == want).all(), (shape, name, low, high, conn)
                    for t in THREADS:
                        assert (C.cpu_hysteresis_threshold(a, low, high, conn, t) == want).all(), (shape, name, t)


def test_ops_front_end():
    torch = pytest.importorskip("torch")
    a = dict(frames((17, 70)))["blur_text"]
    want = NC.canny(a, 40, 100)
    for fn, args, ref in ((ops.canny, (40, 100), want), (ops.canny, (40, 100, "l2", "constant"), NC.canny(a, 40, 100, "l2", "constant")),
                          (ops.canny_classes, (40, 100), NC.classes(a, 40, 100)),
                          (ops.canny_reference, (40, 100), want),
                          (ops.hysteresis_threshold, (100, 150), NC.hysteresis_threshold(a, 100, 150)),
                          (ops.hysteresis_threshold, (100, 150, 4), NC.hysteresis_threshold(a, 100, 150, 4)),
                          (ops.hysteresis_threshold_reference, (100, 150, 4), NC.hysteresis_threshold(a, 100, 150, 4))):
        got = fn(a, *args)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and (got == ref).all(), (fn, args)
        if fn in (ops.canny_reference, ops.hysteresis_threshold_reference):
            assert (fn(torch.from_numpy(a), *args) == ref).all()
            continue
        t = fn(torch.from_numpy(a), *args)
        assert isinstance(t, torch.Tensor) and (t.numpy() == ref).all()
        g3 = fn(a[:, :, None], *args)
        assert g3.shape == a.shape + (1,) and (g3[:, :, 0] == ref).all()
    # any Python or numpy number whose value is integral
    for low, high in ((np.int64(40), np.uint8(100)), (40.0, np.float32(100)), (np.float64(40), 100)):
        assert (ops.canny(a, low, high) == want).all()
    assert set(np.unique(ops.canny(a, 40, 100))) <= {0, 255}
    for name in ("canny", "canny_reference", "canny_classes", "hysteresis_threshold", "hysteresis_threshold_reference"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    ops.clear_cache()


def test_refusals():
    a = np.zeros((6, 7), np.uint8)
    rgb = np.zeros((6, 7, 3), np.uint8)
    for fn in (ops.canny, ops.canny_classes, ops.canny_reference, ops.hysteresis_threshold, ops.hysteresis_threshold_reference):
        with pytest.raises(ValueError, match=r"canny: needs a 1-channel image, got C = 3; convert first \(gray, threshold"):
            fn(rgb, 1, 2)
        with pytest.raises(ValueError, match="one frame at a time"):
            fn(np.zeros((2, 6, 7, 1), np.uint8), 1, 2)
        with pytest.raises(ValueError, match="must be HxW or HxWx1"):
            fn(np.zeros((7,), np.uint8), 1, 2)
        with pytest.raises(ValueError, match="empty image"):
            fn(np.zeros((0, 7), np.uint8), 1, 2)
    for fn in (C.golden_canny, C.golden_canny_classes, C.golden_hysteresis_threshold, C.cpu_canny, C.cpu_canny_classes,
               C.cpu_hysteresis_threshold):
        with pytest.raises(RuntimeError, match="needs a 1-channel image, got C = 3; convert first"):
            fn(rgb, 1, 2)
    shared = "the thresholds must be integers with 0 <= low <= high <= 2040"
    for low, high in ((5, 3), (-1, 3), (0, 2041), (2.5, 3), (1, float("nan")), (1, float("inf")), ("1", 2), (True, 2),
                      (None, 2), (1, [2])):
        for fn in (ops.canny, ops.canny_classes, ops.canny_reference):
            with pytest.raises(ValueError, match=shared):
                fn(a, low, high)
    for fn in (C.golden_canny, C.golden_canny_classes, C.cpu_canny, C.cpu_canny_classes):
        for low, high in ((5, 3), (-1, 3), (0, 2041)):
            with pytest.raises(RuntimeError, match=shared + f", got low = {low}, high = {high}"):
                fn(a, low, high)
    shared8 = "the thresholds must be integers with 0 <= low <= high <= 255"
    for low, high in ((5, 3), (-1, 3), (0, 256), (2.5, 3)):
        for fn in (ops.hysteresis_threshold, ops.hysteresis_threshold_reference):
            with pytest.raises(ValueError, match=shared8):
                fn(a, low, high)
    for fn in (C.golden_hysteresis_threshold, C.cpu_hysteresis_threshold):
        with pytest.raises(RuntimeError, match=shared8 + ", got low = 0, high = 256"):
            fn(a, 0, 256)
        with pytest.raises(RuntimeError, match="connectivity must be 4 or 8, got 6"):
            fn(a, 1, 2, 6)
    for bad in (6, 8.0, True, "8"):
        with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
            ops.hysteresis_threshold(a, 1, 2, bad)
    with pytest.raises(ValueError, match="border must be reflect101, replicate or constant, got 'skip'"):
        ops.canny(a, 1, 2, border="skip")
    for fn in (C.golden_canny, C.cpu_canny, C.golden_canny_classes, C.cpu_canny_classes):
        with pytest.raises(RuntimeError, match="border must be reflect101, replicate or constant"):
            fn(a, 1, 2, "l1", "skip")
        with pytest.raises(RuntimeError, match="the norm must be l1 or l2, got 'linf'"):
            fn(a, 1, 2, "linf")
    with pytest.raises(ValueError, match="the norm must be l1 or l2, got 'linf'"):
        ops.canny(a, 1, 2, norm="linf")
    with pytest.raises(TypeError, match="uint8"):
        ops.canny(a.astype(np.int32), 1, 2)
    with pytest.raises(RuntimeError, match="must be uint8"):
        C.cpu_canny(a.astype(np.float32), 1, 2)
    # the limits themselves are accepted
    assert not ops.canny(a + 200, 2040, 2040).any() and not ops.hysteresis_threshold(a + 255, 255, 255).any()
    assert (ops.hysteresis_threshold(a + 1, 0, 0) == 255).all()


def run_cli(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


@pytest.mark.skipif(not os.path.exists(STRIPE), reason="bin/stripe not built")
def test_cli_edges_on_the_host_backend(tmp_path):
    a = dict(frames((65, 257)))["blur_text"]
    src, dst = str(tmp_path / "a.pgm"), str(tmp_path / "e.pgm")
    C.write_pnm(src, a)
    base = [STRIPE, "edges", "--input", src, "--backend", "host", "--output", dst]
    for extra, want in ((["--low", "40", "--high", "100"], NC.canny(a, 40, 100)),
                        (["--low", "40", "--high", "100", "--norm", "l2", "--border", "replicate"],
                         NC.canny(a, 40, 100, "l2", "replicate")),
                        (["--low", "0", "--high", "2040", "--border", "constant"], NC.canny(a, 0, 2040, "l1", "constant"))):
        r = run_cli(base + extra)
        assert r.returncode == 0, (extra, r.stderr)
        assert (C.read_pnm(dst) == want).all(), extra
        assert r.stdout.strip() == str(int((want == 255).sum()))
    # the chain runs first
    r = run_cli(base + ["--low", "20", "--high", "60", "--chain", "gaussian5"])
    assert r.returncode == 0, r.stderr
    want = NC.canny(ops.apply(a, "gaussian5"), 20, 60)
    assert want.any() and (C.read_pnm(dst) == want).all()
    # edges into label --min-area: short fragments go
    kept = str(tmp_path / "k.pgm")
    r = run_cli([STRIPE, "label", "--input", dst, "--backend", "host", "--min-area", "12", "--output", kept])
    assert r.returncode == 0, r.stderr
    assert (C.read_pnm(kept) == C.cpu_area_filter(want, 8, 12)).all()
    # refusals
    rgb = str(tmp_path / "c.ppm")
    C.write_pnm(rgb, np.dstack([a, a, a]))
    for args, msg in ((["--input", rgb, "--low", "1", "--high", "2"], "convert first"),
                      (["--input", src, "--low", "5", "--high", "3"], "0 <= low <= high <= 2040, got low = 5, high = 3"),
                      (["--input", src, "--low", "5", "--high", "2041"], "0 <= low <= high <= 2040"),
                      (["--input", src, "--high", "3"], "needs --low and --high"),
                      (["--input", src, "--low", "x", "--high", "3"], "--low needs an integer"),
                      (["--input", src, "--low", "1.5", "--high", "3"], "--low needs an integer"),
                      (["--input", src, "--low", "1", "--high", "3", "--norm", "linf"], "the norm must be l1 or l2"),
                      (["--input", src, "--low", "1", "--high", "3", "--border", "skip"], "reflect101, replicate or constant")):
        r = run_cli([STRIPE, "edges", "--backend", "host"] + args)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
