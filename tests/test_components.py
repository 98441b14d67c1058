"""Connected components on the host: the golden flood fill against
scipy.ndimage.label (renumbered to raster-first order), the statistics against
ndimage.sum / find_objects / coordinate sums, the threaded executor against the
golden labels with the seams at its row-block edges, the ops front end on numpy
arrays and CPU tensors, its refusals, and the `stripe label` subcommand.  All
comparisons are exact."""
import json
import os
import subprocess

import numpy as np
import pytest

import components_cases as K
import mpi_cuda_imagemanipulation_amd as m

C = m._C
ops = m.ops
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPE = os.path.join(ROOT, "bin", "stripe")
CONNS = (4, 8)
THREADS = (1, 2, 3, 7)
# odd sizes; heights whose row blocks (H * t // T) end at 1, 2, 3 and 7 threads on different rows; one line each way
SHAPES = ((1, 1), (1, 37), (37, 1), (7, 9), (21, 23), (39, 35))


def all_cases():
    for H, W in SHAPES:
        for name, a in K.cases(H, W):
            yield f"{H}x{W}-{name}", a


CASES = list(all_cases())


@pytest.fixture(scope="module")
def golden():
    return {(name, c): C.golden_components(a, c) for name, a in CASES for c in CONNS}


def test_golden_labels_equal_scipy(golden):
    pytest.importorskip("scipy")
    for name, a in CASES:
        for c in CONNS:
            ref, n = K.scipy_labels(a, c)
            got, gn = golden[(name, c)]
            assert gn == n, (name, c, gn, n)
            assert got.dtype == np.int32 and got.shape == a.shape
            assert (got == ref).all(), (name, c)


def test_known_counts():
    H, W = 21, 23
    cases = dict(K.cases(H, W))
    assert C.golden_components(cases["checkerboard"], 4)[1] == (W * H + 1) // 2
    assert C.golden_components(cases["checkerboard"], 8)[1] == 1
    assert C.golden_components(cases["background"], 8)[1] == 0
    assert C.golden_components(cases["foreground"], 4)[1] == 1
    assert C.golden_components(cases["corners"], 8)[1] == 4
    assert C.golden_components(cases["hstripes"], 8)[1] == (H + 1) // 2
    assert C.golden_components(cases["vstripes"], 8)[1] == (W + 1) // 2
    assert C.golden_components(cases["spiral"], 4)[1] == 1
    assert C.golden_components(cases["comb"], 4)[1] == 1
    assert C.golden_components(cases["u"], 4)[1] == 1
    # a diagonal line is one component only with the diagonals
    d = np.eye(9, dtype=np.uint8)
    assert C.golden_components(d, 4)[1] == 9 and C.golden_components(d, 8)[1] == 1
    lab, n = C.golden_components(np.array([[0, 3, 0, 1], [2, 0, 0, 1]], np.uint8), 4)
    assert n == 3 and lab.tolist() == [[0, 1, 0, 2], [3, 0, 0, 2]]


def test_stats_equal_scipy(golden):
    pytest.importorskip("scipy")
    for name, a in CASES:
        for c in CONNS:
            lab, n = golden[(name, c)]
            ref = K.numpy_stats(lab, n)
            got = C.component_stats(lab, n)
            assert got.dtype == np.int64 and got.shape == (n + 1, 7)
            assert (got == ref).all(), (name, c)
            assert (C.component_stats(lab, n, 3) == ref).all(), (name, c, "threaded")
            assert int(got[:, 0].sum()) == a.size
    # an empty label: only the background of an all-foreground frame
    lab, n = C.golden_components(np.full((3, 4), 9, np.uint8), 8)
    assert C.component_stats(lab, n).tolist() == [[0] * 7, [12, 0, 0, 4, 3, 18, 12]]
    with pytest.raises(RuntimeError, match="outside 0..0"):
        C.component_stats(lab, 0)


@pytest.mark.parametrize("threads", THREADS)
def test_cpu_components_equal_golden(golden, threads):
    for name, a in CASES:
        for c in CONNS:
            ref, n = golden[(name, c)]
            got, gn = C.cpu_components(a, c, threads)
            assert gn == n and (got == ref).all(), (name, c, threads)


def test_cpu_components_block_seams(golden):
    """Shapes whose components cross every row-block edge: a U with its arms either side of the edge's row."""
    H, W = 14, 11
    for threads in THREADS:
        for t in range(1, min(threads, H)):
            y = H * t // threads  # the block edge
            a = np.zeros((H, W), np.uint8)
            a[y - 1, 1:5] = 255
            a[y, 4:9] = 200       # N link across the edge
            a[y - 1, 9] = 7       # NE of (y, 8): joined only with the diagonals
            a[y, 0] = 1           # NW .. of nothing; W neighbour of (y-1, 1) by the diagonal
            for c in CONNS:
                ref, n = C.golden_components(a, c)
                got, gn = C.cpu_components(a, c, threads)
                assert gn == n and (got == ref).all(), (threads, t, c)
            assert C.golden_components(a, 8)[1] == 1 and C.golden_components(a, 4)[1] == 3


def test_area_filter_equal_numpy_mirror(golden):
    for name, a in CASES:
        for c in CONNS:
            lab, n = golden[(name, c)]
            for amin, amax in ((1, None), (2, None), (3, 9), (1, 1), (10 ** 6, None)):
                ref = K.numpy_area_filter(a, lab, n, amin, amax)
                hi = C.AREA_NO_LIMIT if amax is None else amax
                assert (C.golden_area_filter(a, c, amin, hi) == ref).all(), (name, c, amin, amax)
                assert (C.cpu_area_filter(a, c, amin, hi, 3) == ref).all(), (name, c, amin, amax)


def test_ops_containers_and_shapes():
    torch = pytest.importorskip("torch")
    a = K.random_mask(21, 23, 0.5, 5, value=128)
    ref, n = C.golden_components(a, 8)
    lab, gn = ops.label(a)
    assert isinstance(lab, np.ndarray) and lab.dtype == np.int32 and gn == n and (lab == ref).all()
    lab, gn = ops.label(torch.from_numpy(a), 4)
    ref4, n4 = C.golden_components(a, 4)
    assert isinstance(lab, torch.Tensor) and lab.dtype == torch.int32 and gn == n4 and (lab.numpy() == ref4).all()
    lab, gn = ops.label(a[:, :, None])
    assert lab.shape == a.shape and gn == n and (lab == ref).all()
    lab, gn = ops.label_reference(a, connectivity=4)
    assert gn == n4 and (lab == ref4).all()
    st = ops.component_stats(ref, n)
    assert isinstance(st, np.ndarray) and st.dtype == np.int64 and (st == C.component_stats(ref, n)).all()
    assert (ops.component_stats(torch.from_numpy(ref), n) == st).all()
    assert ops.STAT_COLUMNS == ("area", "x0", "y0", "x1", "y1", "sum_x", "sum_y")
    # the area filter keeps shape, dtype and container, and with the default bounds it is the identity
    for x in (a, a[:, :, None], torch.from_numpy(a), torch.from_numpy(a[:, :, None].copy())):
        y = ops.area_filter(x)
        assert type(y) is type(x) and y.shape == x.shape and y.dtype == x.dtype
        assert (np.asarray(y) == np.asarray(x)).all()
    for name in ("label", "label_reference", "component_stats", "area_filter", "remove_small_objects", "keep_largest"):
        assert name in ops.__all__ and callable(getattr(ops, name))


def test_ops_wrappers_equal_numpy_mirror():
    pytest.importorskip("scipy")
    for seed, d in enumerate(K.DENSITIES):
        a = K.random_mask(33, 29, d, 90 + seed, value=3)
        for c in CONNS:
            lab, n = K.scipy_labels(a, c)
            area = np.bincount(lab.ravel(), minlength=n + 1)
            assert (ops.remove_small_objects(a, 4, c) == K.numpy_area_filter(a, lab, n, 4)).all()
            top = int(area[1:].max())
            assert (ops.keep_largest(a, c) == K.numpy_area_filter(a, lab, n, top)).all()
            assert (ops.area_filter(a, 2, 5, c) == K.numpy_area_filter(a, lab, n, 2, 5)).all()
    z = np.zeros((5, 6), np.uint8)
    assert (ops.keep_largest(z) == 0).all() and ops.label(z)[1] == 0


def test_ops_refusals():
    a = np.zeros((6, 7), np.uint8)
    with pytest.raises(ValueError, match=r"needs a 1-channel image, got C = 3; convert first \(gray, threshold"):
        ops.label(np.zeros((6, 7, 3), np.uint8))
    with pytest.raises(RuntimeError, match=r"needs a 1-channel image, got C = 3; convert first"):
        C.golden_components(np.zeros((6, 7, 3), np.uint8), 8)
    with pytest.raises(TypeError, match="uint8"):
        ops.label(a.astype(np.int32))
    with pytest.raises(ValueError, match="connectivity must be 4 or 8, got 6"):
        ops.label(a, 6)
    with pytest.raises(RuntimeError, match="connectivity must be 4 or 8, got 6"):
        C.cpu_components(a, 6)
    with pytest.raises(ValueError, match="min_area must be at least 1, got 0"):
        ops.area_filter(a, min_area=0)
    with pytest.raises(RuntimeError, match="min_area must be at least 1, got 0"):
        C.cpu_area_filter(a, 8, 0, 5)
    with pytest.raises(ValueError, match="max_area 2 < min_area 3"):
        ops.area_filter(a, 3, 2)
    with pytest.raises(ValueError, match="min_area must be an integer"):
        ops.area_filter(a, 1.5)
    with pytest.raises(ValueError, match="one frame at a time"):
        ops.label(np.zeros((2, 6, 7, 1), np.uint8))
    with pytest.raises(ValueError, match="HxW or HxWx1"):
        ops.label(np.zeros((6, 7, 2), np.uint8))
    with pytest.raises(RuntimeError, match="connectivity must be 4 or 8, got '6'"):
        C.parse_connectivity("6")
    assert C.parse_connectivity("4") == 4 and C.components_tile() == (64, 64)


def run_cli(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


@pytest.mark.skipif(not os.path.exists(STRIPE), reason="bin/stripe not built")
def test_cli_label_on_the_host_backend(tmp_path):
    a = np.random.default_rng(4).integers(0, 256, (40, 52), dtype=np.uint8)
    a[10:30, 5:25] = 250  # one large object among the noise
    src, dst, stats = str(tmp_path / "a.pgm"), str(tmp_path / "mask.pgm"), str(tmp_path / "stats.json")
    C.write_pnm(src, a)
    chain = "threshold:128,open3"
    r = run_cli([STRIPE, "label", "--input", src, "--chain", chain, "--backend", "host", "--connectivity", "4",
                 "--min-area", "6", "--max-area", "1000", "--output", dst, "--stats", stats])
    assert r.returncode == 0, r.stderr
    mask = ops.apply(a, chain)
    lab, n = ops.label(mask, 4)
    assert r.stdout.strip() == str(n) and n > 1
    assert (C.read_pnm(dst) == ops.area_filter(mask, 6, 1000, 4)).all()
    with open(stats) as f:
        js = json.load(f)
    table = ops.component_stats(lab, n)
    assert js["n"] == n and js["connectivity"] == 4 and len(js["components"]) == n
    for l, e in enumerate(js["components"], 1):
        assert e == dict(label=l, area=int(table[l, 0]), bbox=[int(v) for v in table[l, 1:5]], sum_x=int(table[l, 5]),
                         sum_y=int(table[l, 6]))
    # the defaults: 8-connectivity, every area, no files
    r = run_cli([STRIPE, "label", "--input", src, "--chain", chain, "--backend", "host"])
    assert r.returncode == 0 and r.stdout.strip() == str(ops.label(mask)[1]), r.stderr
    # an RGB input without a conversion in the chain is refused
    rgb = str(tmp_path / "c.ppm")
    C.write_pnm(rgb, np.dstack([a, a, a]))
    r = run_cli([STRIPE, "label", "--input", rgb, "--chain", "invert", "--backend", "host"])
    assert r.returncode != 0 and "convert first" in r.stderr
    r = run_cli([STRIPE, "label", "--input", rgb, "--chain", "gray,threshold:128,open3", "--backend", "host"])
    assert r.returncode == 0, r.stderr
    r = run_cli([STRIPE, "label", "--input", src, "--connectivity", "6", "--backend", "host"])
    assert r.returncode != 0 and "connectivity must be 4 or 8" in r.stderr
