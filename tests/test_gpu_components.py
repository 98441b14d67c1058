"""k_ccl_* (csrc/hip/components.hip) on the GPU, exactly equal to the golden
functions: labels, n, the statistics table and the area filter on every frame of
components_cases at shapes derived from the kernel's tile (one pixel, one row,
one column, exactly a tile, a tile plus one, several tiles with a remainder, a
width that is no multiple of 4) and on a frame of about a million pixels;
pitched sources and label planes with guard values; determinism; a second
stream; the launch checks.  Only valid inputs: nothing here tries to reach the
step cap."""
import numpy as np
import pytest

import components_cases as K
import mpi_cuda_imagemanipulation_amd as m

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = m._C
ops = m.ops
TW, TH = C.components_tile()
CONNS = (4, 8)
SHAPES = ((1, 1), (1, 5 * TW + 3), (5 * TH + 3, 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 3, 3 * TW + 5),
          (TH + 7, 2 * TW + 2))
assert SHAPES[-1][1] % 4 != 0  # one width that is no multiple of 4
BIG = (1000, 1049)  # about a million pixels: 16 x 17 tiles, rows of 5 segments
BOUNDS = ((2, None), (3, 40))

_frames = {}
_golden = {}


def frames(shape):
    if shape not in _frames:
        _frames[shape] = dict(K.cases(shape[0], shape[1], seam=TW))
    return _frames[shape]


def golden(shape, name, conn):
    """(labels, n, stats) of the golden functions, computed once."""
    key = (shape, name, conn)
    if key not in _golden:
        lab, n = C.golden_components(frames(shape)[name], conn)
        _golden[key] = (lab, n, C.component_stats(lab, n))
    return _golden[key]


def check_frame(shape, name):
    a = frames(shape)[name]
    x = torch.from_numpy(a).cuda()
    for conn in CONNS:
        ref, n, table = golden(shape, name, conn)
        lab, gn = ops.label(x, conn)
        assert lab.is_cuda and lab.dtype == torch.int32 and tuple(lab.shape) == a.shape
        got = lab.cpu().numpy()
        assert gn == n, (shape, name, conn, gn, n)
        assert (got == ref).all(), (shape, name, conn, int((got != ref).sum()))
        st = ops.component_stats(lab, gn)
        assert st.dtype == np.int64 and st.shape == table.shape and (st == table).all(), (shape, name, conn)
        for amin, amax in BOUNDS:
            want = C.golden_area_filter(a, conn, amin, C.AREA_NO_LIMIT if amax is None else amax)
            out = ops.area_filter(x, amin, amax, conn)
            assert out.is_cuda and out.dtype == torch.uint8 and (out.cpu().numpy() == want).all(), (shape, name, conn, amin)


CASE_NAMES = [name for name, _ in K.cases(3, 3)]


def test_tile_constants():
    assert (TW, TH) == (64, 64)
    assert C.components_lds() == dict(k_ccl_tile=TW * TH * 4, k_ccl_number=16, k_ccl_scan=1024)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_frame(shape):
    for name in CASE_NAMES:
        check_frame(shape, name)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_million_pixels(name):
    check_frame(BIG, name)


def test_known_counts_on_the_device():
    H, W = 2 * TH + 3, 3 * TW + 5
    f = frames((H, W))
    n_of = lambda name, conn: ops.label(torch.from_numpy(f[name]).cuda(), conn)[1]
    assert n_of("checkerboard", 4) == (W * H + 1) // 2 and n_of("checkerboard", 8) == 1
    assert n_of("background", 8) == 0 and n_of("foreground", 4) == 1
    assert n_of("spiral", 4) == 1 and n_of("comb", 4) == 1 and n_of("u", 4) == 1 and n_of("border", 4) == 1


def test_pitched_source_and_label_plane():
    H, W = 2 * TH + 3, 3 * TW + 5
    a = K.random_mask(H, W, 0.55, 11, value=9)
    wide = torch.full((H, W + 16), 255, dtype=torch.uint8, device="cuda")  # foreground guard columns, odd pitch
    assert wide.stride(0) % 2 == 1
    view = wide[:, 3:3 + W]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 2 == 1 and not view.is_contiguous()
    for conn in CONNS:
        ref, n = C.golden_components(a, conn)
        lab, gn = ops.label(view, conn)
        lab2, gn2 = ops.label(view.contiguous(), conn)
        assert gn == gn2 == n and torch.equal(lab, lab2) and (lab.cpu().numpy() == ref).all()
        # the raw binding into a wider label plane: nothing outside a row's W ints is written
        plane = torch.full((H, W + 5), -7, dtype=torch.int32, device="cuda")
        gn3 = C.components_device(view.data_ptr(), view.stride(0), W, H, conn, plane.data_ptr(), W + 5,
                                  torch.cuda.current_stream().cuda_stream)
        p = plane.cpu().numpy()
        assert gn3 == n and (p[:, :W] == ref).all() and (p[:, W:] == -7).all()
        # the table and the filter from the pitched plane
        table = torch.empty((n + 1, 7), dtype=torch.int64, device="cuda")
        C.component_stats_device(plane.data_ptr(), W + 5, W, H, n, table.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert (table.cpu().numpy() == C.component_stats(ref, n)).all()
        out = torch.full((H, W + 3), 77, dtype=torch.uint8, device="cuda")
        C.area_filter_device(view.data_ptr(), view.stride(0), W, H, plane.data_ptr(), W + 5, table.data_ptr(), n, 2, 30,
                             out.data_ptr(), W + 3, torch.cuda.current_stream().cuda_stream)
        o = out.cpu().numpy()
        assert (o[:, :W] == C.golden_area_filter(a, conn, 2, 30)).all() and (o[:, W:] == 77).all()
    assert (wide.cpu().numpy()[:, :3] == 255).all() and (wide.cpu().numpy()[:, 3 + W:] == 255).all()


def test_two_runs_are_identical():
    x = torch.from_numpy(frames(BIG)["random0.593"]).cuda()
    for conn in CONNS:
        l1, n1 = ops.label(x, conn)
        l2, n2 = ops.label(x, conn)
        assert n1 == n2 and torch.equal(l1, l2)
        assert (ops.component_stats(l1, n1) == ops.component_stats(l2, n2)).all()


def test_second_stream():
    shape = (2 * TH + 3, 3 * TW + 5)
    a = frames(shape)["random0.5"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.from_numpy(a).cuda()
        lab, n = ops.label(x, 8)
        st = ops.component_stats(lab, n)
        out = ops.area_filter(x, 3, None, 8)
    s.synchronize()
    ref, rn, table = golden(shape, "random0.5", 8)
    assert n == rn and (lab.cpu().numpy() == ref).all() and (st == table).all()
    assert (out.cpu().numpy() == C.golden_area_filter(a, 8, 3, C.AREA_NO_LIMIT)).all()


def test_front_end_shapes_and_wrappers():
    a = K.random_mask(TH + 1, TW + 1, 0.5, 3, value=2)
    x = torch.from_numpy(a).cuda()
    lab, n = ops.label(x[:, :, None])
    ref, rn = C.golden_components(a, 8)
    assert tuple(lab.shape) == a.shape and n == rn and (lab.cpu().numpy() == ref).all()
    y = ops.area_filter(x[:, :, None])
    assert tuple(y.shape) == a.shape + (1,) and torch.equal(y[:, :, 0], x)
    assert (ops.remove_small_objects(x, 5).cpu().numpy() == ops.remove_small_objects(a, 5)).all()
    assert (ops.keep_largest(x, 4).cpu().numpy() == ops.keep_largest(a, 4)).all()
    with pytest.raises(ValueError, match="convert first"):
        ops.label(torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError, match="uint8"):
        ops.label(torch.zeros((4, 4), dtype=torch.int32, device="cuda"))


def test_launch_checks():
    x = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    lab = torch.full((8, 8), -3, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="null src or labels"):
        C.components_device(0, 8, 8, 8, 8, lab.data_ptr(), 8, s)
    with pytest.raises(RuntimeError, match="null src or labels"):
        C.components_device(x.data_ptr(), 8, 8, 8, 8, 0, 8, s)
    with pytest.raises(RuntimeError, match="labels_pitch 7 < the row's 8 elements"):
        C.components_device(x.data_ptr(), 8, 8, 8, 8, lab.data_ptr(), 7, s)
    with pytest.raises(RuntimeError, match="src_pitch 7 < row bytes 8"):
        C.components_device(x.data_ptr(), 7, 8, 8, 8, lab.data_ptr(), 8, s)
    with pytest.raises(RuntimeError, match=r"exceed 2\^31 - 2"):
        C.components_device(x.data_ptr(), 65536, 65536, 32768, 8, lab.data_ptr(), 65536, s)
    with pytest.raises(RuntimeError, match="connectivity must be 4 or 8, got 6"):
        C.components_device(x.data_ptr(), 8, 8, 8, 6, lab.data_ptr(), 8, s)
    with pytest.raises(RuntimeError, match="aligned to 4 bytes"):
        C.components_device(x.data_ptr(), 8, 8, 7, 8, lab.data_ptr() + 2, 8, s)
    torch.cuda.synchronize()
    assert (lab.cpu().numpy() == -3).all()  # refused before any launch


def test_cli_label_on_the_device_backend(tmp_path):
    import json
    import os
    import subprocess

    stripe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "stripe")
    if not os.path.exists(stripe):
        pytest.skip("bin/stripe not built")
    a = np.random.default_rng(8).integers(0, 256, (2 * TH + 3, 3 * TW + 5), dtype=np.uint8)
    a[20:90, 30:150] = 240
    src, dst, stats = str(tmp_path / "a.pgm"), str(tmp_path / "mask.pgm"), str(tmp_path / "stats.json")
    C.write_pnm(src, a)
    chain = "threshold:128,open3"
    r = subprocess.run([stripe, "label", "--input", src, "--chain", chain, "--backend", "device", "--min-area", "4",
                        "--output", dst, "--stats", stats], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mask = ops.reference(a, chain)
    lab, n = C.golden_components(mask, 8)
    assert r.stdout.strip() == str(n) and n > 1
    assert (C.read_pnm(dst) == C.golden_area_filter(mask, 8, 4, C.AREA_NO_LIMIT)).all()
    with open(stats) as f:
        js = json.load(f)
    table = C.component_stats(lab, n)
    assert js["n"] == n and [e["area"] for e in js["components"]] == table[1:, 0].tolist()
    assert [e["bbox"] for e in js["components"]] == table[1:, 1:5].tolist()
