"""k_canny_* (csrc/hip/canny.hip) and the forest passes of k_ccl_* on the GPU,
exactly equal to the golden functions: the edge map and the class plane on every
frame of canny_cases under every border and norm, at shapes derived from the
kernels' constants (one pixel, one row, one column, exactly one tile, one more
pixel in each direction, several tiles with a remainder, a width that is no
multiple of 4, 65 x 257); hysteresis_threshold on spiral masks that cross at
least three forest tiles in each direction, at both connectivities; pitched
odd-aligned sources with guard values around the destination; determinism; a
second stream; alternating sizes and clear_cache; the front end's shapes; the
launch checks; the CLI.  The reference is golden_canny where its loop is
affordable and cpu_canny, which tests/test_canny.py ties to it and to numpy,
elsewhere.  Only valid inputs."""
import numpy as np
import pytest

import canny_cases as CC
import mpi_cuda_imagemanipulation_amd as m
import np_canny as NC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = m._C
ops = m.ops
TX, TY = C.canny_tile()
CT = C.components_tile()[0]  # the forest's tile
ONE = (TY, TX)
MORE = (TY + 1, TX + 1)
MANY = (2 * TY + 3, 3 * TX + 5)
SMALL = ((1, 1), (1, 5 * TX + 3), (5 * TY + 3, 1), ONE, MORE, MANY, (CT + 1, CT + 2), (65, 257))
assert MANY[1] % 4 != 0 and SMALL[1][1] % 4 != 0 and (65, 257)[1] % 4 != 0  # widths that are no multiple of 4
THRESHOLDS = ((40, 100), (100, 300), (0, 0), (2040, 2040))

_frames = {}
_ref = {}


def frames(shape):
    if shape not in _frames:
        _frames[shape] = dict(CC.frames(*shape))
    return _frames[shape]


def reference(shape, name, low, high, norm, border, classes=False):
    """Computed once: the golden loop where it is affordable, the host executor elsewhere."""
    key = (shape, name, low, high, norm, border, classes)
    if key not in _ref:
        a = frames(shape)[name]
        if shape[0] * shape[1] <= 1 << 16:
            fn = C.golden_canny_classes if classes else C.golden_canny
            _ref[key] = fn(a, low, high, norm, border)
        else:
            fn = C.cpu_canny_classes if classes else C.cpu_canny
            _ref[key] = fn(a, low, high, norm, border, 8)
    return _ref[key]


def check(shape, names, thresholds=THRESHOLDS[:1], borders=NC.BORDERS, norms=NC.NORMS):
    for name in names:
        x = torch.from_numpy(frames(shape)[name]).cuda()
        for border in borders:
            for norm in norms:
                for low, high in thresholds:
                    key = (shape, name, border, norm, low, high)
                    got = ops.canny(x, low, high, norm, border)
                    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == shape
                    g = got.cpu().numpy()
                    want = reference(shape, name, low, high, norm, border)
                    assert (g == want).all(), key + (int((g != want).sum()),)
                    c = ops.canny_classes(x, low, high, norm, border).cpu().numpy()
                    want = reference(shape, name, low, high, norm, border, True)
                    assert (c == want).all(), key + ("classes", int((c != want).sum()))


def test_constants():
    assert (TX, TY) == (64, 32) and CT == 64
    lds = C.canny_lds()
    assert set(lds) == {"k_canny_nms", "k_canny_classify", "k_canny_mark", "k_canny_select"}
    assert lds["k_canny_nms"] == (TX + 4) * (TY + 4) + 4 * (TX + 2) * (TY + 2)


@pytest.mark.parametrize("low,high", THRESHOLDS)
def test_every_frame_border_and_norm(low, high):
    check(MORE, CC.NAMES, ((low, high),))


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(shape):
    check(shape, ("random", "blur_random", "blur_text", "ring", "bar45up", "step90down", "all255"), THRESHOLDS[:2])


def test_several_forest_tiles():
    check((3 * CT + 7, 3 * CT + 9), ("blur_random", "blur_text", "ring"), THRESHOLDS[:1], ("reflect101",))


@pytest.mark.parametrize("shape", ((3 * CT + 8, 3 * CT + 8), (2 * CT + 1, 3 * CT + 5)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_spirals_across_forest_tiles(shape):
    H, W = shape
    a, path, _ = CC.spiral(H, W)
    b, _, _ = CC.spiral(H, W, strong=False)
    g, gpath, k = CC.spiral(H, W, gap=True)
    want = np.where(a > 0, 255, 0).astype(np.uint8)
    want_gap = np.zeros((H, W), np.uint8)
    for y, x in gpath[k + 1:]:
        want_gap[y, x] = 255
    stairs = CC.staircase(H, W)
    first = np.zeros((H, W), np.uint8)
    first[0, 0] = 255
    for conn in (4, 8):
        for src, ref in ((a, want), (b, np.zeros_like(want)), (g, want_gap),
                         (stairs, first if conn == 4 else np.where(stairs > 0, 255, 0).astype(np.uint8))):
            assert (C.golden_hysteresis_threshold(src, 50, 150, conn) == ref).all()
            got = ops.hysteresis_threshold(torch.from_numpy(src).cuda(), 50, 150, conn)
            assert got.is_cuda and got.dtype == torch.uint8 and (got.cpu().numpy() == ref).all(), (shape, conn)


def test_hysteresis_threshold_on_frames():
    for shape in (MORE, MANY, (1, 5 * TX + 3), (5 * TY + 3, 1), (1, 1)):
        for name in ("random", "blur_random", "blur_text", "checker", "all255", "flat0"):
            a = frames(shape)[name]
            x = torch.from_numpy(a).cuda()
            for low, high in ((0, 0), (100, 150), (128, 254), (255, 255)):
                for conn in (4, 8):
                    want = C.cpu_hysteresis_threshold(a, low, high, conn, 8)
                    got = ops.hysteresis_threshold(x, low, high, conn).cpu().numpy()
                    assert (got == want).all(), (shape, name, low, high, conn)


def test_pitched_source_and_destination_planes():
    H, W = MANY
    a = frames(MANY)["blur_random"]
    wide = torch.full((H, W + 16), 255, dtype=torch.uint8, device="cuda")  # guard columns, odd pitch
    assert wide.stride(0) % 2 == 1
    view = wide[:, 3:3 + W]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 2 == 1 and not view.is_contiguous()
    s = torch.cuda.current_stream().cuda_stream
    assert (ops.canny(view, 40, 100).cpu().numpy() == reference(MANY, "blur_random", 40, 100, "l1", "reflect101")).all()
    assert (ops.hysteresis_threshold(view, 100, 150).cpu().numpy() == C.cpu_hysteresis_threshold(a, 100, 150, 8, 8)).all()
    # the raw bindings into wider planes at an odd address and pitch, and at an aligned one: nothing outside a row's
    # bytes is written
    for off, pad in ((1, 3), (0, 4)):
        for call, want in (
                (lambda d, dp: C.canny_device(view.data_ptr(), view.stride(0), W, H, 40, 100, "l2", "replicate", d, dp, s),
                 reference(MANY, "blur_random", 40, 100, "l2", "replicate")),
                (lambda d, dp: C.canny_classes_device(view.data_ptr(), view.stride(0), W, H, 40, 100, "l1", "constant", d, dp, s),
                 reference(MANY, "blur_random", 40, 100, "l1", "constant", True)),
                (lambda d, dp: C.hysteresis_device(view.data_ptr(), view.stride(0), W, H, 100, 150, 4, d, dp, s),
                 C.cpu_hysteresis_threshold(a, 100, 150, 4, 8))):
            out = torch.full((H * (W + pad) + off,), 77, dtype=torch.uint8, device="cuda")
            call(out.data_ptr() + off, W + pad)
            o = out.cpu().numpy()
            rows = o[off:].reshape(H, W + pad)
            assert (rows[:, :W] == want).all() and (rows[:, W:] == 77).all() and (o[:off] == 77).all(), (off, pad)
    g = wide.cpu().numpy()
    assert (g[:, :3] == 255).all() and (g[:, 3 + W:] == 255).all() and (g[:, 3:3 + W] == a).all()


def test_two_runs_are_identical():
    x = torch.from_numpy(frames(MANY)["blur_text"]).cuda()
    assert torch.equal(ops.canny(x, 40, 100), ops.canny(x, 40, 100))
    assert torch.equal(ops.canny(x, 40, 100, "l2"), ops.canny(x, 40, 100, "l2"))
    assert torch.equal(ops.hysteresis_threshold(x, 100, 150, 4), ops.hysteresis_threshold(x, 100, 150, 4))


def test_second_stream():
    a = frames(MANY)["blur_text"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.from_numpy(a).cuda()
        e = ops.canny(x, 40, 100, "l2", "replicate")
        c = ops.canny_classes(x, 40, 100)
        h = ops.hysteresis_threshold(x, 100, 150)
    s.synchronize()
    assert (e.cpu().numpy() == reference(MANY, "blur_text", 40, 100, "l2", "replicate")).all()
    assert (c.cpu().numpy() == reference(MANY, "blur_text", 40, 100, "l1", "reflect101", True)).all()
    assert (h.cpu().numpy() == C.cpu_hysteresis_threshold(a, 100, 150, 8, 8)).all()


def test_alternating_sizes_and_clear_cache():
    """Sizes in turn: the scratch cache serves each its own planes, evicts the oldest, and starts again after
    clear_cache."""
    shapes = (MORE, MANY, ONE, (65, 257), (1, 5 * TX + 3), MORE)
    xs = {shape: torch.from_numpy(frames(shape)["blur_random"]).cuda() for shape in shapes}
    got = [(shape, ops.canny(xs[shape], 40, 100), ops.hysteresis_threshold(xs[shape], 100, 150)) for _ in range(2)
           for shape in shapes]
    for shape, e, h in got:
        assert (e.cpu().numpy() == reference(shape, "blur_random", 40, 100, "l1", "reflect101")).all(), shape
        assert (h.cpu().numpy() == C.cpu_hysteresis_threshold(frames(shape)["blur_random"], 100, 150, 8, 8)).all(), shape
    ops.clear_cache()  # releases the scratch; the next call allocates again
    assert (ops.canny(xs[MANY], 40, 100).cpu().numpy() == reference(MANY, "blur_random", 40, 100, "l1", "reflect101")).all()
    # labelling shares the forest passes and its words: still what it was
    lab, n = ops.label(xs[MANY])
    want, wn = C.cpu_components(frames(MANY)["blur_random"], 8)
    assert n == wn and (lab.cpu().numpy() == want).all()


def test_front_end_shapes():
    a = frames(MORE)["blur_text"]
    x = torch.from_numpy(a).cuda()
    want = reference(MORE, "blur_text", 40, 100, "l1", "reflect101")
    y = ops.canny(x[:, :, None], np.int64(40), 100.0)
    assert tuple(y.shape) == MORE + (1,) and (y[:, :, 0].cpu().numpy() == want).all()
    h = ops.hysteresis_threshold(x[:, :, None], 100, 150)
    assert tuple(h.shape) == MORE + (1,)
    t = ops.canny(x.t().contiguous().t(), 40, 100)  # rows not packed: made contiguous
    assert (t.cpu().numpy() == want).all()
    with pytest.raises(ValueError, match="convert first"):
        ops.canny(torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda"), 1, 2)
    with pytest.raises(TypeError, match="uint8"):
        ops.canny(torch.zeros((4, 4), dtype=torch.int32, device="cuda"), 1, 2)
    with pytest.raises(ValueError, match="0 <= low <= high <= 2040"):
        ops.canny(x, 5, 3)
    with pytest.raises(ValueError, match="0 <= low <= high <= 255"):
        ops.hysteresis_threshold(x, 5, 256)


def test_launch_checks():
    x = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    u = torch.full((8, 8), 9, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def canny(fn=C.canny_device, src=x.data_ptr(), sp=8, W=8, H=8, low=1, high=2, norm="l1", border="reflect101",
              dst=u.data_ptr(), dp=8):
        fn(src, sp, W, H, low, high, norm, border, dst, dp, s)

    def hyst(src=x.data_ptr(), sp=8, W=8, H=8, low=1, high=2, conn=8, dst=u.data_ptr(), dp=8):
        C.hysteresis_device(src, sp, W, H, low, high, conn, dst, dp, s)

    cases = (({"src": 0}, "null src or dst"), ({"dst": 0}, "null src or dst"), ({"sp": 7}, "src_pitch 7 < row bytes 8"),
             ({"dp": 7}, "dst_pitch 7 < row bytes 8"), ({"W": 0}, "empty image"), ({"H": 0}, "empty image"),
             ({"W": 1 << 16, "H": 1 << 15, "sp": 1 << 16, "dp": 1 << 16}, "pixels exceed"),
             ({"low": 3, "high": 2}, "0 <= low <= high"), ({"low": -1}, "0 <= low <= high"))
    for fn in (C.canny_device, C.canny_classes_device):
        for kwargs, msg in cases + (({"high": 2041}, "0 <= low <= high <= 2040"), ({"border": "skip"}, "reflect101, replicate or constant"),
                                    ({"norm": "linf"}, "the norm must be l1 or l2")):
            with pytest.raises(RuntimeError, match=msg):
                canny(fn, **kwargs)
    for kwargs, msg in cases + (({"high": 256}, "0 <= low <= high <= 255"), ({"conn": 6}, "connectivity must be 4 or 8")):
        with pytest.raises(RuntimeError, match=msg):
            hyst(**kwargs)
    torch.cuda.synchronize()
    assert (u.cpu().numpy() == 9).all()  # refused before any launch


def test_cli_edges_on_the_device_backend(tmp_path):
    import os
    import subprocess

    stripe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "stripe")
    if not os.path.exists(stripe):
        pytest.skip("bin/stripe not built")
    a = frames(MANY)["blur_text"]
    src = str(tmp_path / "a.pgm")
    C.write_pnm(src, a)
    for extra in (["--low", "40", "--high", "100"], ["--low", "20", "--high", "60", "--chain", "gaussian5", "--norm", "l2"],
                  ["--low", "40", "--high", "100", "--border", "replicate"]):
        outs = {}
        for backend in ("host", "device"):
            dst = str(tmp_path / f"{backend}.pgm")
            r = subprocess.run([stripe, "edges", "--input", src, "--backend", backend, "--output", dst] + extra,
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            outs[backend] = (C.read_pnm(dst), r.stdout)
        assert (outs["host"][0] == outs["device"][0]).all() and outs["host"][1] == outs["device"][1], extra
    assert (outs["host"][0] == C.cpu_canny(a, 40, 100, "l1", "replicate", 8)).all()
