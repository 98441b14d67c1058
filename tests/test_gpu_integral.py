"""k_sat_* (csrc/hip/integral.hip) on the GPU, exactly equal to the golden
functions: the integral and its squares (the 300 x 300 wrap included) against
the numpy tables, and every window operation under every border at K in
{1, 3, 5, 31, 255} on every frame of integral_cases, at shapes derived from the
kernels' constants (one pixel, one row, one column, exactly a workgroup's tiles,
one more in each direction, several with a remainder and a width that is no
multiple of 4, both side limits), a window whose radius exceeds the frame, and
K = 4095 on a tiny frame; pitched odd-aligned sources and destinations with guard
values; determinism; a second stream; alternating sizes and windows; the front
end's shapes; the launch checks; the CLI.  The reference is golden_window where
its loop is affordable and cpu_window, which tests/test_integral.py ties to it
and to numpy, elsewhere.  Only valid inputs."""
import numpy as np
import pytest

import integral_cases as IC
import mpi_cuda_imagemanipulation_amd as m
import np_integral as NI

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = m._C
ops = m.ops
T, WV, PX = C.integral_tile()
TW = T * WV  # a workgroup's columns
SMALL = ((1, 1), (1, 5 * TW + 3), (5 * T + 3, 1), (T, TW), (T + 1, TW + 1), (2 * T + 3, 3 * TW + 5))
LONG = ((3, C.INTEGRAL_MAX_SIDE), (C.INTEGRAL_MAX_SIDE, 3))
assert SMALL[5][1] % 4 != 0 and SMALL[1][1] % 4 != 0  # widths that are no multiple of 4
KS = (1, 3, 5, 31, 255)
VARIANTS = (("box", 0, None), ("std", 0, None), ("mean", 0, None), ("mean", 7, None), ("mean", -10, None),
            ("niblack", 0, 0.2), ("niblack", 5, -0.2), ("sauvola", 0, 0.2), ("sauvola", 0, 0.34), ("sauvola", 0, -0.5))
OP = {name: k for k, name in enumerate(C.WINDOW_OPS)}

_frames = {}
_ref = {}


def frames(shape):
    if shape not in _frames:
        _frames[shape] = dict(IC.cases(shape[0], shape[1]))
    return _frames[shape]


def reference(shape, name, op, K, border, c, k):
    """Computed once: the golden loop where it is affordable, the host executor elsewhere."""
    key = (shape, name, op, K, border, c, k)
    if key not in _ref:
        a = frames(shape)[name]
        kk = 0.0 if k is None else k
        if (shape[0] + K) * shape[1] * K <= 4e6:
            _ref[key] = C.golden_window(a, op, K, border, c, kk)
        else:
            _ref[key] = C.cpu_window(a, op, K, border, c, kk)
    return _ref[key]


def device_window(x, op, K, border, c, k):
    if op == "box":
        return ops.box_filter(x, K, border)
    if op == "std":
        return ops.local_std(x, K, border)
    return ops.local_threshold(x, K, op, c, k, border)


def check(shape, names, ks, variants=VARIANTS):
    for name in names:
        x = torch.from_numpy(frames(shape)[name]).cuda()
        for border in NI.BORDERS:
            for K in ks:
                for op, c, k in variants:
                    got = device_window(x, op, K, border, c, k)
                    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == shape
                    want = reference(shape, name, op, K, border, c, k)
                    g = got.cpu().numpy()
                    assert (g == want).all(), (shape, name, border, K, op, c, k, int((g != want).sum()))


def test_constants():
    assert (T, WV, PX) == (64, 4, 4)
    assert set(C.integral_lds()) == {"k_sat_reduce", "k_sat_carry", "k_sat_scan", "k_sat_window"}


@pytest.mark.parametrize("K", KS)
def test_every_frame_border_and_operation(K):
    check((T + 1, TW + 1), IC.NAMES, (K,))


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(shape):
    check(shape, ("random", "text", "all255"), (1, 5, 31, 255))  # 31 and 255 on 1x1: the radius exceeds the frame


@pytest.mark.parametrize("shape", LONG, ids=lambda s: f"{s[0]}x{s[1]}")
def test_side_limits(shape):
    check(shape, ("random",), (1, 31, 255), (("box", 0, None), ("std", 0, None), ("mean", 7, None), ("sauvola", 0, 0.2)))


def test_radius_above_the_frame_and_the_largest_window():
    check((5, 7), IC.NAMES, (31, 255))
    a = frames((5, 7))["random"]
    x = torch.from_numpy(a).cuda()
    for border in NI.BORDERS:
        assert (ops.box_filter(x, 4095, border).cpu().numpy() == C.golden_window(a, "box", 4095, border, 0, 0.0)).all()
    ops.clear_cache()  # the 4095 tables are large


@pytest.mark.parametrize("shape", SMALL + ((300, 300),) + LONG, ids=lambda s: f"{s[0]}x{s[1]}")
def test_integral_and_squares(shape):
    names = ("all255",) if shape == (300, 300) else ("random", "all255", "flat1")
    for name in names:
        a = frames(shape)[name]
        x = torch.from_numpy(a).cuda()
        for sq in (False, True):
            got = ops.integral(x, squared=sq)
            assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (shape[0] + 1, shape[1] + 1)
            assert (got.cpu().numpy() == NI.integral(a, sq)).all(), (shape, name, sq)
    if shape == (300, 300):
        assert 255 * 255 * 300 * 300 >= 2 ** 32  # the squares table has wrapped


def test_pitched_source_and_destination_planes():
    H, W = 2 * T + 3, 3 * TW + 5
    a = frames((H, W))["random"]
    wide = torch.full((H, W + 16), 255, dtype=torch.uint8, device="cuda")  # guard columns, odd pitch
    assert wide.stride(0) % 2 == 1
    view = wide[:, 3:3 + W]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 2 == 1 and not view.is_contiguous()
    s = torch.cuda.current_stream().cuda_stream
    assert (ops.box_filter(view, 31).cpu().numpy() == reference((H, W), "random", "box", 31, "reflect101", 0, None)).all()
    assert (ops.integral(view).cpu().numpy() == NI.integral(a)).all()
    # the raw bindings into wider planes: nothing outside a row's elements is written
    for sq in (False, True):
        plane = torch.full((H + 1, W + 6), -7, dtype=torch.int32, device="cuda")
        C.integral_device(view.data_ptr(), view.stride(0), W, H, sq, plane.data_ptr(), W + 6, s)
        p = plane.cpu().numpy()
        assert (p[:, :W + 1] == NI.integral(a, sq)).all() and (p[:, W + 1:] == -7).all(), sq
    for op, c, k in VARIANTS:
        for border in ("reflect101", "constant"):
            # an odd destination address and pitch too
            out = torch.full((H * (W + 3) + 1,), 77, dtype=torch.uint8, device="cuda")
            C.window_device(view.data_ptr(), view.stride(0), W, H, OP[op], 15, border, c, C.window_kq(k or 0.0),
                            out.data_ptr() + 1, W + 3, s)
            o = out.cpu().numpy()[1:].reshape(H, W + 3)
            want = reference((H, W), "random", op, 15, border, c, k)
            assert (o[:, :W] == want).all() and (o[:, W:] == 77).all() and out[0].item() == 77, (op, border)
    g = wide.cpu().numpy()
    assert (g[:, :3] == 255).all() and (g[:, 3 + W:] == 255).all()


def test_two_runs_are_identical():
    x = torch.from_numpy(frames((2 * T + 3, 3 * TW + 5))["text"]).cuda()
    assert torch.equal(ops.local_threshold(x, 31, "sauvola"), ops.local_threshold(x, 31, "sauvola"))
    assert torch.equal(ops.integral(x, True), ops.integral(x, True))


def test_second_stream():
    shape = (2 * T + 3, 3 * TW + 5)
    a = frames(shape)["text"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.from_numpy(a).cuda()
        b = ops.box_filter(x, 31)
        t = ops.local_threshold(x, 31, "sauvola", border="replicate")
        i = ops.integral(x)
    s.synchronize()
    assert (b.cpu().numpy() == reference(shape, "text", "box", 31, "reflect101", 0, None)).all()
    assert (t.cpu().numpy() == reference(shape, "text", "sauvola", 31, "replicate", 0, 0.2)).all()
    assert (i.cpu().numpy() == NI.integral(a)).all()


def test_alternating_sizes_and_windows():
    """Sizes and windows in turn, queued without waiting: the scratch cache serves each its own buffers."""
    jobs = (((T + 1, TW + 1), "box", 5), ((2 * T + 3, 3 * TW + 5), "std", 31), ((T + 1, TW + 1), "sauvola", 31),
            ((T, TW), "mean", 255), ((T + 1, TW + 1), "box", 31))
    xs = {shape: torch.from_numpy(frames(shape)["random"]).cuda() for shape, _, _ in jobs}
    got = [(j, device_window(xs[j[0]], j[1], j[2], "reflect101", 0, None)) for _ in range(3) for j in jobs]
    ints = [ops.integral(xs[jobs[0][0]]) for _ in range(2)]
    for (shape, op, K), y in got:
        k = 0.2 if op == "sauvola" else None
        assert (y.cpu().numpy() == reference(shape, "random", op, K, "reflect101", 0, k)).all(), (shape, op, K)
    ops.clear_cache()  # releases the scratch; the next call allocates again
    shape, op, K = jobs[0]
    assert (ops.box_filter(xs[shape], K).cpu().numpy() == reference(shape, "random", op, K, "reflect101", 0, None)).all()
    assert all((i.cpu().numpy() == NI.integral(frames(shape)["random"])).all() for i in ints)


def test_front_end_shapes():
    shape = (T + 1, TW + 1)
    a, b = frames(shape)["text"], frames(shape)["random"]
    x = torch.from_numpy(a).cuda()
    want = reference(shape, "text", "mean", 31, "reflect101", 7, None)
    y = ops.local_threshold(x[:, :, None], 31, c=7)
    assert tuple(y.shape) == shape + (1,) and (y[:, :, 0].cpu().numpy() == want).all()
    batch = torch.from_numpy(np.stack([a, b])[:, :, :, None]).cuda()
    z = ops.local_threshold(batch, 31, c=7)
    assert tuple(z.shape) == (2,) + shape + (1,) and (z[0, :, :, 0].cpu().numpy() == want).all()
    assert (z[1, :, :, 0].cpu().numpy() == reference(shape, "random", "mean", 31, "reflect101", 7, None)).all()
    assert (ops.integral(x[:, :, None]).cpu().numpy() == NI.integral(a)).all()
    with pytest.raises(ValueError, match="convert first"):
        ops.box_filter(torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda"), 3)
    with pytest.raises(TypeError, match="uint8"):
        ops.box_filter(torch.zeros((4, 4), dtype=torch.int32, device="cuda"), 3)
    with pytest.raises(ValueError, match="window must be odd"):
        ops.box_filter(x, 4)


def test_launch_checks():
    x = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    d = torch.full((9, 9), -3, dtype=torch.int32, device="cuda")
    u = torch.full((8, 8), 9, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="null src or dst"):
        C.integral_device(0, 8, 8, 8, False, d.data_ptr(), 9, s)
    with pytest.raises(RuntimeError, match="null src or dst"):
        C.integral_device(x.data_ptr(), 8, 8, 8, False, 0, 9, s)
    with pytest.raises(RuntimeError, match="dst_pitch 8 < the row's 9 elements"):
        C.integral_device(x.data_ptr(), 8, 8, 8, False, d.data_ptr(), 8, s)
    with pytest.raises(RuntimeError, match="src_pitch 7 < row bytes 8"):
        C.integral_device(x.data_ptr(), 7, 8, 8, False, d.data_ptr(), 9, s)
    with pytest.raises(RuntimeError, match="aligned to 4 bytes"):
        C.integral_device(x.data_ptr(), 8, 8, 7, False, d.data_ptr() + 2, 9, s)
    with pytest.raises(RuntimeError, match="side above 32767"):
        C.integral_device(x.data_ptr(), 32768, 32768, 8, False, d.data_ptr(), 32769, s)

    def window(op=0, K=3, border="reflect101", c=0, kq=0, src=x.data_ptr(), sp=8, W=8, H=8, dst=u.data_ptr(), dp=8):
        C.window_device(src, sp, W, H, op, K, border, c, kq, dst, dp, s)

    for kwargs, msg in (({"src": 0}, "null src or dst"), ({"dst": 0}, "null src or dst"),
                        ({"sp": 7}, "src_pitch 7 < row bytes 8"), ({"dp": 7}, "dst_pitch 7 < row bytes 8"),
                        ({"H": 32768}, "side above 32767"), ({"W": 0}, "empty image"),
                        ({"K": 4}, "window must be odd"), ({"K": 0}, "window must be odd"),
                        ({"K": 4097}, "is above 4095, the limit of box"),
                        ({"op": OP["std"], "K": 257}, "is above 255, the limit of std"),
                        ({"op": OP["sauvola"], "K": 257, "kq": 819}, "is above 255, the limit of sauvola"),
                        ({"op": 5}, "unknown window operation 5"), ({"op": -1}, "unknown window operation -1"),
                        ({"border": "skip"}, "reflect101, replicate or constant"),
                        ({"op": OP["mean"], "c": 256}, "c must lie in"), ({"op": OP["mean"], "c": -256}, "c must lie in"),
                        ({"c": 1}, "box takes no c"), ({"op": OP["sauvola"], "c": 1, "kq": 819}, "sauvola takes no c"),
                        ({"op": OP["niblack"], "kq": 16385}, "k must be finite with"),
                        ({"op": OP["sauvola"], "kq": -16385}, "k must be finite with"),
                        ({"op": OP["mean"], "kq": 5}, "mean takes no k")):
        with pytest.raises(RuntimeError, match=msg):
            window(**kwargs)
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == -3).all() and (u.cpu().numpy() == 9).all()  # refused before any launch


def test_cli_binarize_on_the_device_backend(tmp_path):
    import os
    import subprocess

    stripe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "stripe")
    if not os.path.exists(stripe):
        pytest.skip("bin/stripe not built")
    a = IC.text_on_gradient(2 * T + 3, TW + 5)
    src = str(tmp_path / "a.pgm")
    C.write_pnm(src, a)
    for extra in (["--window", "31", "--method", "sauvola"], ["--window", "15", "--chain", "invert", "--c", "5"],
                  ["--window", "31", "--method", "std", "--border", "replicate"]):
        outs = {}
        for backend in ("host", "device"):
            dst = str(tmp_path / f"{backend}.pgm")
            r = subprocess.run([stripe, "binarize", "--input", src, "--backend", backend, "--output", dst] + extra,
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            outs[backend] = (C.read_pnm(dst), r.stdout)
        assert (outs["host"][0] == outs["device"][0]).all() and outs["host"][1] == outs["device"][1], extra
    assert (outs["host"][0] == C.cpu_window(a, "std", 31, "replicate", 0, 0.0)).all()
