"""k_edt_* (csrc/hip/distance.hip) on the GPU, exactly equal to the golden
functions: the int32 plane, the u8 form and the masks for both polarities on
every frame of distance_cases, at shapes derived from the kernels' constants (one
pixel, one row, one column, exactly a band by a workgroup, one more, several
with a remainder, widths that are no multiple of 4, a width either side of each
LDS class of the row pass, both side limits) and on a frame of about a million
pixels; the four disc operations; pitched sources and destinations with guard
values; determinism; a second stream; alternating frame sizes; the launch
checks; the CLI.  The reference is golden_distance where its O(W^2 H) loop is
affordable (W^2 H <= 2e7) and cpu_distance, which tests/test_distance.py ties to
it and to scipy, on the wider frames.  Only valid inputs."""
import numpy as np
import pytest

import distance_cases as D
import mpi_cuda_imagemanipulation_amd as m

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = m._C
ops = m.ops
B, T, R = C.distance_tile()
W0, W1, W2 = C.distance_widths()
SHAPES = ((1, 1), (1, 5 * T + 3), (5 * B + 3, 1), (B, T), (B + 1, T + 1), (2 * B + 3, 3 * T + 5),
          (3, W0), (3, W0 + 1), (2, W1), (2, W1 + 1), (3, C.DISTANCE_MAX_SIDE), (C.DISTANCE_MAX_SIDE, 3))
assert SHAPES[5][1] % 4 != 0 and SHAPES[1][1] % 4 != 0  # widths that are no multiple of 4
assert R == 1  # one row per workgroup: no H = R +- 1 shapes
BIG = (1000, 1049)  # about a million pixels
THRESHOLDS = (0, 2, 50)
RADII = (0, 1.5, 7, 40)
MODE = {name: k for k, name in enumerate(C.DISTANCE_MODES)}

_frames = {}
_ref = {}


def frames(shape):
    if shape not in _frames:
        _frames[shape] = dict(D.cases(shape[0], shape[1], seam=min(T, shape[1] - 1)))
    return _frames[shape]


def small(shape):
    return shape[1] * shape[1] * shape[0] <= 2e7


def reference(shape, name, to):
    """The squared plane, computed once: the golden loop on small shapes, the host executor on the others."""
    key = (shape, name, to)
    if key not in _ref:
        fn = C.golden_distance if small(shape) else C.cpu_distance
        _ref[key] = fn(frames(shape)[name], to == "foreground")
    return _ref[key]


def device_mask(x, to, t, above):
    H, W = x.shape
    out = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    C.distance_device(x.data_ptr(), x.stride(0) if H > 1 else W, W, H, to == "foreground",
                      MODE["mask_above" if above else "mask_within"], t, out.data_ptr(), W,
                      torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()


def check_frame(shape, name):
    a = frames(shape)[name]
    x = torch.from_numpy(a).cuda()
    tiny = shape[1] * shape[1] * shape[0] <= 2e6
    for to in D.TOS:
        ref = reference(shape, name, to)
        d = ops.distance_transform(x, to)
        assert d.is_cuda and d.dtype == torch.int32 and tuple(d.shape) == a.shape
        got = d.cpu().numpy()
        assert (got == ref).all(), (shape, name, to, int((got != ref).sum()))
        u8 = ops.distance_transform(x, to, "u8")
        assert u8.is_cuda and u8.dtype == torch.uint8 and (u8.cpu().numpy() == D.numpy_u8(ref)).all(), (shape, name, to)
        if tiny:
            assert (u8.cpu().numpy() == C.golden_distance_u8(a, to == "foreground")).all(), (shape, name, to)
        for t in THRESHOLDS:
            for above in (True, False):
                got = device_mask(x, to, t, above)
                assert (got == D.numpy_mask(ref, t, above)).all(), (shape, name, to, t, above)
                if tiny and t == 2:
                    assert (got == C.golden_distance_mask(a, to == "foreground", t, above)).all(), (shape, name, to)
        f = ops.distance_transform(x, to, "float")
        assert f.is_cuda and f.dtype == torch.float32
        np.testing.assert_allclose(f.cpu().numpy(), D.numpy_float(ref), rtol=1e-6)


CASE_NAMES = [name for name, _ in D.cases(3, 3)]


def test_constants():
    assert (B, T, R) == (64, 512, 1) and (W0, W1, W2) == (4096, 16384, 32768)
    assert C.distance_lds() == {w: 4 * w + 2048 + 80 for w in (W0, W1, W2)}
    assert W2 >= C.DISTANCE_MAX_SIDE and max(C.distance_lds().values()) <= 160 * 1024


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_frame(shape):
    for name in CASE_NAMES:
        check_frame(shape, name)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_million_pixels(name):
    check_frame(BIG, name)


@pytest.mark.parametrize("shape", ((B + 1, T + 1), (2 * B + 3, 70)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_disk_operations(shape):
    for name in CASE_NAMES:
        a = frames(shape)[name]
        x = torch.from_numpy(a).cuda()
        for r in RADII:
            for op, fn in (("erode", ops.erode_disk), ("dilate", ops.dilate_disk), ("open", ops.open_disk),
                           ("close", ops.close_disk)):
                want = C.golden_disk_morph(a, op, r) if shape[1] <= 70 else C.cpu_disk_morph(a, op, r)
                got = fn(x, r)
                assert got.is_cuda and got.dtype == torch.uint8 and (got.cpu().numpy() == want).all(), (shape, name, op, r)


def test_pitched_source_and_destination_planes():
    H, W = 2 * B + 3, 3 * T + 5
    a = D.K.random_mask(H, W, 0.9, 11, value=9)
    wide = torch.full((H, W + 16), 255, dtype=torch.uint8, device="cuda")  # foreground guard columns, odd pitch
    assert wide.stride(0) % 2 == 1
    view = wide[:, 3:3 + W]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 2 == 1 and not view.is_contiguous()
    s = torch.cuda.current_stream().cuda_stream
    for to in D.TOS:
        ref = C.cpu_distance(a, to == "foreground")
        assert (ops.distance_transform(view, to).cpu().numpy() == ref).all()
        assert (ops.distance_transform(view, to, "u8").cpu().numpy() == D.numpy_u8(ref)).all()
        # the raw binding into wider planes: nothing outside a row's W elements is written
        plane = torch.full((H, W + 5), -7, dtype=torch.int32, device="cuda")
        C.distance_device(view.data_ptr(), view.stride(0), W, H, to == "foreground", MODE["squared"], 0, plane.data_ptr(),
                          W + 5, s)
        p = plane.cpu().numpy()
        assert (p[:, :W] == ref).all() and (p[:, W:] == -7).all()
        for mode, want in (("u8", D.numpy_u8(ref)), ("mask_above", D.numpy_mask(ref, 2, True)),
                           ("mask_within", D.numpy_mask(ref, 2, False))):
            # an odd destination address too
            out = torch.full((H * (W + 3) + 1,), 77, dtype=torch.uint8, device="cuda")
            C.distance_device(view.data_ptr(), view.stride(0), W, H, to == "foreground", MODE[mode], 2,
                              out.data_ptr() + 1, W + 3, s)
            o = out.cpu().numpy()[1:].reshape(H, W + 3)
            assert (o[:, :W] == want).all() and (o[:, W:] == 77).all() and out[0].item() == 77, (to, mode)
    for op in ("erode", "dilate", "open", "close"):
        out = torch.full((H, W + 3), 77, dtype=torch.uint8, device="cuda")
        C.disk_morph_device(view.data_ptr(), view.stride(0), W, H, op, 5, out.data_ptr(), W + 3, s)
        o = out.cpu().numpy()
        assert (o[:, :W] == C.cpu_disk_morph(a, op, 2.3)).all() and (o[:, W:] == 77).all(), op
    assert (wide.cpu().numpy()[:, :3] == 255).all() and (wide.cpu().numpy()[:, 3 + W:] == 255).all()


def test_two_runs_are_identical():
    x = torch.from_numpy(frames(BIG)["sparse"]).cuda()
    for to in D.TOS:
        assert torch.equal(ops.distance_transform(x, to), ops.distance_transform(x, to))
    assert torch.equal(ops.open_disk(x, 3), ops.open_disk(x, 3))


def test_second_stream():
    shape = (2 * B + 3, 3 * T + 5)
    a = frames(shape)["random0.8"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.from_numpy(a).cuda()
        d = ops.distance_transform(x)
        u8 = ops.distance_transform(x, "foreground", "u8")
        e = ops.close_disk(x, 2)
    s.synchronize()
    assert (d.cpu().numpy() == reference(shape, "random0.8", "background")).all()
    assert (u8.cpu().numpy() == D.numpy_u8(reference(shape, "random0.8", "foreground"))).all()
    assert (e.cpu().numpy() == C.cpu_disk_morph(a, "close", 2)).all()


def test_alternating_frame_sizes():
    """Two sizes in turn (and one that shares the height): the scratch cache serves each its own buffers."""
    shapes = ((B + 1, T + 1), (2 * B + 3, 3 * T + 5), (B + 1, 300))
    xs = {s: torch.from_numpy(frames(s)["disc"] if s != shapes[2] else D.K.random_mask(s[0], s[1], 0.9, 5)).cuda()
          for s in shapes}
    want = {s: C.cpu_distance(xs[s].cpu().numpy()) for s in shapes}
    got = [(s, ops.distance_transform(xs[s])) for _ in range(3) for s in shapes]  # queued without waiting
    for s, d in got:
        assert (d.cpu().numpy() == want[s]).all(), s
    ops.clear_cache()  # releases the scratch; the next call allocates again
    assert (ops.distance_transform(xs[shapes[0]]).cpu().numpy() == want[shapes[0]]).all()


def test_front_end_shapes_and_refusals():
    a = D.K.random_mask(B + 1, T + 1, 0.8, 3, value=2)
    x = torch.from_numpy(a).cuda()
    d = ops.distance_transform(x[:, :, None])
    assert tuple(d.shape) == a.shape and (d.cpu().numpy() == C.cpu_distance(a)).all()
    y = ops.erode_disk(x[:, :, None], 1)
    assert tuple(y.shape) == a.shape + (1,) and (y[:, :, 0].cpu().numpy() == C.cpu_disk_morph(a, "erode", 1)).all()
    z = torch.zeros((5, 9), dtype=torch.uint8, device="cuda")
    assert (ops.distance_transform(z, "foreground").cpu().numpy() == ops.DISTANCE_NONE).all()
    assert torch.isinf(ops.distance_transform(z, "foreground", "float")).all()
    with pytest.raises(ValueError, match="convert first"):
        ops.distance_transform(torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError, match="uint8"):
        ops.distance_transform(torch.zeros((4, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="radius must be finite and not negative"):
        ops.erode_disk(x, -1)


def test_launch_checks():
    x = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    d = torch.full((8, 8), -3, dtype=torch.int32, device="cuda")
    u = torch.full((8, 8), 9, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="null src or dst"):
        C.distance_device(0, 8, 8, 8, False, 0, 0, d.data_ptr(), 8, s)
    with pytest.raises(RuntimeError, match="null src or dst"):
        C.distance_device(x.data_ptr(), 8, 8, 8, False, 0, 0, 0, 8, s)
    with pytest.raises(RuntimeError, match="dst_pitch 7 < the row's 8 elements"):
        C.distance_device(x.data_ptr(), 8, 8, 8, False, 0, 0, d.data_ptr(), 7, s)
    with pytest.raises(RuntimeError, match="src_pitch 7 < row bytes 8"):
        C.distance_device(x.data_ptr(), 7, 8, 8, False, 0, 0, d.data_ptr(), 8, s)
    with pytest.raises(RuntimeError, match="aligned to 4 bytes"):
        C.distance_device(x.data_ptr(), 8, 8, 7, False, 0, 0, d.data_ptr() + 2, 8, s)
    with pytest.raises(RuntimeError, match="side above 32767"):
        C.distance_device(x.data_ptr(), 32768, 32768, 8, False, 0, 0, d.data_ptr(), 32768, s)
    with pytest.raises(RuntimeError, match="side above 32767"):
        C.distance_device(x.data_ptr(), 8, 8, 32768, False, 1, 0, u.data_ptr(), 8, s)
    with pytest.raises(RuntimeError, match="unknown mode 4"):
        C.distance_device(x.data_ptr(), 8, 8, 8, False, 4, 0, d.data_ptr(), 8, s)
    with pytest.raises(RuntimeError, match="threshold must lie in"):
        C.distance_device(x.data_ptr(), 8, 8, 8, False, 2, -1, u.data_ptr(), 8, s)
    with pytest.raises(RuntimeError, match="null src or dst"):
        C.disk_morph_device(x.data_ptr(), 8, 8, 8, "open", 4, 0, 8, s)
    with pytest.raises(RuntimeError, match="erode, dilate, open or close"):
        C.disk_morph_device(x.data_ptr(), 8, 8, 8, "thin", 4, u.data_ptr(), 8, s)
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == -3).all() and (u.cpu().numpy() == 9).all()  # refused before any launch


def test_cli_distance_on_the_device_backend(tmp_path):
    import os
    import subprocess

    stripe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "stripe")
    if not os.path.exists(stripe):
        pytest.skip("bin/stripe not built")
    a = np.random.default_rng(8).integers(0, 256, (2 * B + 3, T + 5), dtype=np.uint8)
    a[20:90, 30:150] = 240
    src, dst = str(tmp_path / "a.pgm"), str(tmp_path / "d.pgm")
    C.write_pnm(src, a)
    chain = "threshold:128,open3"
    mask = ops.reference(a, chain)
    d2 = C.cpu_distance(mask)
    r = subprocess.run([stripe, "distance", "--input", src, "--chain", chain, "--backend", "device", "--output", dst],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == str(int(d2.max())) and d2.max() > 100
    assert (C.read_pnm(dst) == D.numpy_u8(d2)).all()
    r = subprocess.run([stripe, "distance", "--input", src, "--chain", chain, "--backend", "device", "--open", "4.5",
                        "--output", dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (C.read_pnm(dst) == C.cpu_disk_morph(mask, "open", 4.5)).all()
