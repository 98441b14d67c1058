"""k_warp (csrc/hip/warp.hip) on the GPU, bit-exact against golden_warp: the
map list of the CPU tests on gray and RGB x both modes x both borders,
destination sizes around the tile side on both axes, both instances (asserted
through `_C.warp_plan`), tiles wholly outside the frame, unaligned pitched views
with guard bytes, a source that ends its tensor, both store policies, a second
stream, quarter turns against k_orient, the torch front end, the launch checks
and the CLI.  Frames stay within 300 pixels a side."""
import json
import os
import subprocess

import numpy as np
import pytest

import mpi_cuda_imagemanipulation_amd as m
from np_warp import invert, maps, quantise

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = m._C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPE = os.path.join(ROOT, "bin", "stripe")
TILE = C.warp_tile()
T = TILE["tile"]
ONE = 1 << 24
BORDERS = (("constant", 0), ("constant", 200), ("replicate", 0))
MODES = ("bilinear", "nearest")


def frame(W, H, ch):
    shape = (H, W) if ch == 1 else (H, W, ch)
    return np.random.default_rng(W * 7919 + H * 31 + ch).integers(0, 256, shape, dtype=np.uint8)


def device_warp(x, q, W2, H2, mode, border, fill):
    """k_warp on a contiguous CUDA tensor through the raw binding."""
    H, W = x.shape[:2]
    ch = 1 if x.ndim == 2 else x.shape[2]
    out = torch.empty((H2, W2) + tuple(x.shape[2:]), dtype=torch.uint8, device="cuda")
    C.warp_device(x.data_ptr(), W * ch, W, H, ch, out.data_ptr(), W2 * ch, q, W2, H2, mode, border, fill,
                  torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()


def check(a, q, W2, H2, modes=MODES, borders=BORDERS, what=None):
    x = torch.from_numpy(a).cuda()
    for mode in modes:
        for border, fill in borders:
            ref = C.golden_warp(a, q, W2, H2, mode, border, fill)
            got = device_warp(x, q, W2, H2, mode, border, fill)
            assert got.shape == ref.shape
            assert (got == ref).all(), (what, a.shape, W2, H2, mode, border, fill, int((got != ref).sum()))


def rotation(deg, fit, W, H):
    minv, W2, H2 = C.rotate_matrix(float(deg), fit, W, H)
    return quantise(C, minv, W, H, W2, H2), W2, H2


def test_tile_constants():
    assert TILE == dict(tile=64, box=92, row_bytes_gray=92, row_bytes_rgb=276, lds_gray=8464, lds_rgb=25392)
    # the box covers a rotation at scale 1 over a tile: floor(63 * sqrt(2)) + 3
    assert TILE["box"] >= int(63 * 2 ** 0.5) + 3


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("size", [(90, 70), (1, 1), (2, 300), (300, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_list(ch, size):
    W, H = size
    a = frame(W, H, ch)
    plans = set()
    for name, minv, W2, H2 in maps(C, W, H):
        q = quantise(C, minv, W, H, W2, H2)
        plans.add(C.warp_plan(q))
        if name.startswith("rot") or name in ("identity", "shift+3-2", "scale2"):
            assert C.warp_plan(q) == "staged", name
        if name in ("minify8", "coef+63.9"):
            assert C.warp_plan(q) == "direct", name
        check(a, q, W2, H2, what=name)
    assert plans == {"staged", "direct"}


def test_plan():
    # a rotation at scale 1 always plans staged: |cos| + |sin| <= sqrt(2)
    for deg in np.arange(0, 360, 0.5):
        q, _, _ = rotation(deg, True, 300, 200)
        assert C.warp_plan(q) == "staged", deg
    # the threshold in A: (63 * (|a0| + |a1|) >> 24) + 3 <= 92, i.e. 63 * (|a0| + |a1|) < 90 * 2^24
    lim = -(-90 * ONE // 63)  # the smallest sum that plans direct
    for a0, a1 in ((lim - 1, 0), (0, lim - 1), (-(lim - 1), 0), (lim // 2, -(lim - 1 - lim // 2))):
        assert C.warp_plan([a0, a1, 0, ONE, 0, 0]) == "staged" and C.warp_plan([ONE, 0, 0, a0, a1, 0]) == "staged"
    for a0, a1 in ((lim, 0), (0, -lim), (lim // 2, lim - lim // 2)):
        assert C.warp_plan([a0, a1, 0, ONE, 0, 0]) == "direct" and C.warp_plan([ONE, 0, 0, a0, a1, 0]) == "direct"


def axis_sizes():
    return [1, T - 1, T, T + 1, 2 * T + 3]


@pytest.mark.parametrize("ch", [1, 3])
def test_destination_sizes_around_the_tile(ch):
    a = frame(150, 140, ch)
    for inst, M in (("staged", [0.9, 0.35, -20, -0.3, 0.95, 30]), ("direct", [0.3, 0.04, 2, -0.05, 0.28, 3])):
        for W2 in axis_sizes():
            for H2 in (axis_sizes() if W2 in (1, T + 1) else (9,)):
                q = quantise(C, invert(M), 150, 140, W2, H2)
                assert C.warp_plan(q) == inst
                check(a, q, W2, H2, borders=BORDERS[1:], what=inst)
        for H2 in axis_sizes():
            q = quantise(C, invert(M), 150, 140, 19, H2)
            check(a, q, 19, H2, borders=BORDERS[1:], what=inst)


@pytest.mark.parametrize("ch", [1, 3])
def test_both_axes_beyond_one_tile(ch):
    a = frame(2 * T + 9, 2 * T + 5, ch)
    for deg in (30, 45, -77.7):
        for fit in (False, True):
            q, W2, H2 = rotation(deg, fit, 2 * T + 9, 2 * T + 5)
            check(a, q, W2, H2, what=deg)
    # the largest staged box: 45 degrees at a scale just inside the plan's threshold
    s = 90 / 63 / 2 ** 0.5 * 0.999
    q = quantise(C, [s * 2 ** -0.5, -s * 2 ** -0.5, 40, s * 2 ** -0.5, s * 2 ** -0.5, -60], 2 * T + 9, 2 * T + 5, 200, 150)
    assert C.warp_plan(q) == "staged"
    check(a, q, 200, 150, what="largest box")
    q = quantise(C, [1.43, 0, -3.5, 0, -1.43, 130.25], 2 * T + 9, 2 * T + 5, 131, 129)
    assert C.warp_plan(q) == "direct"
    check(a, q, 131, 129, what="just direct")


@pytest.mark.parametrize("ch", [1, 3])
def test_tiles_wholly_outside_the_frame(ch):
    # a small source in the middle of a destination of 3 x 3 tiles: the corner tiles' boxes miss the frame
    a = frame(40, 30, ch)
    for M in ([1, 0, 70, 0, 1, 80], [0.8, -0.6, 90, 0.6, 0.8, 60]):
        q = quantise(C, invert(M), 40, 30, 3 * T - 5, 3 * T - 9)
        assert C.warp_plan(q) == "staged"
        check(a, q, 3 * T - 5, 3 * T - 9, what="outside")
    # the same with the source far outside on every side of the destination
    for dx, dy in ((-500, 0), (500, 0), (0, -500), (0, 500), (400, 400)):
        q = quantise(C, invert([1, 0, dx, 0, 1, dy]), 40, 30, T + 3, T + 2)
        check(a, q, T + 3, T + 2, what=("far", dx, dy))
    # direct instance: every tap outside
    q = quantise(C, [8, 0, 1000, 0, 8, -3000], 40, 30, T + 3, 5)
    assert C.warp_plan(q) == "direct"
    check(a, q, T + 3, 5, what="direct outside")


@pytest.mark.parametrize("ch", [1, 3])
def test_partial_last_column_of_a_map_that_runs_backwards(ch):
    # a lane whose four pixels straddle the tile's last column (W2 mod 4 = 1, 2, 3) with A00 < 0: the pixels
    # beyond the column are not computed from coordinates outside the staged box
    a = frame(2 * T + 40, 2 * T + 30, ch)
    for deg in (135, 180, -120):
        minv = C.rotate_matrix(float(deg), False, 2 * T + 40, 2 * T + 30)[0]
        for W2 in (1, 2, 3, T + 1, T + 2, T + 3, 2 * T + 3):
            q = quantise(C, minv, 2 * T + 40, 2 * T + 30, W2, T + 5)
            assert q[0] < 0 and C.warp_plan(q) == "staged"
            check(a, q, W2, T + 5, what=(deg, W2))


def device_bytes(n, fill):
    return torch.full((n,), fill, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("off", [1, 7, 15])
def test_unaligned_pitched_views(ch, off):
    stream = torch.cuda.current_stream().cuda_stream
    for (W, H) in ((131, 19), (37, 133), (16, 5), (T + 1, T + 1)):
        a = frame(W, H, ch)
        E = W * ch
        sp = (E + 5) | 1  # odd pitches: every row has its own misalignment
        src = device_bytes(off + sp * H + 64, 0x5A)
        src[off:off + sp * H].view(H, sp)[:, :E] = torch.from_numpy(a.reshape(H, E)).cuda()
        for minv, W2, H2 in ((C.rotate_matrix(30.0, True, W, H)), ([0.5, 0, 0.25, 0, 0.5, 0.75], 2 * W - 3, 2 * H - 1),
                             ([3, 0.5, 0, -0.5, 3, 1], W // 3 + 1, H // 3 + 1)):
            q = quantise(C, minv, W, H, W2, H2)
            E2 = W2 * ch
            dp = (E2 + 13) | 1
            for mode in MODES:
                for border, fill in BORDERS[1:]:
                    ref = C.golden_warp(a, q, W2, H2, mode, border, fill)
                    dst = device_bytes(off + dp * H2 + 64, 0xA5)
                    C.warp_device(src.data_ptr() + off, sp, W, H, ch, dst.data_ptr() + off, dp, q, W2, H2, mode,
                                  border, fill, stream)
                    torch.cuda.synchronize()
                    d = dst.cpu().numpy()
                    body = d[off:off + dp * H2].reshape(H2, dp)
                    assert (body[:, :E2] == ref.reshape(H2, E2)).all(), (W, H, W2, H2, mode, border)
                    # the bytes around the destination and its pitch padding are untouched
                    assert (d[:off] == 0xA5).all() and (body[:, E2:] == 0xA5).all() and (d[off + dp * H2:] == 0xA5).all()


@pytest.mark.parametrize("ch", [1, 3])
def test_source_at_the_end_of_its_tensor(ch):
    # the last pixel of the source is the tensor's last byte; the maps read its last rows and columns
    for (W, H) in ((133, 11), (17, 140), (T + 3, 9)):
        a = frame(W, H, ch)
        n = a.size
        big = torch.empty(n + 37, dtype=torch.uint8, device="cuda")
        big[37:] = torch.from_numpy(a.reshape(-1)).cuda()
        x = big[37:].view(a.shape)
        assert x.data_ptr() + n == big.data_ptr() + big.numel()
        for deg in (0, 1, 180, 45):
            for border in ("constant", "replicate"):
                got = m.ops.rotate(x, deg, border=border, fill=3).cpu().numpy()
                assert (got == m.ops.rotate(a, deg, border=border, fill=3)).all(), (deg, border)
        M = [[0.2, 0, 0], [0, 0.2, 0]]  # direct
        assert (m.ops.warp_affine(x, M, border="replicate").cpu().numpy() ==
                m.ops.warp_reference(a, M, border="replicate")).all()


@pytest.mark.parametrize("nt", ["0", "1"])
def test_both_store_policies(monkeypatch, nt):
    monkeypatch.setenv("STRIPE_NT", nt)
    assert C.launch_policy("warp", cin=3, W=100, rows=100, W2=100, rows2=100)["nt_stores"] == (nt == "1")
    for ch in (1, 3):
        a = frame(T + 37, T + 5, ch)
        q, W2, H2 = rotation(30, True, T + 37, T + 5)
        check(a, q, W2, H2, borders=BORDERS[1:])
        q = quantise(C, [4, 0, 0, 0, 4, 0], T + 37, T + 5, 33, 21)  # direct
        check(a, q, 33, 21, borders=BORDERS[1:])


def test_second_stream():
    a = frame(260, 200, 3)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.from_numpy(a).cuda()
        y = m.ops.rotate(x, 30, expand=True)
        z = m.ops.warp_affine(y, [[0.5, 0, 0], [0, 0.5, 0]], size=(100, 120), mode="nearest")
    s.synchronize()
    ref = m.ops.rotate(a, 30, expand=True)
    assert (y.cpu().numpy() == ref).all()
    assert (z.cpu().numpy() == m.ops.warp_reference(ref, [[0.5, 0, 0], [0, 0.5, 0]], size=(100, 120), mode="nearest")).all()


def test_quarter_turns_equal_orient_on_the_device():
    for ch in (1, 3):
        a = frame(T + 7, 2 * T + 2, ch)
        x = torch.from_numpy(a).cuda()
        for k, op in ((0, "none"), (1, "rot270"), (2, "rot180"), (3, "rot90")):
            for mode in MODES:
                got = m.ops.rotate(x, 90 * k, expand=True, mode=mode)
                assert torch.equal(got, m.ops.orient(x, op)), (k, mode)
                assert (got.cpu().numpy() == np.rot90(a, k)).all()
        assert torch.equal(m.ops.rotate(x, 180), m.ops.orient(x, "rot180"))


def test_front_end_on_tensors():
    a = frame(150, 90, 3)
    x = torch.from_numpy(a).cuda()
    M = [[0.9, 0.2, 3], [-0.2, 0.9, 5]]
    got = m.ops.warp_affine(x, M, size=(80, 140), fill=9)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (80, 140, 3)
    assert (got.cpu().numpy() == m.ops.warp_reference(a, M, size=(80, 140), fill=9)).all()
    g = x[:, :, 1]  # non-contiguous gray view: made contiguous
    assert not g.is_contiguous()
    assert (m.ops.rotate(g, 17).cpu().numpy() == m.ops.rotate(np.ascontiguousarray(a[:, :, 1]), 17)).all()
    t = x.transpose(0, 1)  # non-contiguous RGB
    assert (m.ops.rotate(t, 17).cpu().numpy() == m.ops.rotate(np.ascontiguousarray(a.transpose(1, 0, 2)), 17)).all()
    v = x[10:70, 20:101]  # a strided window with packed pixels: read in place
    assert not v.is_contiguous()
    for border in ("constant", "replicate"):
        assert (m.ops.rotate(v, -33, expand=True, border=border).cpu().numpy() ==
                m.ops.rotate(np.ascontiguousarray(a[10:70, 20:101]), -33, expand=True, border=border)).all()
    b = torch.stack([x, 255 - x, x.flip(0)])
    out = m.ops.rotate(b, 30, expand=True)
    assert (out.cpu().numpy() == m.ops.rotate(b.cpu().numpy(), 30, expand=True)).all()
    assert m.ops.rotate(x[:, :, :1], 45, expand=True).shape == m.ops.rotate(a[:, :, :1], 45, expand=True).shape
    assert m.ops.rotate(b[:0], 30, expand=True).shape == (0,) + tuple(out.shape[1:])
    with pytest.raises(TypeError, match="uint8"):
        m.ops.rotate(x.float(), 3)
    with pytest.raises(ValueError, match="singular"):
        m.ops.warp_affine(x, [[1, 2, 0], [2, 4, 0]])
    with pytest.raises(ValueError, match=r"outside \(-64, 64\)"):
        m.ops.warp_affine(x, [[0.01, 0, 0], [0, 1, 0]])


def test_launch_checks():
    x = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    p = x.data_ptr()
    I = [ONE, 0, 0, 0, ONE, 0]
    for args, msg in (((p, 63, 64, 64, 1, p, 64, I, 64, 64), "src_pitch 63 < row bytes 64"),
                      ((p, 64, 64, 32, 1, p, 31, I, 32, 64), "dst_pitch 31 < row bytes 32"),
                      ((p, 64, 64, 64, 2, p, 64, I, 64, 64), "1 or 3 channels"),
                      ((p, 64, 64, 64, 1, 0, 64, I, 64, 64), "null src or dst"),
                      ((p, 64, 0, 64, 1, p, 64, I, 64, 64), r"source size 0x64 outside 1\.\.65535"),
                      ((p, 64, 64, 64, 1, p, 64, I, 64, 65536), r"destination size 64x65536 outside 1\.\.65535"),
                      ((p, 64, 64, 64, 1, p, 64, [64 * ONE, 0, 0, 0, ONE, 0], 64, 64), r"coefficient outside \(-64, 64\)"),
                      ((p, 64, 64, 64, 1, p, 64, [ONE, 0, ONE << 20, 0, ONE, 0], 64, 64), r"offset outside \(-2\^20, 2\^20\)"),
                      ((p, 64, 64, 64, 1, p, 64, I, 64, 64, "cubic"), "unknown mode 'cubic'"),
                      ((p, 64, 64, 64, 1, p, 64, I, 64, 64, "nearest", "wrap"), "unknown border 'wrap'")):
        with pytest.raises(RuntimeError, match=msg):
            C.warp_device(*args)


@pytest.mark.skipif(not os.path.exists(STRIPE), reason="bin/stripe not built")
def test_cli_device_equals_host(tmp_path):
    a = frame(300, 200, 3)
    src = str(tmp_path / "a.ppm")
    C.write_pnm(src, a)
    outs = {}
    for backend in ("local", "host"):
        dst = str(tmp_path / f"{backend}.ppm")
        args = ["run", "--input", src, "--output", dst, "--orient", "fliph", "--rotate", "30:fit", "--warp-border",
                "constant:40", "--resize", "150x120:bilinear", "--chain", "gaussian5"]
        if backend == "host":
            args += ["--backend", "host"]  # (the default is the device backend where a GPU is present)
        r = subprocess.run([STRIPE, *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        j = json.loads(r.stdout.strip().splitlines()[-1])
        assert j["warp"] == "rotate:30:fit" and j["warped_from"] == [300, 200] and j["backend"] == backend
        assert (j["W"], j["H"]) == (150, 120)
        outs[backend] = C.read_pnm(dst)
    assert (outs["local"] == outs["host"]).all()
    minv, W2, H2 = C.rotate_matrix(30.0, True, 300, 200)
    ref = C.golden_warp(C.golden_orient(a, "fliph"), quantise(C, minv, 300, 200, W2, H2), W2, H2, "bilinear",
                        "constant", 40)
    ref = C.golden_resize(ref, 150, 120, "bilinear")
    assert (outs["host"] == C.golden_apply(ref, "gaussian5", "reflect101", True)).all()
