"""k_resize (csrc/hip/resize.hip) on the GPU, bit-exact against golden_resize:
row widths around 16 bytes and the kernel's tile, band heights, every factor
class, unaligned and pitched views, a source that ends its allocation, the
torch front end and the CLI.  Frames stay small: at most about 1300 pixels
wide (one 3073-byte gray row case aside) and 300 rows high."""
import json
import os
import subprocess

import numpy as np
import pytest

import mpi_cuda_imagemanipulation_amd as m

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = m._C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPE = os.path.join(ROOT, "bin", "stripe")
TILE = C.resize_tile()["tile"]  # output bytes of a workgroup tile
BAND = C.resize_tile()["band"]  # output rows of a workgroup
_golden = {}


def frame(W, H, ch, kind="random"):
    shape = (H, W) if ch == 1 else (H, W, ch)
    if kind == "last":
        a = np.zeros(shape, np.uint8)
        a[-1, -1] = 255
        return a
    return np.random.default_rng(W * 7919 + H * 31 + ch).integers(0, 256, shape, dtype=np.uint8)


def golden(a, W2, H2, mode):
    key = (a.shape, int(a.sum()), W2, H2, mode)
    if key not in _golden:
        _golden[key] = C.golden_resize(a, W2, H2, mode)
    return _golden[key]


def gpu(a, W2, H2, mode):
    out = m.ops.resize(torch.from_numpy(a).cuda(), size=(H2, W2), mode=mode)
    assert out.is_cuda and out.dtype == torch.uint8
    return out.cpu().numpy()


def check(W, H, ch, W2, H2, mode, kinds=("random", "last")):
    for kind in kinds:
        a = frame(W, H, ch, kind)
        got, ref = gpu(a, W2, H2, mode), golden(a, W2, H2, mode)
        assert got.shape == ref.shape
        assert (got == ref).all(), (W, H, ch, W2, H2, mode, kind, int((got != ref).sum()))


def test_tile_constants():
    assert TILE == 1024 and BAND == 8


@pytest.mark.parametrize("ch", [1, 3])
def test_destination_row_bytes(ch):
    # one below, at and one above 16 bytes, the tile (1 KiB) and two tiles; gray widths are
    # the byte counts themselves, RGB rows the nearest multiples of 3
    widths = [15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 1] if ch == 1 else \
        [5, 6, (TILE - 1) // 3, TILE // 3 + 1, (2 * TILE + 1) // 3 + 1]
    for W2 in widths:
        for W in (150, 1290):
            if W2 * 32 < W:
                continue  # auto would be an area factor above the cap
            check(W, 9, ch, W2, 7, "auto", kinds=("random",))
            check(W, 9, ch, W2, 9, "bilinear", kinds=("last",))
        check(301, 5, ch, W2, 5, "nearest", kinds=("random",))


@pytest.mark.parametrize("ch", [1, 3])
def test_source_row_bytes(ch):
    widths = [1, 15, 16, 17, 1023, 1024, 1025, 3073] if ch == 1 else [1, 5, 6, 341, 342, 1025]
    for W in widths:
        check(W, 6, ch, max(1, W // 3), 4, "auto")           # area x (identity-like at W = 1)
        check(W, 6, ch, min(1300, 2 * W + 1), 6, "auto")     # bilinear x
        check(W, 6, ch, 37, 6, "nearest", kinds=("random",))
        check(W, 6, ch, max(1, (W + 31) // 32), 6, "auto", kinds=("random",))  # up to 33 taps a pixel


@pytest.mark.parametrize("ch", [1, 3])
def test_heights(ch):
    for H2 in (1, 2, BAND - 1, BAND, BAND + 1, 2 * BAND + 1):
        check(130, 2 * H2 + 1, ch, 70, H2, "auto", kinds=("random",))   # area y, adjacent cells share a row
        check(130, 5, ch, 70, H2, "bilinear", kinds=("random",))        # grows (or shrinks) on two-row lookups
        check(130, H2, ch, 130, H2, "auto", kinds=("random",))          # identity
    for H in (1, 2, BAND - 1, BAND, BAND + 1):
        check(70, H, ch, 90, 3 * H + 1, "auto", kinds=("last",))


FACTORS = [
    # W, H -> W2, H2, mode
    (262, 130, 262, 130, "auto"),      # 1
    (262, 130, 131, 65, "auto"),       # 2
    (262, 130, 131, 65, "nearest"),
    (261, 129, 174, 86, "auto"),       # 3/2
    (131, 131, 65, 65, "auto"),        # 131 -> 65
    (131, 131, 65, 65, "bilinear"),
    (1280, 64, 40, 2, "auto"),         # 32 on both axes: 33 taps never, 32 always
    (1290, 34, 41, 3, "auto"),         # 31.46 x, 11.3 y
    (131, 65, 262, 130, "auto"),       # upscale 2
    (51, 21, 289, 119, "auto"),        # upscale 17/3
    (51, 21, 289, 119, "nearest"),
    (300, 40, 100, 120, "auto"),       # shrink x, grow y
    (100, 120, 300, 40, "auto"),       # grow x, shrink y
    (200, 100, 200, 37, "auto"),       # H only
    (200, 100, 77, 100, "auto"),       # W only
    (200, 100, 640, 100, "auto"),
    (1, 1, 40, 30, "auto"),            # 1x1 source
    (1, 1, 1, 1, "auto"),
    (40, 30, 1, 1, "bilinear"),        # 1x1 destination
    (30, 28, 1, 1, "auto"),
    (1, 9, 1, 4, "auto"),
]


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("W,H,W2,H2,mode", FACTORS)
def test_factors(W, H, W2, H2, mode, ch):
    check(W, H, ch, W2, H2, mode)


@pytest.mark.parametrize("ch", [1, 3])
def test_factor_32_and_just_below_on_four_rows(ch):
    # 16384 -> 512 columns has 32 or 33 taps a pixel (count 33 where a cell straddles), 16383 -> 512 is
    # 31.998; gray rows are the full 16384 columns, RGB rows a third of that (the tile plan is per byte)
    for W in ((16384, 16383) if ch == 1 else (5472, 5471)):
        W2 = 512 if ch == 1 else 171
        cnt = C.resize_taps(W, W2, "area")[1]
        assert cnt.max() == (32 if W % W2 == 0 else 33)  # a cell of 31.998 pixels straddles 33
        check(W, 4, ch, W2, 4, "auto", kinds=("random",))
        check(W, 4, ch, W2, 1, "area", kinds=("last",))


def device_bytes(n, fill):
    return torch.full((n,), fill, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("off", [1, 7, 15])
def test_unaligned_pitched_views(ch, off):
    stream = torch.cuda.current_stream().cuda_stream
    for (W, H, W2, H2, mode) in ((131, 19, 65, 9, "auto"), (65, 9, 341, 19, "auto"), (341, 11, 341, 11, "auto"),
                                 (700, 6, 23, 6, "auto"), (67, 9, 33, 5, "nearest")):
        a = frame(W, H, ch)
        ref = golden(a, W2, H2, mode)
        E, E2 = W * ch, W2 * ch
        sp, dp = E + 5, E2 + 13  # odd pitches: every row has its own misalignment
        src = device_bytes(off + sp * H + 64, 0x5A)
        rows = torch.from_numpy(a.reshape(H, E)).cuda()
        src[off:off + sp * H].view(H, sp)[:, :E] = rows
        dst = device_bytes(off + dp * H2 + 64, 0xA5)
        C.resize_device(src.data_ptr() + off, sp, W, H, ch, dst.data_ptr() + off, dp, W2, H2, mode, stream)
        torch.cuda.synchronize()
        d = dst.cpu().numpy()
        body = d[off:off + dp * H2].reshape(H2, dp)
        assert (body[:, :E2] == ref.reshape(H2, E2)).all(), (W, H, W2, H2, mode)
        # the bytes around the destination and its pitch padding are untouched
        assert (d[:off] == 0xA5).all() and (body[:, E2:] == 0xA5).all() and (d[off + dp * H2:] == 0xA5).all()


@pytest.mark.parametrize("ch", [1, 3])
def test_source_at_the_end_of_its_tensor(ch):
    # an ordinary run: the last pixel is the tensor's last byte
    for (W, H, W2, H2, mode) in ((133, 11, 67, 5, "auto"), (133, 11, 300, 20, "auto"), (1027, 3, 33, 3, "auto"),
                                 (17, 2, 17, 2, "nearest")):
        a = frame(W, H, ch)
        n = a.size
        big = torch.empty(n + 37, dtype=torch.uint8, device="cuda")
        big[37:] = torch.from_numpy(a.reshape(-1)).cuda()
        x = big[37:].view(a.shape)
        assert x.data_ptr() + n == big.data_ptr() + big.numel()
        got = m.ops.resize(x, size=(H2, W2), mode=mode).cpu().numpy()
        assert (got == golden(a, W2, H2, mode)).all()


def test_ops_resize_on_tensors():
    a = frame(200, 90, 3)
    x = torch.from_numpy(a).cuda()
    for kw in (dict(size=(45, 100)), dict(scale=0.5), dict(scale=(2, 0.25)), dict(size=(91, 333), mode="nearest"),
               dict(size=(91, 333), mode="bilinear"), dict(scale=0.1, mode="area")):
        assert (m.ops.resize(x, **kw).cpu().numpy() == m.ops.resize(a, **kw)).all(), kw
    g = x[:, :, 1]  # non-contiguous gray view
    assert not g.is_contiguous()
    assert (m.ops.resize(g, size=(30, 41)).cpu().numpy() == m.ops.resize(np.ascontiguousarray(a[:, :, 1]), size=(30, 41))).all()
    t = x.transpose(0, 1)  # non-contiguous RGB
    assert (m.ops.resize(t, scale=1.5).cpu().numpy() == m.ops.resize(np.ascontiguousarray(a.transpose(1, 0, 2)), scale=1.5)).all()
    b = torch.stack([x, 255 - x, x.flip(0)])
    out = m.ops.resize(b, size=(33, 50))
    assert out.shape == (3, 33, 50, 3)
    assert (out.cpu().numpy() == m.ops.resize(b.cpu().numpy(), size=(33, 50))).all()
    k = m.ops.resize(x[:, :, :1], size=(10, 10))
    assert k.shape == (10, 10, 1)
    with pytest.raises(TypeError, match="uint8"):
        m.ops.resize(x.float(), size=(3, 3))
    with pytest.raises(RuntimeError, match="exceeds the limit of 32"):
        m.ops.resize(x, size=(2, 2))


def test_second_stream():
    a = frame(640, 200, 3)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.from_numpy(a).cuda()
        y = m.ops.resize(x, size=(100, 320))
        z = m.ops.resize(y, scale=3)
    s.synchronize()
    ref = C.golden_resize(a, 320, 100, "auto")
    assert (y.cpu().numpy() == ref).all() and (z.cpu().numpy() == C.golden_resize(ref, 960, 300, "auto")).all()


def test_launch_checks():
    x = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    for args, msg in (((x.data_ptr(), 63, 64, 64, 1, x.data_ptr(), 64, 8, 8), "src_pitch 63 < row bytes 64"),
                      ((x.data_ptr(), 64, 64, 64, 1, x.data_ptr(), 7, 8, 8), "dst_pitch 7 < row bytes 8"),
                      ((x.data_ptr(), 64, 64, 64, 2, x.data_ptr(), 64, 8, 8), "1 or 3 channels"),
                      ((0, 64, 64, 64, 1, x.data_ptr(), 64, 8, 8), "null src or dst")):
        with pytest.raises(RuntimeError, match=msg):
            C.resize_device(*args, "auto", 0)


@pytest.mark.skipif(not os.path.exists(STRIPE), reason="bin/stripe not built")
def test_cli_device_equals_host(tmp_path):
    a = frame(300, 200, 3)
    src = str(tmp_path / "a.ppm")
    C.write_pnm(src, a)
    outs = {}
    for backend in ("local", "host"):
        dst = str(tmp_path / f"{backend}.ppm")
        args = ["run", "--input", src, "--output", dst, "--resize", "120x75", "--chain", "gaussian5"]
        if backend == "host":
            args += ["--backend", "host"]  # (the default is the device backend where a GPU is present)
        r = subprocess.run([STRIPE, *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        j = json.loads(r.stdout.strip().splitlines()[-1])
        assert j["resized_from"] == [300, 200] and j["backend"] == backend and (j["W"], j["H"]) == (120, 75)
        outs[backend] = C.read_pnm(dst)
    assert (outs["local"] == outs["host"]).all()
    assert (outs["host"] == C.golden_apply(C.golden_resize(a, 120, 75, "auto"), "gaussian5", "reflect101", True)).all()
