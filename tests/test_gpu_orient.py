"""k_orient (csrc/hip/orient.hip) on the GPU, bit-exact against golden_orient:
all eight orientations on gray and RGB, row lengths around 16 bytes and the
sides of both tile shapes on both axes, unaligned pitched views with guard bytes, a source
window that ends its tensor, crops at tile seams, both store policies, a second
stream, the torch front end and the CLI.  Frames stay within 300 pixels (a few
narrow ones of 515: two of the widest tiles plus 3)."""
import json
import os
import subprocess

import numpy as np
import pytest

import mpi_cuda_imagemanipulation_amd as m
from np_orient import BITS, NAMES, np_orient

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C = m._C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPE = os.path.join(ROOT, "bin", "stripe")
TILE = C.orient_tile()
ROWS = TILE["transposing"]["rows"]  # source rows of a transposing tile (the destination tile's width)
FX_ROWS = TILE["fx"]["rows"]        # rows of an FX tile


def seg(ch, kind="transposing"):  # source pixels per tile row
    return TILE[kind]["seg_gray" if ch == 1 else "seg_rgb"]


def frame(W, H, ch):
    shape = (H, W) if ch == 1 else (H, W, ch)
    return np.random.default_rng(W * 7919 + H * 31 + ch).integers(0, 256, shape, dtype=np.uint8)


def check(W, H, ch, names=NAMES, crop=None):
    a = frame(W, H, ch)
    x = torch.from_numpy(a).cuda()
    for name in names:
        got = m.ops.orient(x, name, crop)
        assert got.is_cuda and got.dtype == torch.uint8
        ref = C.golden_orient(a, name, crop)
        assert tuple(got.shape) == ref.shape, (W, H, ch, name)
        got = got.cpu().numpy()
        assert (got == ref).all(), (W, H, ch, name, crop, int((got != ref).sum()))
        assert (ref == np_orient(a, name, crop)).all()


def test_tile_constants():
    assert TILE == dict(fx=dict(rows=64, seg_gray=256, seg_rgb=128, lds_gray=16640, lds_rgb=24832),
                        transposing=dict(rows=128, seg_gray=128, seg_rgb=64, lds_gray=17024, lds_rgb=25344),
                        copy_rows=4, cpu_tile=32)


def axis_sizes(ch):
    # row lengths of 15, 16, 17 and 33 bytes (RGB: the nearest whole pixels), the tile's two sides -1, +0, +1,
    # two tiles plus 3, and 1
    small = [15, 16, 17, 33] if ch == 1 else [5, 6, 11]
    sides = (ROWS, seg(ch), FX_ROWS, seg(ch, "fx"))  # every tile side of either tiled instance
    tiles = sorted({s + d for s in sides for d in (-1, 0, 1)} | {2 * s + 3 for s in sides})
    return [1] + small + tiles


@pytest.mark.parametrize("ch", [1, 3])
def test_widths(ch):
    # a transposing op swaps the axes: every size is a width here and a height below
    for W in axis_sizes(ch):
        check(W, 9, ch)


@pytest.mark.parametrize("ch", [1, 3])
def test_heights(ch):
    for H in axis_sizes(ch):
        check(19, H, ch)


@pytest.mark.parametrize("ch", [1, 3])
def test_both_axes_beyond_one_tile(ch):
    check(2 * ROWS + 3, 2 * seg(ch) + 3, ch)
    check(2 * seg(ch) + 3, 2 * ROWS + 3, ch)
    check(2 * seg(ch, "fx") + 3, 2 * FX_ROWS + 3, ch, names=("fliph", "rot180"))
    check(1, 1, ch)


def device_bytes(n, fill):
    return torch.full((n,), fill, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("off", [1, 7, 15])
def test_unaligned_pitched_views(ch, off):
    stream = torch.cuda.current_stream().cuda_stream
    for (W, H) in ((131, 19), (37, 133), (16, 5), (seg(ch) + 1, ROWS + 1), (seg(ch, "fx") + 1, FX_ROWS + 1)):
        a = frame(W, H, ch)
        E = W * ch
        sp = E + 5  # odd pitches: every row has its own misalignment
        src = device_bytes(off + sp * H + 64, 0x5A)
        src[off:off + sp * H].view(H, sp)[:, :E] = torch.from_numpy(a.reshape(H, E)).cuda()
        for name in NAMES:
            ref = C.golden_orient(a, name)
            H2, E2 = ref.shape[0], ref.shape[1] * ch
            dp = E2 + 13
            dst = device_bytes(off + dp * H2 + 64, 0xA5)
            C.orient_device(src.data_ptr() + off, sp, W, H, ch, dst.data_ptr() + off, dp, name, None, stream)
            torch.cuda.synchronize()
            d = dst.cpu().numpy()
            body = d[off:off + dp * H2].reshape(H2, dp)
            assert (body[:, :E2] == ref.reshape(H2, E2)).all(), (W, H, name)
            # the bytes around the destination and its pitch padding are untouched
            assert (d[:off] == 0xA5).all() and (body[:, E2:] == 0xA5).all() and (d[off + dp * H2:] == 0xA5).all()


@pytest.mark.parametrize("ch", [1, 3])
def test_source_window_at_the_end_of_its_tensor(ch):
    # the last pixel of the window is the tensor's last byte, whole frames and crops that end there
    for (W, H) in ((133, 11), (17, 140), (seg(ch) + 3, 9)):
        a = frame(W, H, ch)
        n = a.size
        big = torch.empty(n + 37, dtype=torch.uint8, device="cuda")
        big[37:] = torch.from_numpy(a.reshape(-1)).cuda()
        x = big[37:].view(a.shape)
        assert x.data_ptr() + n == big.data_ptr() + big.numel()
        for name in NAMES:
            assert (m.ops.orient(x, name).cpu().numpy() == C.golden_orient(a, name)).all(), name
            # the source window of this crop is the frame's last rows and columns
            t, fx, fy = BITS[name]
            ow, oh = (H, W) if t else (W, H)
            srcw = (W - 5, H - 3, 5, 3)
            crop = [c for c in [(x0, y0, 3 if t else 5, 5 if t else 3) for x0 in (0, ow - (3 if t else 5))
                                for y0 in (0, oh - (5 if t else 3))]
                    if C.orient_source_window(name, W, H, c) == srcw]
            assert len(crop) == 1, (name, crop)
            assert (m.ops.orient(x, name, crop[0]).cpu().numpy() == C.golden_orient(a, name, crop[0])).all(), name


@pytest.mark.parametrize("ch", [1, 3])
def test_crops_at_tile_seams(ch):
    # a frame of more than two tiles a side; windows (of the oriented frame) that start and end inside a tile,
    # on the seams, one pixel either side of them, and at the frame's last pixel
    W, H = 2 * ROWS + 9, 2 * ROWS + 5
    a = frame(W, H, ch)
    x = torch.from_numpy(a).cuda()
    for name in NAMES:
        ow, oh = (H, W) if BITS[name][0] else (W, H)
        s = seg(ch) if BITS[name][0] else min(seg(ch, "fx"), ROWS)
        crops = [(3, 5, 40, 30), (s, ROWS, s, ROWS), (ROWS, s, ROWS, s), (s - 1, ROWS - 1, s + 2, ROWS + 2),
                 (s + 1, ROWS + 1, s - 2, 7), (ow - 1, oh - 1, 1, 1), (ow - 17, oh - 33, 17, 33), (0, 0, ow, 1),
                 (0, 0, 1, oh), (1, 0, ow - 1, oh)]
        for crop in crops:
            got = m.ops.orient(x, name, crop).cpu().numpy()
            ref = C.golden_orient(a, name, crop)
            assert got.shape == ref.shape and (got == ref).all(), (name, crop)
            assert (ref == np_orient(a, name, crop)).all()


@pytest.mark.parametrize("nt", ["0", "1"])
def test_both_store_policies(monkeypatch, nt):
    monkeypatch.setenv("STRIPE_NT", nt)
    assert C.launch_policy("orient", cin=3, W=100, rows=100)["nt_stores"] == (nt == "1")
    for ch in (1, 3):
        check(ROWS + 5, seg(ch) + 3, ch)
        check(33, 7, ch, crop=(1, 2, 5, 3))


def test_second_stream():
    a = frame(260, 200, 3)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.from_numpy(a).cuda()
        y = m.ops.orient(x, "rot90")
        z = m.ops.orient(y, "fliph", (3, 4, 100, 50))
    s.synchronize()
    ref = C.golden_orient(a, "rot90")
    assert (y.cpu().numpy() == ref).all() and (z.cpu().numpy() == C.golden_orient(ref, "fliph", (3, 4, 100, 50))).all()


def test_round_trips_on_the_device():
    for ch in (1, 3):
        a = frame(ROWS + 7, seg(ch) + 2, ch)
        x = torch.from_numpy(a).cuda()
        for name in NAMES:
            back = m.ops.orient(m.ops.orient(x, name), C.orient_inverse(name))
            assert torch.equal(back, x), name
            for other in ("rot90", "fliph"):
                both = m.ops.orient(m.ops.orient(x, name), other)
                assert torch.equal(both, m.ops.orient(x, C.orient_compose(name, other))), (name, other)


def test_front_end_on_tensors():
    a = frame(150, 90, 3)
    x = torch.from_numpy(a).cuda()
    g = x[:, :, 1]  # non-contiguous gray view: made contiguous
    assert not g.is_contiguous()
    assert (m.ops.orient(g, "rot270").cpu().numpy() == np.rot90(a[:, :, 1], 1)).all()
    t = x.transpose(0, 1)  # non-contiguous RGB
    assert (m.ops.orient(t, "fliph").cpu().numpy() == a.transpose(1, 0, 2)[:, ::-1]).all()
    v = x[10:70, 20:101]  # a strided window with packed pixels: read in place
    assert not v.is_contiguous()
    for name in NAMES:
        assert (m.ops.orient(v, name).cpu().numpy() == np_orient(a[10:70, 20:101], name)).all(), name
    b = torch.stack([x, 255 - x, x.flip(0)])
    out = m.ops.orient(b, "rot90", (2, 3, 40, 50))
    assert out.shape == (3, 50, 40, 3)
    assert (out.cpu().numpy() == m.ops.orient(b.cpu().numpy(), "rot90", (2, 3, 40, 50))).all()
    assert m.ops.orient(x[:, :, :1], "transpose").shape == (150, 90, 1)
    for k in range(-5, 6):
        assert torch.equal(m.ops.rot90(x, k), torch.rot90(x, k, (0, 1))), k
    assert torch.equal(m.ops.flip(x, 0), x.flip(0)) and torch.equal(m.ops.flip(x, 1), x.flip(1))
    assert torch.equal(m.ops.flip(x, (0, 1)), x.flip(0, 1))
    assert torch.equal(m.ops.transpose_image(x), x.transpose(0, 1))
    assert torch.equal(m.ops.crop(x, 7, 9, 50, 40), x[9:49, 7:57])
    with pytest.raises(TypeError, match="uint8"):
        m.ops.orient(x.float(), "fliph")
    with pytest.raises(ValueError, match="leaves the oriented frame of 90x150"):
        m.ops.orient(x, "rot90", (0, 0, 91, 10))


def test_launch_checks():
    x = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    p = x.data_ptr()
    for args, msg in (((p, 63, 64, 64, 1, p, 64, "fliph"), "src_pitch 63 < row bytes 64"),
                      ((p, 64, 64, 32, 1, p, 31, "rot90"), "dst_pitch 31 < row bytes 32"),
                      ((p, 64, 64, 64, 2, p, 64, "none"), "1 or 3 channels"),
                      ((p, 64, 64, 64, 1, 0, 64, "none"), "null src or dst"),
                      ((p, 64, 64, 64, 1, p, 64, "none", (60, 0, 5, 5)), "leaves the frame of 64x64")):
        with pytest.raises(RuntimeError, match=msg):
            C.orient_device(*args)


@pytest.mark.skipif(not os.path.exists(STRIPE), reason="bin/stripe not built")
def test_cli_device_equals_host(tmp_path):
    a = frame(300, 200, 3)
    src = str(tmp_path / "a.ppm")
    C.write_pnm(src, a)
    outs = {}
    for backend in ("local", "host"):
        dst = str(tmp_path / f"{backend}.ppm")
        args = ["run", "--input", src, "--output", dst, "--orient", "rot90", "--crop", "150x220+30+40", "--chain",
                "gaussian5"]
        if backend == "host":
            args += ["--backend", "host"]  # (the default is the device backend where a GPU is present)
        r = subprocess.run([STRIPE, *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        j = json.loads(r.stdout.strip().splitlines()[-1])
        assert j["oriented"] == "rot90" and j["cropped_from"] == [300, 200] and j["backend"] == backend
        assert (j["W"], j["H"]) == (150, 220)
        outs[backend] = C.read_pnm(dst)
    assert (outs["local"] == outs["host"]).all()
    ref = np_orient(a, "rot90", (30, 40, 150, 220))
    assert (outs["host"] == C.golden_apply(ref, "gaussian5", "reflect101", True)).all()
