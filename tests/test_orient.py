"""Orientation and crop on the CPU: the rule (golden_orient) against the numpy
column of its table, the host executor against the golden loop, the group
table, the parsers and their refusals, the Exif Orientation reader on spliced
JPEG streams, and the CLIs end to end on the host backend.  No GPU."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import mpi_cuda_imagemanipulation_amd as m
from np_orient import BITS, NAMES, NP, coord_frame, np_orient

C = m._C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIPE = os.path.join(ROOT, "bin", "stripe")
TS = C.orient_tile()["cpu_tile"]


# ---- rule and executor ----
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_golden_equals_numpy(name, ch):
    for (W, H) in ((7, 5), (40, 33), (1, 9), (9, 1), (1, 1)):
        a = coord_frame(W, H, ch)
        got = C.golden_orient(a, name)
        assert got.shape == np_orient(a, name).shape
        assert (got == np_orient(a, name)).all(), (name, W, H)


def test_names_bits_and_exif():
    assert tuple(C.orient_names()) == NAMES
    for i, name in enumerate(NAMES):
        t, fx, fy = BITS[name]
        assert C.parse_orient(name) == (name, t << 2 | fx << 1 | fy)
        assert C.parse_orient(f"exif:{i + 1}") == C.parse_orient(name)
    assert C.parse_orient("cw")[0] == "rot90" and C.parse_orient("ccw")[0] == "rot270"
    # the Exif column: a frame stored under tag N (the inverse applied to the upright frame) comes out upright
    up = coord_frame(6, 4, 3)
    for i, name in enumerate(NAMES):
        stored = np_orient(up, C.orient_inverse(name))
        assert (C.golden_orient(stored, f"exif:{i + 1}") == up).all(), name


SHAPES = [(1, 1), (1, 37), (37, 1), (13, 17), (101, 67), (TS - 1, TS + 1), (TS, TS), (TS + 1, TS - 1),
          (2 * TS + 3, 3 * TS + 1)]


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("threads", [1, 2, 7])
def test_cpu_orient_equals_golden(threads, ch):
    for (W, H) in SHAPES:
        a = coord_frame(W, H, ch, seed=threads)
        for name in NAMES:
            assert (C.cpu_orient(a, name, None, threads) == C.golden_orient(a, name)).all(), (name, W, H)


@pytest.mark.parametrize("threads", [2, 7])
def test_cpu_orient_row_blocks_on_a_frame_that_splits(threads):
    # 900 KB: enough work for three row blocks
    a = coord_frame(601, 499, 3)
    for name in NAMES:
        assert (C.cpu_orient(a, name, None, threads) == np_orient(a, name)).all(), name


def test_compose_and_inverse_all_pairs():
    a = coord_frame(5, 3, 3)
    for x in NAMES:
        inv = C.orient_inverse(x)
        assert (np_orient(np_orient(a, x), inv) == a).all() and C.orient_compose(x, inv) == "none"
        for y in NAMES:
            z = C.orient_compose(x, y)
            assert (np_orient(np_orient(a, x), y) == np_orient(a, z)).all(), (x, y, z)
    assert C.orient_compose("cw", "exif:6") == "rot180"


def test_ops_front_end_on_numpy():
    a = coord_frame(23, 17, 3)
    for name in NAMES:
        assert (m.ops.orient(a, name) == np_orient(a, name)).all()
        assert (m.ops.orient_reference(a, name) == np_orient(a, name)).all()
    for k in range(-5, 6):
        assert (m.ops.rot90(a, k) == np.rot90(a, k)).all(), k
    assert (m.ops.flip(a, 0) == a[::-1]).all() and (m.ops.flip(a, 1) == a[:, ::-1]).all()
    assert (m.ops.flip(a, (0, 1)) == a[::-1, ::-1]).all()
    assert (m.ops.transpose_image(a) == a.transpose(1, 0, 2)).all()
    assert (m.ops.crop(a, 3, 2, 10, 9) == a[2:11, 3:13]).all()
    assert m.ops.orient(a[:, :, :1], "rot90").shape == (23, 17, 1)
    b = np.stack([a, 255 - a])
    assert (m.ops.orient(b, "transverse", (1, 2, 5, 7)) == np.stack([np_orient(f, "transverse", (1, 2, 5, 7)) for f in b])).all()
    assert m.ops.orient(b[:0], "rot90").shape == (0, 23, 17, 3)
    for name in ("orient", "orient_reference", "flip", "rot90", "transpose_image", "crop", "exif_orientation"):
        assert name in m.ops.__all__
    with pytest.raises(ValueError, match="axis"):
        m.ops.flip(a, 2)
    with pytest.raises(TypeError, match="uint8"):
        m.ops.orient(a.astype(np.float32), "fliph")


# ---- parsing and refusals ----
def test_orient_refusals_quote_the_token():
    for tok in ("rot45", "", "exif:0", "exif:9", "exif:", "exif:12", "ROT90", "rot90 "):
        with pytest.raises(RuntimeError) as e:
            C.parse_orient(tok)
        assert f"'{tok}'" in str(e.value) and "transverse" in str(e.value) and "exif:1..8" in str(e.value)


def test_crop_spec():
    assert C.parse_crop_spec("3x2+1+2") == (1, 2, 3, 2)
    assert C.parse_crop_spec("65535x1+0+0") == (0, 0, 65535, 1)
    assert C.parse_crop_spec("10x20+30+40", 40, 60) == (30, 40, 10, 20)
    for tok in ("", "3x2", "3x2+1", "3+1+2", "x2+1+2", "3x+1+2", "3x2+1+", "3x2+-1+2", "3x2+1+2+3", "axb+1+2",
                "3 x2+1+2", "70000x2+0+0", "3x2+1+2 "):
        with pytest.raises(RuntimeError) as e:
            C.parse_crop_spec(tok)
        assert f"'{tok}'" in str(e.value), tok
    for tok in ("0x2+1+2", "3x0+1+2"):
        with pytest.raises(RuntimeError, match="empty window") as e:
            C.parse_crop_spec(tok)
        assert f"'{tok}'" in str(e.value)
    # outside the frame: the error names the token and the frame
    for tok in ("10x20+31+40", "10x20+30+41", "41x1+0+0", "1x61+0+0", "1x1+40+0", "1x1+0+60"):
        with pytest.raises(RuntimeError) as e:
            C.parse_crop_spec(tok, 40, 60)
        assert f"'{tok}'" in str(e.value) and "40x60" in str(e.value), tok


@pytest.mark.parametrize("ch", [1, 3])
def test_crop_after_each_orientation(ch):
    a = coord_frame(41, 29, ch)
    for name in NAMES:
        ow, oh = (29, 41) if BITS[name][0] else (41, 29)
        for crop in ((0, 0, ow, oh), (3, 5, 11, 7), (ow - 1, oh - 1, 1, 1), (0, oh - 4, ow, 4), (ow - 6, 0, 6, oh)):
            ref = np_orient(a, name, crop)
            assert (C.golden_orient(a, name, crop) == ref).all(), (name, crop)
            for threads in (1, 2):
                assert (C.cpu_orient(a, name, crop, threads) == ref).all(), (name, crop)
            # the window of the source it comes from, oriented on its own, is the same picture
            x0, y0, w, h = C.orient_source_window(name, 41, 29, crop)
            assert (np_orient(a[y0:y0 + h, x0:x0 + w], name) == ref).all(), (name, crop)
        for crop in ((0, 0, ow + 1, 1), (1, 0, ow, 1), (0, 0, 1, oh + 1), (0, oh, 1, 1)):
            with pytest.raises(RuntimeError, match=f"leaves the frame of {ow}x{oh}"):
                C.golden_orient(a, name, crop)
            with pytest.raises(RuntimeError, match=f"leaves the frame of {ow}x{oh}"):
                C.cpu_orient(a, name, crop)
        with pytest.raises(RuntimeError, match="empty window"):
            C.cpu_orient(a, name, (0, 0, 0, 3))


# ---- jpeg_orientation ----
def tiff(order, entries, ifd_offset=8):
    """A TIFF header and an IFD0 of (tag, type, count, value) entries; SHORT values sit in the first two bytes
    of the value field, as the standard has it."""
    e = "<" if order == "II" else ">"
    out = order.encode() + struct.pack(e + "HI", 42, ifd_offset) + b"\0" * (ifd_offset - 8)
    out += struct.pack(e + "H", len(entries))
    for tag, typ, count, value in entries:
        out += struct.pack(e + "HHI", tag, typ, count)
        out += struct.pack(e + "HH", value, 0) if typ == 3 else struct.pack(e + "I", value)
    return out + struct.pack(e + "I", 0)


def app1(payload):
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def exif(order, entries, **kw):
    return app1(b"Exif\0\0" + tiff(order, entries, **kw))


@pytest.fixture(scope="module")
def jpeg():
    a = coord_frame(24, 16, 3)
    data = bytes(C.encode_jpeg(a, 90))
    assert data[:2] == b"\xff\xd8"
    return data


def splice(jpeg, segment):
    return jpeg[:2] + segment + jpeg[2:]


ORIENTATION = 0x0112


@pytest.mark.parametrize("order", ["II", "MM"])
def test_jpeg_orientation_reads_the_tag(jpeg, order):
    assert C.jpeg_orientation(jpeg) == 1  # no APP1
    for v in range(1, 9):
        assert C.jpeg_orientation(splice(jpeg, exif(order, [(ORIENTATION, 3, 1, v)]))) == v
        # the tag in a later position of IFD0, and IFD0 further into the segment
        later = [(0x010F, 2, 1, 0x41), (0x0110, 3, 1, 7), (ORIENTATION, 3, 1, v), (0x011A, 4, 1, 72)]
        assert C.jpeg_orientation(splice(jpeg, exif(order, later))) == v
        assert C.jpeg_orientation(splice(jpeg, exif(order, later, ifd_offset=20))) == v
        # behind another marker segment, and with the decoder unchanged: the stored pixels
        tagged = splice(jpeg, app1(b"http://ns.adobe.com/xap/1.0/\0<x/>") + exif(order, [(ORIENTATION, 3, 1, v)]))
        assert C.jpeg_orientation(tagged) == v
        assert m.ops.exif_orientation(tagged) == v
        assert (C.decode_jpeg(tagged) == C.decode_jpeg(jpeg)).all()


@pytest.mark.parametrize("order", ["II", "MM"])
def test_jpeg_orientation_returns_1(jpeg, order):
    one = lambda seg: C.jpeg_orientation(splice(jpeg, seg))  # noqa: E731
    assert one(exif(order, [(ORIENTATION, 4, 1, 6)])) == 1    # wrong type (LONG)
    assert one(exif(order, [(ORIENTATION, 1, 1, 6)])) == 1    # wrong type (BYTE)
    assert one(exif(order, [(ORIENTATION, 3, 2, 6)])) == 1    # wrong count
    assert one(exif(order, [(ORIENTATION, 3, 0, 6)])) == 1
    assert one(exif(order, [(ORIENTATION, 3, 1, 0)])) == 1    # value 0
    assert one(exif(order, [(ORIENTATION, 3, 1, 9)])) == 1    # value 9
    assert one(exif(order, [(ORIENTATION, 3, 1, 0x0600)])) == 1  # the other byte order's 6
    assert one(exif(order, [(0x0110, 3, 1, 6)])) == 1          # no orientation tag
    assert one(app1(b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta/>")) == 1  # a non-Exif APP1 (XMP)
    good = b"Exif\0\0" + tiff(order, [(ORIENTATION, 3, 1, 6)])
    assert one(app1(good)) == 6
    e = "<" if order == "II" else ">"
    for off in (len(good) - 6, len(good) - 6 - 1, len(good) - 6 - 13, 0xFFFFFFFF, 0x7FFFFFF0):  # IFD outside the segment
        bad = good[:10] + struct.pack(e + "I", off) + good[14:]
        assert one(app1(bad)) == 1, off
    for cut in range(0, len(good) - 4):  # a segment that ends anywhere inside the entry (the last 4 bytes: next IFD)
        assert one(app1(good[:cut])) == 1, cut
    assert one(app1(good[:6] + b"XX" + good[8:])) == 1          # neither II nor MM
    assert one(app1(good[:8] + b"\0\0" + good[10:])) == 1        # not 42
    # the first Exif segment decides
    assert one(exif(order, [(ORIENTATION, 3, 1, 9)]) + exif(order, [(ORIENTATION, 3, 1, 6)])) == 1
    # behind the first SOS nothing counts
    sos = jpeg.index(b"\xff\xda")
    assert C.jpeg_orientation(jpeg[:sos] + jpeg[sos:-2] + app1(good) + jpeg[-2:]) == 1
    assert C.jpeg_orientation(b"") == 1 and C.jpeg_orientation(b"\xff") == 1 and C.jpeg_orientation(b"P6 1 1 255 abc") == 1
    assert C.jpeg_orientation(b"\xff\xd8\xff\xe1\xff\xff") == 1


@pytest.mark.parametrize("order", ["II", "MM"])
def test_jpeg_orientation_of_every_proper_prefix(jpeg, order):
    tagged = splice(jpeg, exif(order, [(0x0110, 3, 1, 7), (ORIENTATION, 3, 1, 6)]))
    assert C.jpeg_orientation(tagged) == 6
    for n in range(len(tagged)):
        assert C.jpeg_orientation(tagged[:n]) == 1, n


# ---- end to end ----
def run_json(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.skipif(not os.path.exists(STRIPE), reason="bin/stripe not built")
def test_cli_orient_auto_on_tagged_files(tmp_path, jpeg):
    stored = C.decode_jpeg(jpeg)
    plain = str(tmp_path / "plain.jpg")
    open(plain, "wb").write(jpeg)
    for v in range(1, 9):
        src = str(tmp_path / f"tag{v}.jpg")
        open(src, "wb").write(splice(jpeg, exif("MM" if v % 2 else "II", [(ORIENTATION, 3, 1, v)])))
        dst = str(tmp_path / f"out{v}.ppm")
        j = run_json([STRIPE, "convert", "--input", src, "--output", dst, "--orient", "auto", "--backend", "host"])
        ref = np_orient(stored, NAMES[v - 1])
        assert (C.read_pnm(dst) == ref).all(), v
        assert j["oriented"] == NAMES[v - 1] and j["cropped_from"] == [24, 16]
        assert (j["W"], j["H"]) == (ref.shape[1], ref.shape[0])
        # without --orient nothing changes: the stored pixels, and no new JSON member
        j = run_json([STRIPE, "convert", "--input", src, "--output", dst, "--backend", "host"])
        assert (C.read_pnm(dst) == stored).all() and "oriented" not in j and "cropped_from" not in j
        # the Python CLI (an identity chain)
        pdst = str(tmp_path / f"py{v}.ppm")
        j = run_json([sys.executable, "-m", "mpi_cuda_imagemanipulation_amd", "run", "--input", src, "--output", pdst,
                      "--orient", "auto", "--backend", "host", "--chain", "invert,invert"])
        assert (C.read_pnm(pdst) == ref).all(), v
        assert j["oriented"] == NAMES[v - 1] and j["cropped_from"] == [24, 16] and j["shape"] == list(ref.shape)
    # auto on a file without the tag, and on a format that has none
    j = run_json([STRIPE, "convert", "--input", plain, "--output", dst, "--orient", "auto", "--backend", "host"])
    assert j["oriented"] == "none" and (C.read_pnm(dst) == stored).all()
    ppm = str(tmp_path / "a.ppm")
    C.write_pnm(ppm, stored)
    j = run_json([STRIPE, "convert", "--input", ppm, "--output", dst, "--orient", "auto", "--backend", "host"])
    assert j["oriented"] == "none" and (C.read_pnm(dst) == stored).all()
    # a written JPEG carries no Exif: upright by construction
    out_jpg = str(tmp_path / "upright.jpg")
    run_json([STRIPE, "convert", "--input", str(tmp_path / "tag6.jpg"), "--output", out_jpg, "--orient", "auto",
              "--backend", "host"])
    assert m.ops.exif_orientation(out_jpg) == 1 and C.decode_jpeg(open(out_jpg, "rb").read()).shape == (24, 16, 3)


@pytest.mark.skipif(not os.path.exists(STRIPE), reason="bin/stripe not built")
def test_cli_orient_crop_resize_chain_order(tmp_path):
    a = coord_frame(60, 40, 3)
    src, held, dst, pdst = (str(tmp_path / n) for n in ("a.ppm", "h.ppm", "out.ppm", "py.ppm"))
    C.write_pnm(src, a)
    C.write_pnm(held, 255 - a)
    # decode -> orient -> crop -> resize -> chain
    ref = C.golden_apply(C.golden_resize(np_orient(a, "rot90", (4, 6, 30, 50)), 15, 25, "auto"), "gaussian3",
                         "reflect101", True)
    args = ["--input", src, "--orient", "cw", "--crop", "30x50+4+6", "--resize", "15x25", "--chain", "gaussian3",
            "--backend", "host"]
    j = run_json([STRIPE, "run", *args, "--output", dst])
    assert (C.read_pnm(dst) == ref).all()
    assert j["oriented"] == "rot90" and j["cropped_from"] == [60, 40] and j["resized_from"] == [30, 50]
    j = run_json([sys.executable, "-m", "mpi_cuda_imagemanipulation_amd", "run", *args, "--output", pdst])
    assert (C.read_pnm(pdst) == ref).all()
    assert j["oriented"] == "rot90" and j["cropped_from"] == [60, 40] and j["resized_from"] == [30, 50]
    # --crop alone is the `none` orientation; --held's image is treated the same way
    j = run_json([STRIPE, "run", "--input", src, "--held", held, "--crop", "20x10+7+3", "--chain", "absdiff",
                  "--backend", "host", "--output", dst])
    w = a[3:13, 7:27].astype(int)
    assert j["oriented"] == "none" and (C.read_pnm(dst) == np.abs(w - (255 - w))).all()
    # refusals name the token and the frame
    r = subprocess.run([STRIPE, "convert", "--input", src, "--output", dst, "--orient", "rot90", "--crop", "41x1+0+0",
                        "--backend", "host"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "'41x1+0+0'" in r.stderr and "40x60" in r.stderr
    r = subprocess.run([STRIPE, "convert", "--input", src, "--output", dst, "--orient", "rot91", "--backend", "host"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "'rot91'" in r.stderr
