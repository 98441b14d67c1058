"""Static resources of the orientation kernel (k_orient, csrc/hip/orient.hip)
from build/kernel_resources.json: every instance (channels x {row copy, FX
through a tile, transposing tile} x store policy) is reported, none uses
scratch or spills a register, and each holds exactly the LDS its tile layout
declares (`_C.orient_tile`; transposing: 128 rows in groups of four, 33 / 49
dwords a row and one / two dwords of padding a group; FX: 64 rows of 65 / 97
dwords; none for the row copies).

Recorded from the shipped build (hipcc, gfx950): the row copies use 38 VGPRs
and run 8 waves per SIMD; the FX tile instances 56 VGPRs, the transposing ones
60; with 16640 / 17024 B of LDS the gray tile instances run 8 waves per SIMD,
with 24832 / 25344 B the RGB ones 6."""
import json
import os
import re

import pytest

import mpi_cuda_imagemanipulation_amd as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "build", "kernel_resources.json")
# (C, T, FX) of the instances; FX and FY of a transposing op are reflections inside the tile
SHAPES = [(c, t, fx) for c in (1, 3) for (t, fx) in ((0, 0), (0, 1), (1, 0))]
TILE = m._C.orient_tile()


@pytest.fixture(scope="module")
def orient():
    assert os.path.exists(REPORT), "build/kernel_resources.json missing (run python tools/build.py)"
    with open(REPORT) as f:
        rep = json.load(f)
    return {k: v for k, v in rep.items() if "k_orient" in k}


def parse(k):
    # _ZN6stripe3dev8k_orientILi<C>ELb<T>ELb<FX>ELb<nt>EE...
    mm = re.search(r"k_orientILi(\d)ELb([01])ELb([01])ELb([01])E", k)
    assert mm, k
    return tuple(int(g) for g in mm.groups())


def test_every_instance_reported(orient):
    seen = set()
    for k, v in orient.items():
        seen.add(parse(k))
        assert v["source"] == "hip/orient.hip"
    assert seen == {(*s, nt) for s in SHAPES for nt in (0, 1)}


def test_no_scratch_no_spills(orient):
    assert orient
    for k, v in orient.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v.get("Dynamic Stack", "False") == "False", k


def test_lds_and_occupancy(orient):
    # the layouts, written out.  Transposing: 32 groups of four rows, gray 4 * 33 + 1 dwords a group, RGB
    # 4 * 49 + 2; FX: 64 rows of 256 + 3 gray / 384 + 3 RGB bytes in whole dwords
    tt, tf = TILE["transposing"], TILE["fx"]
    assert tt["rows"] == 128 and tt["lds_gray"] == 32 * (4 * 33 + 1) * 4 and tt["lds_rgb"] == 32 * (4 * 49 + 2) * 4
    assert tf["rows"] == 64 and tf["lds_gray"] == 64 * 65 * 4 and tf["lds_rgb"] == 64 * 97 * 4
    for k, v in orient.items():
        c, t, fx, _ = parse(k)
        tiled = t or fx
        lds = (tt if t else tf)["lds_gray" if c == 1 else "lds_rgb"] if tiled else 0
        assert v["LDS Size [bytes/block]"] == lds, (k, v)
        assert v["VGPRs"] <= 64, (k, v)
        assert v["Occupancy [waves/SIMD]"] >= (8 if not tiled or c == 1 else 6), (k, v)
