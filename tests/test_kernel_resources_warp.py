"""Static resources of the warp kernel (k_warp, csrc/hip/warp.hip) from
build/kernel_resources.json: every instance (channels x mode x border x
{direct, staged} x store policy) is reported, none uses scratch or spills a
register, and each holds exactly the LDS its layout declares (`_C.warp_tile`:
92 rows of 23 dwords gray / 69 dwords RGB for the staged instances, none for the
direct ones).

Recorded from the shipped build (hipcc, gfx950), VGPRs (the same for both store
policies) and waves per SIMD:

                      staged gray  staged RGB   direct gray  direct RGB
  nearest constant    39 / 8       52 / 6       36 / 8       42 / 8
  nearest replicate   39 / 8       52 / 6       34 / 8       39 / 8
  bilinear constant   41 / 8       76 / 6       60 / 8       94 / 5
  bilinear replicate  39 / 8       52 / 6       62 / 8       63 / 8

The staged RGB instances are held at 6 waves per SIMD by their 25392 B of LDS
(six workgroups of 256 threads in 160 KiB)."""
import json
import os
import re

import pytest

import mpi_cuda_imagemanipulation_amd as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "build", "kernel_resources.json")
TILE = m._C.warp_tile()
# (C, bilinear, replicate, staged) -> (VGPRs, waves per SIMD)
RECORDED = {
    (1, 0, 0, 1): (39, 8), (3, 0, 0, 1): (52, 6), (1, 0, 0, 0): (36, 8), (3, 0, 0, 0): (42, 8),
    (1, 0, 1, 1): (39, 8), (3, 0, 1, 1): (52, 6), (1, 0, 1, 0): (34, 8), (3, 0, 1, 0): (39, 8),
    (1, 1, 0, 1): (41, 8), (3, 1, 0, 1): (76, 6), (1, 1, 0, 0): (60, 8), (3, 1, 0, 0): (94, 5),
    (1, 1, 1, 1): (39, 8), (3, 1, 1, 1): (52, 6), (1, 1, 1, 0): (62, 8), (3, 1, 1, 0): (63, 8),
}


@pytest.fixture(scope="module")
def warp():
    assert os.path.exists(REPORT), "build/kernel_resources.json missing (run python tools/build.py)"
    with open(REPORT) as f:
        rep = json.load(f)
    return {k: v for k, v in rep.items() if "k_warp" in k}


def parse(k):
    # _ZN6stripe3dev6k_warpILi<C>ELb<bilinear>ELb<replicate>ELb<staged>ELb<nt>EE...
    mm = re.search(r"k_warpILi(\d)ELb([01])ELb([01])ELb([01])ELb([01])E", k)
    assert mm, k
    return tuple(int(g) for g in mm.groups())


def test_every_instance_reported(warp):
    seen = set()
    for k, v in warp.items():
        seen.add(parse(k))
        assert v["source"] == "hip/warp.hip"
    assert seen == {(*s, nt) for s in RECORDED for nt in (0, 1)} and len(seen) == 32


def test_no_scratch_no_spills(warp):
    assert warp
    for k, v in warp.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v.get("Dynamic Stack", "False") == "False", k


def test_lds_registers_and_occupancy(warp):
    # the layout, written out: 92 staged rows of 92 gray / 276 RGB bytes, an odd number of whole dwords
    assert TILE["box"] == 92 and TILE["row_bytes_gray"] == 23 * 4 and TILE["row_bytes_rgb"] == 69 * 4
    assert TILE["lds_gray"] == 92 * 23 * 4 and TILE["lds_rgb"] == 92 * 69 * 4
    for k, v in warp.items():
        c, bil, rep, staged, _ = parse(k)
        lds = TILE["lds_gray" if c == 1 else "lds_rgb"] if staged else 0
        assert v["LDS Size [bytes/block]"] == lds, (k, v)
        vgprs, waves = RECORDED[(c, bil, rep, staged)]
        assert v["VGPRs"] == vgprs and v["Occupancy [waves/SIMD]"] == waves, (k, v)
