"""Static resources of the mesh warp kernel (k_remap, csrc/hip/remap.hip) from
build/kernel_resources.json: every instance (channels x mode x border x
{nodes from global memory, nodes in LDS} x store policy) is reported, none uses
scratch or spills a register, and each holds exactly the LDS its layout
declares (`_C.remap_tile`: k_warp's staged box, 92 rows of 23 dwords gray / 69
dwords RGB, plus 17 x 17 nodes of two int32 and four waves' minima and maxima
for the instances with nodes in LDS, none for the others).

Recorded from the shipped build (hipcc, gfx950), VGPRs (the same for both store
policies) and waves per SIMD:

                      LDS gray   LDS RGB    global gray  global RGB
  nearest constant    42 / 8     52 / 5     87 / 5       89 / 5
  nearest replicate   39 / 8     52 / 5     83 / 5       86 / 5
  bilinear constant   54 / 8     59 / 5     106 / 4      117 / 4
  bilinear replicate  49 / 8     63 / 5     94 / 5       107 / 4

The RGB instances with nodes in LDS are held at 5 waves per SIMD by their 27768
B of LDS (five workgroups of 256 threads in 160 KiB; k_warp's 25392 B allow
six).  The registers are bounds here, not pins: the waves per SIMD are what a
change must not lose."""
import json
import os
import re

import pytest

import mpi_cuda_imagemanipulation_amd as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "build", "kernel_resources.json")
TILE = m._C.remap_tile()
# (C, bilinear, replicate, nodes in LDS) -> (VGPRs, waves per SIMD)
RECORDED = {
    (1, 0, 0, 1): (42, 8), (3, 0, 0, 1): (52, 5), (1, 0, 0, 0): (87, 5), (3, 0, 0, 0): (89, 5),
    (1, 0, 1, 1): (39, 8), (3, 0, 1, 1): (52, 5), (1, 0, 1, 0): (83, 5), (3, 0, 1, 0): (86, 5),
    (1, 1, 0, 1): (54, 8), (3, 1, 0, 1): (59, 5), (1, 1, 0, 0): (106, 4), (3, 1, 0, 0): (117, 4),
    (1, 1, 1, 1): (49, 8), (3, 1, 1, 1): (63, 5), (1, 1, 1, 0): (94, 5), (3, 1, 1, 0): (107, 4),
}


@pytest.fixture(scope="module")
def remap():
    assert os.path.exists(REPORT), "build/kernel_resources.json missing (run python tools/build.py)"
    with open(REPORT) as f:
        rep = json.load(f)
    return {k: v for k, v in rep.items() if "k_remap" in k}


def parse(k):
    # _ZN6stripe3dev7k_remapILi<C>ELb<bilinear>ELb<replicate>ELb<nodes in LDS>ELb<nt>EE...
    mm = re.search(r"k_remapILi(\d)ELb([01])ELb([01])ELb([01])ELb([01])E", k)
    assert mm, k
    return tuple(int(g) for g in mm.groups())


def test_every_instance_reported(remap):
    seen = set()
    for k, v in remap.items():
        seen.add(parse(k))
        assert v["source"] == "hip/remap.hip"
    assert seen == {(*s, nt) for s in RECORDED for nt in (0, 1)} and len(seen) == 32


def test_no_scratch_no_spills(remap):
    assert remap
    for k, v in remap.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v.get("Dynamic Stack", "False") == "False", k


def test_lds_registers_and_occupancy(remap):
    # the layout, written out: the box of k_warp, 17 x 17 nodes of 8 bytes, 16 int32 of reduction
    W = m._C.warp_tile()
    assert TILE["nodes"] == 64 // TILE["lds_spacing"] + 1 == 17 and TILE["node_bytes"] == 17 * 17 * 8
    assert TILE["lds_gray"] == W["lds_gray"] + 2312 + 64 == 10840 and TILE["lds_rgb"] == W["lds_rgb"] + 2312 + 64 == 27768
    for k, v in remap.items():
        c, bil, rep, ln, _ = parse(k)
        lds = TILE["lds_gray" if c == 1 else "lds_rgb"] if ln else 0
        # (the compiler rounds each array up to its alignment: at most 8 bytes more)
        assert lds <= v["LDS Size [bytes/block]"] <= lds + 8, (k, v)
        vgprs, waves = RECORDED[(c, bil, rep, ln)]
        assert v["VGPRs"] <= vgprs and v["Occupancy [waves/SIMD]"] >= waves, (k, v)
