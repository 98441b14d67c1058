"""Static resources of the resize kernel (k_resize, csrc/hip/resize.hip) from
build/kernel_resources.json: every instance (channels x LDS class x store
policy) is reported, none uses scratch or spills a register, and each holds
exactly the LDS of its class.

Recorded from the shipped build (hipcc, gfx950): the instances with the taps
in registers (at most 2 per pixel) use 42 VGPRs, those with the weights in LDS
72; occupancy is bounded by LDS: 8 waves per SIMD at 4.5 KiB, 7 at 21 KiB, 4 at
36 KiB and 2 at 60 KiB."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "build", "kernel_resources.json")
# (taps in registers, source-span bytes, weight entries) -> least occupancy [waves/SIMD]
CLASSES = {(1, 4608, 0): 8, (1, 36864, 0): 4, (0, 9216, 6144): 7, (0, 36864, 12288): 2}


@pytest.fixture(scope="module")
def resize():
    assert os.path.exists(REPORT), "build/kernel_resources.json missing (run python tools/build.py)"
    with open(REPORT) as f:
        rep = json.load(f)
    return {k: v for k, v in rep.items() if "k_resize" in k}


def parse(k):
    # _ZN6stripe3dev8k_resizeILi<C>ELb<xs>ELi<src bytes>ELi<weights>ELb<nt>EE...
    mm = re.search(r"k_resizeILi(\d)ELb([01])ELi(\d+)ELi(\d+)ELb([01])E", k)
    assert mm, k
    return tuple(int(g) for g in mm.groups())


def test_every_instance_reported(resize):
    seen = set()
    for k, v in resize.items():
        seen.add(parse(k))
        assert v["source"] == "hip/resize.hip"
    assert seen == {(c, *cls, nt) for c in (1, 3) for cls in CLASSES for nt in (0, 1)}


def test_no_scratch_no_spills(resize):
    assert resize
    for k, v in resize.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v.get("Dynamic Stack", "False") == "False", k


def test_lds_and_occupancy_of_each_class(resize):
    for k, v in resize.items():
        _, xs, src, wn, _ = parse(k)
        assert v["LDS Size [bytes/block]"] == src + 2 * wn, (k, v)
        assert v["VGPRs"] <= (48 if xs else 80), (k, v)
        assert v["Occupancy [waves/SIMD]"] >= CLASSES[(xs, src, wn)], (k, v)
