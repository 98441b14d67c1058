"""Static resources of the combine kernel (k_combine, csrc/hip/combine.hip) from
build/kernel_resources.json: every instance (8 ops x store policy x post
table) is reported, none uses scratch or spills a register, and only the
instances with a post table hold LDS."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "build", "kernel_resources.json")


@pytest.fixture(scope="module")
def combine():
    assert os.path.exists(REPORT), "build/kernel_resources.json missing (run python tools/build.py)"
    with open(REPORT) as f:
        rep = json.load(f)
    return {k: v for k, v in rep.items() if "k_combine" in k}


def test_every_instance_reported(combine):
    # _ZN6stripe3dev9k_combineILi<op>ELb<nt>ELb<lut>EE...
    seen = set()
    for k, v in combine.items():
        mm = re.search(r"k_combineILi(\d)ELb([01])ELb([01])E", k)
        assert mm, k
        seen.add(tuple(int(g) for g in mm.groups()))
        assert v["source"] == "hip/combine.hip"
    assert seen == {(op, nt, lut) for op in range(8) for nt in (0, 1) for lut in (0, 1)}


def test_no_scratch_no_spills(combine):
    assert combine
    for k, v in combine.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v.get("Dynamic Stack", "False") == "False", k
        assert v["VGPRs"] <= 64 and v["Occupancy [waves/SIMD]"] >= 8, (k, v)


def test_lds_only_with_a_post_table(combine):
    for k, v in combine.items():
        lut = re.search(r"ELb[01]ELb([01])E", k).group(1) == "1"
        assert v["LDS Size [bytes/block]"] == (256 if lut else 0), (k, v)
