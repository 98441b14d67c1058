"""Static resources of the bilateral kernel (k_bilateral, csrc/hip/bilateral_kernels.h)
from build/kernel_resources.json: every instance the launcher can pick is
reported from hip/stencil_inst_f.hip, none uses scratch or spills a register,
each reaches the waves per SIMD its __launch_bounds__ asks for, and its LDS is
the three LUTs, the mirrored range table and, with the expand epilogue, the
re-tiling buffer."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "build", "kernel_resources.json")
PRO_GRAY, PRO_GRAYLUT = 2, 3


@pytest.fixture(scope="module")
def bilateral():
    assert os.path.exists(REPORT), "build/kernel_resources.json missing (run python tools/build.py)"
    with open(REPORT) as f:
        rep = json.load(f)
    out = {}
    for k, v in rep.items():
        if "k_bilateral" not in k:
            continue
        # _ZN6stripe3dev11k_bilateralILi<C>ENS_4sdef10Bilateral<K>ELi<PRO>ELb<SKIP>ELi<SAUX>ELb<EXP>EE...
        mm = re.search(r"k_bilateralILi(\d)ENS_4sdef10Bilateral(\d)ELi(\d)ELb([01])ELi(\d)ELb([01])E", k)
        assert mm, k
        out[tuple(int(g) for g in mm.groups())] = v
    return out


def test_every_instance_reported(bilateral):
    want = set()
    for K in (3, 5):
        for skip in (0, 1):
            for saux in (0, 2):
                want |= {(3, K, pro, skip, saux, 0) for pro in (0, 1)}  # RGB: plain / LUT prologue
                want |= {(1, K, pro, skip, saux, ex) for pro in (0, 1, 2, 3) for ex in (0, 1)}
    assert set(bilateral) == want
    assert all(v["source"] == "hip/stencil_inst_f.hip" for v in bilateral.values())


def test_no_scratch_no_spills(bilateral):
    assert bilateral
    for k, v in bilateral.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v.get("Dynamic Stack", "False") == "False", k


def test_occupancy_meets_launch_bounds(bilateral):
    for (C, K, pro, skip, saux, ex), v in bilateral.items():
        asked = 2 if K == 5 else 3 if pro in (PRO_GRAY, PRO_GRAYLUT) else 4  # k_bilateral's __launch_bounds__
        assert v["Occupancy [waves/SIMD]"] >= asked, ((C, K, pro, skip, saux, ex), v)
        assert v["VGPRs"] <= 512 // asked, ((C, K, pro, skip, saux, ex), v)


def test_lds(bilateral):
    for (C, K, pro, skip, saux, ex), v in bilateral.items():
        # 768 B of LUTs + 512 B mirrored range table; expand: 4 waves x 3 KiB of re-tiling buffer
        assert v["LDS Size [bytes/block]"] == 1280 + (12288 if ex else 0), ((C, K, pro, skip, saux, ex), v)
