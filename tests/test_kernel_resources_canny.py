"""Static resources of the canny kernels (csrc/hip/canny.hip): every k_canny_*
kernel the launchers use is in build/kernel_resources.json, none uses scratch,
spills or a dynamic stack, and each one's LDS is what _C.canny_lds() says."""
import json
import os

import pytest

import mpi_cuda_imagemanipulation_amd as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "build", "kernel_resources.json")
# name -> instances: nms <l1 | l2>; the others are no templates
KERNELS = {"k_canny_nms": 2, "k_canny_classify": 1, "k_canny_mark": 1, "k_canny_select": 1}


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(REPORT):
        pytest.skip("build/kernel_resources.json missing (run python tools/build.py)")
    with open(REPORT) as f:
        rep = json.load(f)
    return {k: v for k, v in rep.items() if "k_canny_" in k}


def instances(report, name):
    # the mangled name carries the length of the plain one, then I (template arguments) or E (none)
    return {k: v for k, v in report.items() if f"{len(name)}{name}I" in k or f"{len(name)}{name}E" in k}


def test_every_kernel_reported(report):
    for name, count in KERNELS.items():
        hits = instances(report, name)
        assert len(hits) == count, (name, sorted(hits))
        assert all(v["source"] == "hip/canny.hip" for v in hits.values()), name
    assert len(report) == sum(KERNELS.values()), sorted(report)


def test_no_scratch_no_spills_no_dynamic_stack(report):
    assert report
    for k, v in report.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["Dynamic Stack"] == "False", (k, v)


def test_lds_is_what_the_bindings_say(report):
    lds = m._C.canny_lds()
    assert sorted(lds) == sorted(KERNELS)
    for name, nbytes in lds.items():
        hits = instances(report, name)
        assert hits, name
        for k, v in hits.items():
            assert v["LDS Size [bytes/block]"] == nbytes, (k, v["LDS Size [bytes/block]"], nbytes)
