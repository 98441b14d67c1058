"""Static resources of the connected-component kernels (csrc/hip/components.hip):
every k_ccl_* kernel the launchers use is in build/kernel_resources.json, none
uses scratch, spills or a dynamic stack, and each one's LDS is what
stripe/kernels.h says (ccl_lds_bytes and its neighbours)."""
import json
import os

import pytest

import mpi_cuda_imagemanipulation_amd as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "build", "kernel_resources.json")
KERNELS = ("k_ccl_tile", "k_ccl_seam", "k_ccl_flatten", "k_ccl_scan", "k_ccl_number", "k_ccl_resolve",
           "k_ccl_stats_init", "k_ccl_stats", "k_ccl_stats_fix", "k_ccl_select")


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(REPORT):
        pytest.skip("build/kernel_resources.json missing (run python tools/build.py)")
    with open(REPORT) as f:
        rep = json.load(f)
    return {k: v for k, v in rep.items() if "k_ccl_" in k}


def instances(report, name):
    # the mangled name carries the length of the plain one: 10k_ccl_tile
    return {k: v for k, v in report.items() if f"{len(name)}{name}E" in k}


def test_every_kernel_reported_once(report):
    for name in KERNELS:
        hits = instances(report, name)
        assert len(hits) == 1, (name, sorted(hits))
        assert all(v["source"] == "hip/components.hip" for v in hits.values()), name
    assert len(report) == len(KERNELS), sorted(report)


def test_no_scratch_no_spills_no_dynamic_stack(report):
    assert report
    for k, v in report.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["Dynamic Stack"] == "False", (k, v)


def test_lds_is_what_the_header_says(report):
    lds = m._C.components_lds()
    tw, th = m._C.components_tile()
    assert lds["k_ccl_tile"] == tw * th * 4
    for name in KERNELS:
        (v,) = instances(report, name).values()
        assert v["LDS Size [bytes/block]"] == lds.get(name, 0), (name, v["LDS Size [bytes/block]"])
