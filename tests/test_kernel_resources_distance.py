"""Static resources of the distance-transform kernels (csrc/hip/distance.hip):
every k_edt_* kernel the launchers use is in build/kernel_resources.json, none
uses scratch, spills or a dynamic stack, and each one's LDS is what
stripe/kernels.h says (edt_row_lds_bytes per width class; the column pass uses
none)."""
import json
import os

import pytest

import mpi_cuda_imagemanipulation_amd as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "build", "kernel_resources.json")
# name -> instances: k_edt_bits<aligned>, k_edt_row<width class, store>
KERNELS = {"k_edt_bits": 2, "k_edt_carry": 1, "k_edt_band": 1, "k_edt_row": 9}


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(REPORT):
        pytest.skip("build/kernel_resources.json missing (run python tools/build.py)")
    with open(REPORT) as f:
        rep = json.load(f)
    return {k: v for k, v in rep.items() if "k_edt_" in k}


def instances(report, name):
    # the mangled name carries the length of the plain one: 10k_edt_band, then E (plain) or I (template arguments)
    return {k: v for k, v in report.items() if f"{len(name)}{name}E" in k or f"{len(name)}{name}I" in k}


def test_every_kernel_reported(report):
    for name, count in KERNELS.items():
        hits = instances(report, name)
        assert len(hits) == count, (name, sorted(hits))
        assert all(v["source"] == "hip/distance.hip" for v in hits.values()), name
    assert len(report) == sum(KERNELS.values()), sorted(report)


def test_no_scratch_no_spills_no_dynamic_stack(report):
    assert report
    for k, v in report.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["Dynamic Stack"] == "False", (k, v)


def test_lds_is_what_the_header_says(report):
    lds = m._C.distance_lds()
    assert sorted(lds) == sorted(m._C.distance_widths())
    for name in ("k_edt_bits", "k_edt_carry", "k_edt_band"):
        for k, v in instances(report, name).items():
            assert v["LDS Size [bytes/block]"] == 0, k
    rows = instances(report, "k_edt_row")
    for w, nbytes in lds.items():
        hits = {k: v for k, v in rows.items() if f"k_edt_rowILi{w}ELi" in k}
        assert len(hits) == 3, (w, sorted(hits))
        for k, v in hits.items():
            assert v["LDS Size [bytes/block]"] == nbytes == 4 * w + 2048 + 80, (k, v["LDS Size [bytes/block]"])
