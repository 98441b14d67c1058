"""The launch decision of the mesh warp family (k_remap, csrc/hip/launch_policy.h
Family::Remap) through `_C.launch_policy`: the warp family's rule with the mesh
bytes added, (W * rows + W2 * rows2) * C + mesh_bytes against kNtMinBytes
(224 MiB = 234881024).  With the source W = 16384 and a destination of the same
size:
  RGB : 234881024 / (16384 * 3 * 2) = 2389.3 -> rows 2389 | 2390 without a mesh;
        rows 2389 leave 234881024 - 234848256 = 32768 bytes: a mesh of 32768
        bytes stays below, one of 32769 streams
  gray: 234881024 / (16384 * 2) = 7168 exactly -> rows 7168 without a mesh is
        at the threshold (not above): one more byte of mesh streams
Expected values are written out; nothing is computed by the code under test.
STRIPE_NT is read at every launch, so it is set in-process.  No GPU."""
import pytest

import mpi_cuda_imagemanipulation_amd as m

C = m._C
W = 16384
MIN = 224 << 20


def policy(cc, rows, mesh_bytes=0, **kw):
    kw.setdefault("W2", W)
    kw.setdefault("rows2", rows)
    return C.launch_policy("remap", cin=cc, cout=cc, cmid=cc, W=W, rows=rows, mesh_bytes=mesh_bytes, **kw)


@pytest.fixture
def no_nt(monkeypatch):
    monkeypatch.delenv("STRIPE_NT", raising=False)


LO = dict(nt_stores=False, streaming=False, nxcd=0, cap=0, cap_applied=False)
HI = dict(nt_stores=True, streaming=True, nxcd=0, cap=0, cap_applied=False)


def test_threshold_includes_the_mesh_bytes(no_nt):
    assert 2 * W * 2389 * 3 == 234848256 and MIN - 234848256 == 32768
    assert policy(3, 2389) == LO and policy(3, 2390) == HI
    assert policy(3, 2389, 32768) == LO and policy(3, 2389, 32769) == HI
    assert 2 * W * 7168 == MIN
    assert policy(1, 7168) == LO and policy(1, 7168, 1) == HI and policy(1, 7169) == HI
    # a full map of spacing 1 for a 4096 x 4096 gray destination: 4097 * 4097 * 8 = 134283272 bytes of mesh
    # beside 2 * 16777216 bytes of pixels: 167837704, below; at 5000 x 5000, 5001 * 5001 * 8 + 50000000 = 250080008
    full = lambda n: C.launch_policy("remap", cin=1, W=n, rows=n, W2=n, rows2=n, mesh_bytes=(n + 1) * (n + 1) * 8)  # noqa: E731
    assert not full(4096)["streaming"] and full(5000)["streaming"]
    # PassLaunch::nt / wgs (the stencil autotuner's fields) are not consulted
    assert policy(3, 2389, nt=1, wgs=2) == LO and policy(3, 2390, nt=0, wgs=2) == HI


def test_stripe_nt_overrides_both_ways(monkeypatch, no_nt):
    monkeypatch.setenv("STRIPE_NT", "1")
    lo, hi = policy(3, 2389), policy(3, 2390)
    assert lo["nt_stores"] and not lo["streaming"] and hi["nt_stores"] and hi["streaming"]
    monkeypatch.setenv("STRIPE_NT", "0")
    lo, hi = policy(3, 2389), policy(3, 2390)
    assert not lo["nt_stores"] and not lo["streaming"] and not hi["nt_stores"] and hi["streaming"]


def test_other_families_unchanged(no_nt):
    w = lambda rows, **kw: C.launch_policy("warp", cin=3, W=W, rows=rows, W2=W, rows2=rows, **kw)  # noqa: E731
    assert not w(2389)["streaming"] and w(2390)["streaming"]
    assert not w(2389, mesh_bytes=1 << 30)["streaming"]  # the mesh bytes count for remap alone
    r = lambda rows: C.launch_policy("resize", cin=3, W=W, rows=rows, W2=W // 2, rows2=rows // 2, mesh_bytes=1 << 30)  # noqa: E731
    assert not r(3822)["streaming"] and r(3824)["streaming"]
    o = lambda rows: C.launch_policy("orient", cin=3, W=W, rows=rows, W2=W, rows2=rows, mesh_bytes=1 << 30)  # noqa: E731
    assert not o(2389)["streaming"] and o(2390)["streaming"]
    with pytest.raises(RuntimeError, match="unknown kernel family"):
        C.launch_policy("remap2")
