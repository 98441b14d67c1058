"""The launch decision of the orientation family (k_orient, csrc/hip/launch_policy.h
Family::Orient) through `_C.launch_policy`.  The kernel reads the source window
once and writes as many pixels once: 2 * W * rows * C bytes against kNtMinBytes
(224 MiB = 234881024).  At W = 16384:
  RGB : 234881024 / (16384 * 3 * 2) = 2389.3 -> rows 2389 | 2390
  gray: 234881024 / (16384 * 2)     = 7168   -> rows 7168 | 7169
Expected values are written out; nothing is computed by the code under test.
STRIPE_NT is read at every launch, so it is set in-process.  No GPU."""
import pytest

import mpi_cuda_imagemanipulation_amd as m

C = m._C
W = 16384
MIN = 224 << 20
CASES = [(3, 2389, 2390), (1, 7168, 7169)]


def policy(cc, rows, **kw):
    return C.launch_policy("orient", cin=cc, cout=cc, cmid=cc, W=W, rows=rows, **kw)


@pytest.fixture
def no_nt(monkeypatch):
    monkeypatch.delenv("STRIPE_NT", raising=False)


@pytest.mark.parametrize("cc,at,above", CASES)
def test_row_pair(no_nt, cc, at, above):
    assert 2 * W * at * cc <= MIN < 2 * W * above * cc  # the pair brackets the family's own formula
    lo, hi = policy(cc, at), policy(cc, above)
    assert lo == dict(nt_stores=False, streaming=False, nxcd=0, cap=0, cap_applied=False)
    assert hi == dict(nt_stores=True, streaming=True, nxcd=0, cap=0, cap_applied=False)
    # PassLaunch::nt / wgs (the stencil autotuner's fields) and a resize's destination are not consulted
    assert policy(cc, at, nt=1, wgs=2, W2=W, rows2=at) == lo and policy(cc, above, nt=0, wgs=2) == hi


def test_the_window_counts_not_the_frame(no_nt):
    # the policy sees the source window of a crop: the same pixels whichever way they are turned
    assert not C.launch_policy("orient", cin=3, W=4096, rows=4096)["streaming"]
    assert C.launch_policy("orient", cin=3, W=2390, rows=16384)["streaming"]
    assert not C.launch_policy("orient", cin=3, W=2389, rows=16384)["streaming"]


@pytest.mark.parametrize("cc,at,above", CASES)
def test_stripe_nt_overrides_both_ways(monkeypatch, no_nt, cc, at, above):
    monkeypatch.setenv("STRIPE_NT", "1")
    lo, hi = policy(cc, at), policy(cc, above)
    assert lo["nt_stores"] and not lo["streaming"] and hi["nt_stores"] and hi["streaming"]
    monkeypatch.setenv("STRIPE_NT", "0")
    lo, hi = policy(cc, at), policy(cc, above)
    assert not lo["nt_stores"] and not lo["streaming"] and not hi["nt_stores"] and hi["streaming"]


def test_other_families_unchanged(no_nt):
    r = lambda rows: C.launch_policy("resize", cin=3, W=W, rows=rows, W2=W // 2, rows2=rows // 2)  # noqa: E731
    assert not r(3822)["streaming"] and r(3824)["streaming"]
    with pytest.raises(RuntimeError, match="unknown kernel family"):
        C.launch_policy("orient2")
