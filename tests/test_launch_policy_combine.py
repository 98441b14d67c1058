"""The launch decision of the combine family (k_combine, csrc/hip/launch_policy.h
Family::Combine) through `_C.launch_policy`.  A combine pass reads two images
and writes one: 3 * C bytes a pixel against kNtMinBytes (224 MiB).  At
W = 16384 that puts the row pair at / above the threshold at
  RGB  (9 bytes a pixel): 224 MiB / (16384 * 9) = 1592.9 -> rows 1592 | 1593
  gray (3 bytes a pixel): 224 MiB / (16384 * 3) = 4778.7 -> rows 4778 | 4779
(a family that took the flat passes' 2 * C formula would put RGB at 2389 | 2390).
Expected values are written out; nothing is computed by the code under test.
STRIPE_NT is read at every launch, so it is set in-process.  No GPU."""
import pytest

import mpi_cuda_imagemanipulation_amd as m

C = m._C
W = 16384
MIN = 224 << 20
CASES = [(3, 1592, 1593), (1, 4778, 4779)]
CAP = 2  # the family's residency cap (kPwWgsCombine, profiles/combine/README.md)


def policy(cc, rows, **kw):
    return C.launch_policy("combine", cin=cc, cout=cc, cmid=cc, W=W, rows=rows, **kw)


@pytest.fixture
def no_nt(monkeypatch):
    monkeypatch.delenv("STRIPE_NT", raising=False)
    monkeypatch.delenv("STRIPE_PW_WGS", raising=False)


@pytest.mark.parametrize("cc,at,above", CASES)
def test_row_pair(no_nt, cc, at, above):
    assert at * W * 3 * cc <= MIN < above * W * 3 * cc  # the pair brackets the family's own formula
    lo, hi = policy(cc, at), policy(cc, above)
    assert lo == dict(nt_stores=False, streaming=False, nxcd=0, cap=CAP, cap_applied=False)
    assert hi == dict(nt_stores=True, streaming=True, nxcd=0, cap=CAP, cap_applied=True)
    # PassLaunch::nt / wgs (the stencil autotuner's fields) are not consulted
    assert policy(cc, at, nt=1, wgs=2) == lo and policy(cc, above, nt=0, wgs=2) == hi


@pytest.mark.parametrize("cc,at,above", CASES)
def test_stripe_nt_overrides_both_ways(monkeypatch, no_nt, cc, at, above):
    monkeypatch.setenv("STRIPE_NT", "1")
    lo, hi = policy(cc, at), policy(cc, above)
    assert lo["nt_stores"] and not lo["streaming"] and not lo["cap_applied"]  # nt on; the cap needs the size too
    assert hi["nt_stores"] and hi["streaming"] and hi["cap_applied"]
    monkeypatch.setenv("STRIPE_NT", "0")
    lo, hi = policy(cc, at), policy(cc, above)
    assert not lo["nt_stores"] and not lo["streaming"] and not lo["cap_applied"]
    assert not hi["nt_stores"] and hi["streaming"] and not hi["cap_applied"]  # default stores: no cap


def test_other_families_unchanged(no_nt):
    # the flat family keeps its 2 * C formula: RGB rows 2389 | 2390
    f = lambda rows: C.launch_policy("pointwise_flat", cin=3, cout=3, cmid=3, W=W, rows=rows)  # noqa: E731
    assert not f(2389)["streaming"] and f(2390)["streaming"]
    with pytest.raises(RuntimeError, match="unknown kernel family"):
        C.launch_policy("combine2")
