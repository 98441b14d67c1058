"""The launch decision of the bilateral family (k_bilateral, csrc/hip/launch_policy.h
Family::Bilateral) through `_C.launch_policy`.  It starts from the rank family's
values: a stencil pass reads cin and writes cout bytes a pixel against
kNtMinBytes (224 MiB).  At W = 16384 that puts the row pair at / above the
threshold at
  RGB  (6 bytes a pixel): 224 MiB / (16384 * 6) = 2389.3 -> rows 2389 | 2390
  gray (2 bytes a pixel): 224 MiB / (16384 * 2) = 7168   -> rows 7168 | 7169
Streaming launches are capped at 3 workgroups per CU (kNtWgsDirect), none with a
gray prologue; cache-resident launches take the XCD-aware order, uncapped.
Expected values are written out; nothing is computed by the code under test.
STRIPE_NT is read at every launch, so it is set in-process.  No GPU."""
import pytest

import mpi_cuda_imagemanipulation_amd as m

C = m._C
W = 16384
MIN = 224 << 20
CASES = [(3, 2389, 2390), (1, 7168, 7169)]
CAP = 3  # the family's residency cap on streaming launches, as the rank family's


def policy(cc, rows, family="bilateral", **kw):
    return C.launch_policy(family, cin=cc, cout=cc, cmid=cc, W=W, rows=rows, **kw)


@pytest.fixture
def no_knobs(monkeypatch):
    monkeypatch.delenv("STRIPE_NT", raising=False)


@pytest.mark.parametrize("cc,at,above", CASES)
def test_row_pair(no_knobs, cc, at, above):
    assert at * W * 2 * cc <= MIN < above * W * 2 * cc  # the pair brackets the stencil formula
    lo, hi = policy(cc, at), policy(cc, above)
    assert lo == dict(nt_stores=False, streaming=False, nxcd=8, cap=0, cap_applied=False)
    assert hi == dict(nt_stores=True, streaming=True, nxcd=0, cap=CAP, cap_applied=True)
    # the engine's tuned fields count: PassLaunch::nt picks the policy, ::wgs the cap
    assert policy(cc, at, nt=1) == hi and policy(cc, above, nt=0) == lo
    assert policy(cc, above, wgs=2)["cap"] == 2 and policy(cc, above, wgs=0) == dict(hi, cap=0, cap_applied=False)
    # a gray prologue reads 3 bytes per output byte and takes no cap
    assert policy(cc, above, nt=1, gray_prologue=True) == dict(hi, cap=0, cap_applied=False)


@pytest.mark.parametrize("cc,at,above", CASES)
def test_stripe_nt_overrides_both_ways(monkeypatch, no_knobs, cc, at, above):
    monkeypatch.setenv("STRIPE_NT", "1")
    assert policy(cc, at)["nt_stores"] and policy(cc, at)["cap"] == CAP
    monkeypatch.setenv("STRIPE_NT", "0")
    assert not policy(cc, above)["nt_stores"] and policy(cc, above)["cap"] == 0


def test_other_families_unchanged(no_knobs):
    for cc, at, above in CASES:
        for fam, cap in (("rank", 3), ("direct", 3), ("sep", 2), ("sobel_rp", 2)):
            lo, hi = policy(cc, at, fam), policy(cc, above, fam)
            assert lo == dict(nt_stores=False, streaming=False, nxcd=8, cap=0, cap_applied=False), fam
            assert hi == dict(nt_stores=True, streaming=True, nxcd=0, cap=cap, cap_applied=True), fam
    # the combine family keeps its 3 * C formula (RGB rows 1592 | 1593) and its cap of 2
    f = lambda rows: C.launch_policy("combine", cin=3, cout=3, cmid=3, W=W, rows=rows)  # noqa: E731
    assert not f(1592)["streaming"] and f(1593) == dict(nt_stores=True, streaming=True, nxcd=0, cap=2, cap_applied=True)
    # the flat family its 2 * C formula: RGB rows 2389 | 2390
    g = lambda rows: C.launch_policy("pointwise_flat", cin=3, cout=3, cmid=3, W=W, rows=rows)  # noqa: E731
    assert not g(2389)["streaming"] and g(2390)["streaming"]
    with pytest.raises(RuntimeError, match="unknown kernel family"):
        C.launch_policy("bilateral2")
