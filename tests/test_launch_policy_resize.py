"""The launch decision of the resize family (k_resize, csrc/hip/launch_policy.h
Family::Resize) through `_C.launch_policy`.  A resize reads the source frame
once and writes the destination once: (W * rows + W2 * rows2) * C bytes against
kNtMinBytes (224 MiB = 234881024).  Halving a W = 16384 frame (W2 = 8192,
rows2 = rows / 2) moves 16384 * rows * C * 5 / 4 bytes:
  RGB : 234881024 / (16384 * 3 * 1.25) = 3822.9 -> rows 3822 | 3824
  gray: 234881024 / (16384 * 1.25)     = 11468.8 -> rows 11468 | 11470
(rows even, so that rows2 is exact).  Expected values are written out; nothing
is computed by the code under test.  STRIPE_NT is read at every launch, so it
is set in-process.  No GPU."""
import pytest

import mpi_cuda_imagemanipulation_amd as m

C = m._C
W = 16384
MIN = 224 << 20
CASES = [(3, 3822, 3824), (1, 11468, 11470)]


def policy(cc, rows, **kw):
    return C.launch_policy("resize", cin=cc, cout=cc, cmid=cc, W=W, rows=rows, W2=W // 2, rows2=rows // 2, **kw)


@pytest.fixture
def no_nt(monkeypatch):
    monkeypatch.delenv("STRIPE_NT", raising=False)


@pytest.mark.parametrize("cc,at,above", CASES)
def test_row_pair(no_nt, cc, at, above):
    bytes_of = lambda rows: (W * rows + (W // 2) * (rows // 2)) * cc  # noqa: E731
    assert bytes_of(at) <= MIN < bytes_of(above)  # the pair brackets the family's own formula
    lo, hi = policy(cc, at), policy(cc, above)
    assert lo == dict(nt_stores=False, streaming=False, nxcd=0, cap=0, cap_applied=False)
    assert hi == dict(nt_stores=True, streaming=True, nxcd=0, cap=0, cap_applied=False)
    # PassLaunch::nt / wgs (the stencil autotuner's fields) are not consulted
    assert policy(cc, at, nt=1, wgs=2) == lo and policy(cc, above, nt=0, wgs=2) == hi


def test_source_and_destination_both_count(no_nt):
    # an 8192^2 RGB frame is 192 MiB: below the threshold alone, above it with a 4096^2 destination
    p = lambda W2, rows2: C.launch_policy("resize", cin=3, W=8192, rows=8192, W2=W2, rows2=rows2)  # noqa: E731
    assert not p(1, 1)["streaming"] and not p(3344, 3344)["streaming"] and p(3345, 3345)["streaming"]
    assert 3 * (8192 * 8192 + 3344 * 3344) <= MIN < 3 * (8192 * 8192 + 3345 * 3345)
    # a 2x upscale of 4096^2 RGB: 48 MiB in, 192 MiB out
    assert C.launch_policy("resize", cin=3, W=4096, rows=4096, W2=8192, rows2=8192)["nt_stores"]


@pytest.mark.parametrize("cc,at,above", CASES)
def test_stripe_nt_overrides_both_ways(monkeypatch, no_nt, cc, at, above):
    monkeypatch.setenv("STRIPE_NT", "1")
    lo, hi = policy(cc, at), policy(cc, above)
    assert lo["nt_stores"] and not lo["streaming"] and hi["nt_stores"] and hi["streaming"]
    monkeypatch.setenv("STRIPE_NT", "0")
    lo, hi = policy(cc, at), policy(cc, above)
    assert not lo["nt_stores"] and not lo["streaming"] and not hi["nt_stores"] and hi["streaming"]


def test_other_families_unchanged(no_nt):
    # W2 / rows2 count for resize only: the flat family keeps its 2 * C formula, RGB rows 2389 | 2390
    f = lambda rows: C.launch_policy("pointwise_flat", cin=3, cout=3, cmid=3, W=W, rows=rows, W2=W, rows2=rows)  # noqa: E731
    assert not f(2389)["streaming"] and f(2390)["streaming"]
    with pytest.raises(RuntimeError, match="unknown kernel family"):
        C.launch_policy("resize2")
