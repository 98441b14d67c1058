"""The launch decision of the warp family (k_warp, csrc/hip/launch_policy.h
Family::Warp) through `_C.launch_policy`: the orient family's size rule on the
pixels of both frames, (W * rows + W2 * rows2) * C bytes against kNtMinBytes
(224 MiB = 234881024).  With the source W = 16384 and a destination of the same
size (a rotation with `same`):
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
    kw.setdefault("W2", W)
    kw.setdefault("rows2", rows)
    return C.launch_policy("warp", cin=cc, cout=cc, cmid=cc, W=W, rows=rows, **kw)


@pytest.fixture
def no_nt(monkeypatch):
    monkeypatch.delenv("STRIPE_NT", raising=False)


@pytest.mark.parametrize("cc,at,above", CASES)
def test_row_pair(no_nt, cc, at, above):
    assert 2 * W * at * cc <= MIN < 2 * W * above * cc  # the pair brackets the family's own formula
    lo, hi = policy(cc, at), policy(cc, above)
    assert lo == dict(nt_stores=False, streaming=False, nxcd=0, cap=0, cap_applied=False)
    assert hi == dict(nt_stores=True, streaming=True, nxcd=0, cap=0, cap_applied=False)
    # PassLaunch::nt / wgs (the stencil autotuner's fields) are not consulted
    assert policy(cc, at, nt=1, wgs=2) == lo and policy(cc, above, nt=0, wgs=2) == hi


def test_both_frames_count(no_nt):
    # source 16384 x 2389 RGB alone is half the threshold: the destination decides
    p = lambda W2, rows2: C.launch_policy("warp", cin=3, W=W, rows=2389, W2=W2, rows2=rows2)  # noqa: E731
    assert not p(W, 2389)["streaming"] and p(W, 2390)["streaming"] and not p(1, 1)["streaming"]
    # 16384 * 2389 = 39141376 source pixels; MIN / 3 = 78293674.67: the destination tips it from 39152299 pixels
    assert (W * 2389 + 39152298) * 3 <= MIN < (W * 2389 + 39152299) * 3
    assert not p(39152298, 1)["streaming"] and p(39152299, 1)["streaming"]
    assert not p(2, 19576149)["streaming"] and p(3, 13050767)["streaming"]  # 39152298 | 39152301 pixels
    # a small destination of a large source streams too (the source is read at most once)
    assert C.launch_policy("warp", cin=3, W=W, rows=W, W2=64, rows2=64)["streaming"]


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
    o = lambda rows: C.launch_policy("orient", cin=3, W=W, rows=rows, W2=W, rows2=rows)  # noqa: E731
    assert not o(2389)["streaming"] and o(2390)["streaming"]
    with pytest.raises(RuntimeError, match="unknown kernel family"):
        C.launch_policy("warp2")
