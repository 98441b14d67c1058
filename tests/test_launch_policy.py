"""The launch decisions of the HIP kernel families (csrc/hip/launch_policy.h)
through `_C.launch_policy`: store policy, HBM-streaming verdict, XCD remap and
residency cap, per family, against the table the families were gathered from.
Expected values are written out here (`expected`), family by family; nothing
is computed by the code under test.  No GPU.

Per family, `bytes` is taken one pixel row at or below and one above
kNtMinBytes (224 MiB) for that family's own byte formula, at W = 16384:
  6 bytes a pixel (3->3 stencil, 2*3 flat / conv / blur, colour matrix): rows 2389 | 2390
  4 bytes a pixel (3->1 gray pass or gray-prologue stencil, 1->3 expand):  rows 3584 | 3585
  2 bytes a pixel (1-channel flat / conv / blur):                         rows 7168 | 7169
A 3->1 pass has cin + cout = 4 but 2 * cmid = 2, so a family that took the
other family's formula fails its row pair."""
import json
import os
import subprocess
import sys

import pytest

MIN = 224 << 20
W = 16384
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STENCIL = ("sep", "sobel_rp", "direct", "rank")

# (family, cin, cout, cmid, gray_prologue, lut_stage, rows at/below, rows above)
CASES = [
    ("sep", 3, 3, 3, False, False, 2389, 2390),
    ("sep", 1, 1, 1, False, False, 7168, 7169),
    ("sep", 3, 1, 1, True, False, 3584, 3585),       # gray prologue: 3 + 1 bytes a pixel
    ("sobel_rp", 1, 1, 1, False, False, 7168, 7169),
    ("direct", 3, 3, 3, False, False, 2389, 2390),
    ("direct", 3, 1, 1, True, False, 3584, 3585),
    ("direct", 3, 3, 1, True, False, 2389, 2390),    # gray prologue + expand epilogue
    ("rank", 3, 3, 3, False, False, 2389, 2390),
    ("rank", 3, 1, 1, True, False, 3584, 3585),
    ("conv_small", 3, 3, 3, False, False, 2389, 2390),
    ("conv_small", 1, 1, 1, False, False, 7168, 7169),
    ("pointwise", 3, 1, 1, True, False, 3584, 3585),  # gray
    ("pointwise", 3, 3, 1, True, False, 2389, 2390),  # gray,expand
    ("pointwise", 1, 3, 1, False, False, 3584, 3585),  # expand
    ("pointwise_flat", 3, 3, 3, False, False, 2389, 2390),
    ("pointwise_flat", 1, 1, 1, False, False, 7168, 7169),
    ("colormix", 3, 3, 3, False, False, 2389, 2390),
    ("colormix", 3, 3, 3, False, True, 2389, 2390),
    ("blur", 3, 3, 3, False, False, 2389, 2390),
    ("blur", 1, 1, 1, False, False, 7168, 7169),
]


def expected(fam, cin, cout, cmid, gray, lut, rows, nt, wgs, env, nt_wgs=-1, pw_wgs=None, xcd=-1):
    """The table, row by row.  env: STRIPE_NT (None | 0 | 1); nt_wgs / pw_wgs /
    xcd: the cached knobs (unset: -1 / None / -1)."""
    px = rows * W
    if fam in STENCIL:
        n = (nt != 0) if nt >= 0 else px * (cin + cout) > MIN
        if env is not None:
            n = env == 1  # overrides both ways
        default = 2 if fam in ("sep", "sobel_rp") else (0 if gray else 3)
        if n and nt_wgs >= 0:
            cap = nt_wgs
        elif wgs >= 0:
            cap = wgs
        else:
            cap = default if n else 0
        nxcd = xcd if xcd >= 0 else (0 if n else 8)
        return dict(nt_stores=n, streaming=n, nxcd=nxcd, cap=cap, cap_applied=cap > 0)
    if fam == "conv_small":
        n = px * 2 * cmid > MIN  # PassLaunch::nt ignored
        if env is not None:
            n = env == 1
        return dict(nt_stores=n, streaming=n, nxcd=xcd if xcd >= 0 else 0, cap=0, cap_applied=False)
    if fam == "pointwise":
        big = px * (cin + cout) > MIN
        n = cout == 1 and big
        if env is not None:
            n = env == 1  # also for cout == 3
        return dict(nt_stores=n, streaming=big, nxcd=0, cap=0, cap_applied=False)  # STRIPE_PWG_WGS: off
    if fam == "pointwise_flat":
        big = px * 2 * cin > MIN
        n = big and env != 0  # =0 turns it off, =1 cannot turn it on
        cap = 3 if pw_wgs is None else pw_wgs
        return dict(nt_stores=n, streaming=big, nxcd=0, cap=cap, cap_applied=cap > 0 and n)
    if fam == "colormix":
        big = px * 6 > MIN
        n = big
        if env is not None:
            n = env == 1
        cap = pw_wgs if pw_wgs is not None and pw_wgs >= 0 else (6 if lut else 3)
        return dict(nt_stores=n, streaming=big, nxcd=0, cap=cap, cap_applied=cap > 0 and big and n)
    assert fam == "blur"
    st = (nt != 0) if nt >= 0 else px * 2 * cmid > MIN  # STRIPE_NT not read
    return dict(nt_stores=False, streaming=st, nxcd=xcd if xcd >= 0 else (0 if st else 8), cap=0, cap_applied=False)


def test_case_rows_straddle_the_threshold():
    """The row pairs above sit at/below and above 224 MiB for their family's formula."""
    for fam, cin, cout, cmid, gray, lut, lo, hi in CASES:
        per_px = (cin + cout) if fam in STENCIL or fam == "pointwise" else 6 if fam == "colormix" else (
            2 * cin if fam == "pointwise_flat" else 2 * cmid)
        assert lo * W * per_px <= MIN < hi * W * per_px, (fam, cin, cout)
        assert hi == lo + 1


@pytest.mark.parametrize("env", [None, "0", "1"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d%d%d%s%s" % (c[0], c[1], c[2], c[3], "g" * c[4], "l" * c[5]))
def test_table(C, monkeypatch, case, env):
    fam, cin, cout, cmid, gray, lut, lo, hi = case
    if env is None:
        monkeypatch.delenv("STRIPE_NT", raising=False)
    else:
        monkeypatch.setenv("STRIPE_NT", env)  # live: read at every launch
    for k in ("STRIPE_NT_WGS", "STRIPE_PW_WGS", "STRIPE_PWG_WGS", "STRIPE_XCD"):
        assert k not in os.environ, k + " is cached per process and tested in test_cached_knobs: unset it"
    for rows in (lo, hi):
        for nt in (-1, 0, 1):
            for wgs in (-1, 0, 4):
                got = C.launch_policy(fam, cin, cout, cmid, W, rows, nt, wgs, gray, lut)
                want = expected(fam, cin, cout, cmid, gray, lut, rows, nt, wgs, None if env is None else int(env))
                assert got == want, (case, rows, nt, wgs, env)


def test_spot_values(C, monkeypatch):
    """A few cells as literals, so the table above cannot drift together with `expected`."""
    monkeypatch.delenv("STRIPE_NT", raising=False)
    lp = C.launch_policy
    # headline gaussian5 on 16384^2 RGB: nt stores, linear order, 2 workgroups per CU
    assert lp("sep", 3, 3, 3, W, 16384) == dict(nt_stores=True, streaming=True, nxcd=0, cap=2, cap_applied=True)
    # one N=8 share of it: cache-resident, XCD remap, no cap
    assert lp("sep", 3, 3, 3, W, 2048) == dict(nt_stores=False, streaming=False, nxcd=8, cap=0, cap_applied=False)
    # ... unless the engine says the stripe is cold, or picks a cap
    assert lp("sep", 3, 3, 3, W, 2048, nt=1)["cap"] == 2
    assert lp("sep", 3, 3, 3, W, 2048, nt=0, wgs=4) == dict(nt_stores=False, streaming=False, nxcd=8, cap=4,
                                                           cap_applied=True)
    assert lp("direct", 3, 1, 1, W, 16384, gray_prologue=True)["cap"] == 0
    assert lp("rank", 3, 3, 3, W, 16384)["cap"] == 3
    # 3->1 gray: nt stores; gray,expand (3->3): default stores though it streams
    assert lp("pointwise", 3, 1, 1, W, 16384, gray_prologue=True)["nt_stores"] is True
    assert lp("pointwise", 3, 3, 1, W, 16384, gray_prologue=True) == dict(nt_stores=False, streaming=True, nxcd=0,
                                                                         cap=0, cap_applied=False)
    assert lp("colormix", 3, 3, 3, W, 16384, lut_stage=True)["cap"] == 6
    monkeypatch.setenv("STRIPE_NT", "1")
    assert lp("pointwise_flat", 3, 3, 3, W, 100)["nt_stores"] is False  # cannot be turned on
    assert lp("pointwise", 3, 3, 1, W, 100, gray_prologue=True)["nt_stores"] is True  # forced onto 3-channel output
    assert lp("colormix", 3, 3, 3, W, 100) == dict(nt_stores=True, streaming=False, nxcd=0, cap=3, cap_applied=False)
    assert lp("blur", 3, 3, 3, W, 100)["streaming"] is False  # not read
    assert lp("sep", 3, 3, 3, W, 100, nt=0) == dict(nt_stores=True, streaming=True, nxcd=0, cap=2, cap_applied=True)
    monkeypatch.setenv("STRIPE_NT", "0")
    assert lp("pointwise_flat", 3, 3, 3, W, 16384) == dict(nt_stores=False, streaming=True, nxcd=0, cap=3,
                                                          cap_applied=False)
    assert lp("conv_small", 3, 3, 3, W, 16384, nt=1)["nt_stores"] is False
    with pytest.raises(Exception):
        lp("no_such_family", 3, 3, 3, W, 1)


def test_lds_reserve_bytes(C):
    f = C.lds_reserve_bytes
    assert f(163840, 512, 3) == 163840 // 4 + 1024 - 512 == 41472  # k_pointwise_flat at 3 per CU
    assert f(163840, 12800, 6) == 163840 // 7 + 1024 - 12800 == 11629  # k_colormix at 6
    assert f(163840, 768, 2) == 163840 // 3 + 1024 - 768 == 54869  # k_sep at 2
    assert f(163840, 512, 0) == 0 and f(163840, 512, -1) == 0
    assert f(163840, 100000, 3) == 0  # static LDS beyond the share: 0, not a wrapped size_t
    assert f(65536, 12800, 6) == 0


# ---- cached knobs: read once per process, so each value gets a fresh one ----
CHILD = r"""
import json, sys
import mpi_cuda_imagemanipulation_amd as m
print("RESULT " + json.dumps([m._C.launch_policy(*q) for q in json.loads(sys.argv[1])]))
"""
QUERIES = [(c[0], c[1], c[2], c[3], W, rows, nt, wgs, c[4], c[5])
           for c in CASES for rows in (c[6], c[7]) for nt, wgs in ((-1, -1), (1, 4), (0, 0))]
KNOBS = {
    "STRIPE_NT_WGS=1": dict(nt_wgs=1),
    "STRIPE_PW_WGS=0": dict(pw_wgs=0),
    "STRIPE_PW_WGS=5": dict(pw_wgs=5),
    "STRIPE_XCD=0": dict(xcd=0),
}


@pytest.fixture(scope="module")
def knob_runs():
    """One child per knob setting, started together."""
    procs = {}
    for setting in KNOBS:
        env = {k: v for k, v in os.environ.items() if not k.startswith("STRIPE_")}
        name, value = setting.split("=")
        env[name] = value
        procs[setting] = subprocess.Popen([sys.executable, "-c", CHILD, json.dumps(QUERIES)], cwd=ROOT, env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for setting, p in procs.items():
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, (setting, se[-2000:])
        out[setting] = json.loads([l for l in so.splitlines() if l.startswith("RESULT ")][-1][7:])
    return out


@pytest.mark.parametrize("setting", list(KNOBS))
def test_cached_knobs(knob_runs, setting):
    got = knob_runs[setting]
    assert len(got) == len(QUERIES)
    moved = 0
    for q, g in zip(QUERIES, got):
        fam, cin, cout, cmid, _, rows, nt, wgs, gray, lut = q
        assert g == expected(fam, cin, cout, cmid, gray, lut, rows, nt, wgs, None, **KNOBS[setting]), (setting, q)
        moved += g != expected(fam, cin, cout, cmid, gray, lut, rows, nt, wgs, None)
    assert moved > 0, setting + " changed no decision"
