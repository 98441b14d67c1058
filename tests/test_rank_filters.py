"""Rank filters on the CPU: median3/5, erode3/5, dilate3/5 and the open / close
sugar.  Spec (parser, plan), the golden path against scipy.ndimage, the host
executor against the golden path, the median networks themselves, and the
distributed host backend."""
import itertools
import json
import os
import re

import numpy as np
import pytest

try:
    import scipy.ndimage as ndi
except ImportError:  # only the scipy comparison needs it
    ndi = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "build", "kernel_resources.json")

NAMES = ["median3", "median5", "erode3", "erode5", "dilate3", "dilate5"]
BORDERS = ("reflect101", "replicate", "constant")
SCIPY_MODE = {"reflect101": "mirror", "replicate": "nearest", "constant": "constant"}
SCIPY_FN = {"median": "median_filter", "erode": "minimum_filter", "dilate": "maximum_filter"}
TIES = np.array([0, 1, 2, 253, 254, 255], np.uint8)
CHAINS = ["gray:ref,contrast:3.5,median3,expand", "median3,threshold:128,open3", "gaussian5,dilate5@constant,invert",
          "erode3@skip,median5"]
DIRECT = 2  # PassKind::Direct


@pytest.fixture(scope="module")
def m():
    import mpi_cuda_imagemanipulation_amd as m

    return m


def _full(shape, C):
    return shape + (3,) if C == 3 else shape


def _scipy(img, name, border):
    fam, K = name[:-1], int(name[-1])
    size = (K, K) if img.ndim == 2 else (K, K, 1)
    return getattr(ndi, SCIPY_FN[fam])(img, size=size, mode=SCIPY_MODE[border], cval=0)


# ---- parsing ------------------------------------------------------------------------
def test_spellings_and_aliases(C):
    for n in NAMES:
        assert C.parse_chain(n) == n
    assert C.parse_chain("median,erode,dilate") == "median3,erode3,dilate3"
    assert C.parse_chain("median5@skip") == "median5@skip"


def test_open_close_expand(C):
    assert C.parse_chain("open3@replicate") == "erode3@replicate,dilate3@replicate"
    assert C.parse_chain("open5") == "erode5,dilate5"
    assert C.parse_chain("close3") == "dilate3,erode3"
    assert C.parse_chain("gray,close5@constant,invert") == "gray:bt601,dilate5@constant,erode5@constant,invert"


@pytest.mark.parametrize("bad", ["median4", "erode7", "open", "close", "dilate1", "open7", "median3:2"])
def test_bad_sizes_rejected(C, bad):
    with pytest.raises(Exception) as ei:
        C.parse_chain(bad)
    if ":" in bad:
        assert "takes no arguments" in str(ei.value)
    else:
        assert "3" in str(ei.value) and "5" in str(ei.value) and "size" in str(ei.value)


def test_unknown_filter_message_lists_rank_names(C):
    with pytest.raises(Exception) as ei:
        C.parse_chain("nosuchfilter")
    # the message is assembled from the catalogue's syntax strings (ops.FILTERS keys)
    for word in ("median3 / median5", "erode3 / erode5", "dilate3 / dilate5", "open3 / open5", "close3 / close5"):
        assert word in str(ei.value)


def test_stencil_weights_rank_key(C):
    want = {"median": "median", "erode": "min", "dilate": "max"}
    for n in NAMES:
        d = C.stencil_weights(n)
        assert d["rank"] == want[n[:-1]] and d["K"] == int(n[-1])
        assert d["w"] == [] and d["div"] == 1 and not d["separable"] and not d["sobel"]
    assert C.stencil_weights("emboss3")["rank"] == "none"
    assert C.stencil_weights("gaussian5")["rank"] == "none"


def test_filters_listed_and_helpers_exported(m):
    text = " ".join(m.ops.FILTERS)
    for word in ("median3", "erode3", "dilate5", "open3", "close3"):
        assert word in text
    for fn in ("median", "erode", "dilate", "morph_open", "morph_close"):
        assert fn in m.ops.__all__ and callable(getattr(m.ops, fn))


# ---- plan ---------------------------------------------------------------------------
def test_plan_fused_pipeline_is_one_direct_pass(C):
    info = C.plan_info("gray:ref,contrast:3.5,median3,expand", 3)
    assert len(info["passes"]) == 1
    p = info["passes"][0]
    assert p["kind"] == DIRECT and p["R"] == 1 and p["epi_expand"]
    assert p["cin"] == 3 and p["cmid"] == 1 and p["cout"] == 3
    assert p["desc"].startswith("rank median3 ")


def test_plan_margins(C):
    info = C.plan_info("median5,median5", 3)
    assert info["in_margin_px"] == 2
    assert [p["out_margin_px"] for p in info["passes"]] == [2, 2]  # the cyclic contract of an iterated chain
    info = C.plan_info("close5", 3)
    assert len(info["passes"]) == 2 and info["max_radius"] == 2
    assert all(p["kind"] == DIRECT for p in info["passes"])
    assert C.plan_info("erode3,invert", 3)["passes"][0]["epi_lut"]


# ---- the median networks (rank_net.h) -----------------------------------------------
@pytest.mark.parametrize("K", [3, 5])
def test_median_networks_zero_one_principle(C, K):
    """A compare-exchange network selects the median of every input iff it does
    on every 0-1 input; with sorted columns those are the (K + 1)^K inputs
    where column c holds k_c ones at its top ranks."""
    net = C.rank_network(K)
    # the column sorter on all 2^K 0-1 columns
    cols = np.array(list(itertools.product((0, 1), repeat=K)), np.uint8).T.copy()  # wire x input
    for i, j, mode in net["colsort"]:
        assert mode == 0 and 0 <= i < j < K
        lo, hi = np.minimum(cols[i], cols[j]), np.maximum(cols[i], cols[j])
        cols[i], cols[j] = lo, hi
    assert (np.diff(cols.astype(int), axis=0) >= 0).all()
    # the selection network on all sorted-column 0-1 windows
    ks = np.array(list(itertools.product(range(K + 1), repeat=K)))  # input x column: ones per column
    w = np.zeros((K * K, len(ks)), np.uint8)
    for dx in range(K):
        for r in range(K):
            w[dx * K + r] = ks[:, dx] >= K - r
    want = ks.sum(axis=1) >= K * K - K * K // 2  # element K*K/2 (ascending) is a one
    for i, j, mode in net["select"]:
        assert 0 <= i < j < K * K and mode in (0, 1, 2)
        lo, hi = np.minimum(w[i], w[j]), np.maximum(w[i], w[j])
        if mode != 2:
            w[i] = lo
        if mode != 1:
            w[j] = hi
    assert (w[net["out"]] == want).all()


# ---- golden path vs scipy -----------------------------------------------------------
@pytest.mark.skipif(ndi is None, reason="scipy.ndimage not installed")
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (2, 7), (17, 15), (64, 65)])
@pytest.mark.parametrize("Cn", [1, 3])
def test_golden_matches_scipy(C, rng, name, shape, Cn):
    imgs = [rng.integers(0, 256, size=_full(shape, Cn), dtype=np.uint8),
            rng.choice(TIES, size=_full(shape, Cn)),  # equal keys and the byte extremes
            np.full(_full(shape, Cn), 200, np.uint8)]
    for img in imgs:
        for border in BORDERS:
            got = C.golden_apply(img, name, border, True)
            assert (got == _scipy(img, name, border)).all(), (name, shape, Cn, border)


def _skip_mirror(img, name):
    """@skip: pixels with x <= R, y <= R, x >= W - R or y >= H - R keep their
    value; the others take the rank of their (fully interior) window."""
    K = int(name[-1])
    R = K // 2
    H, W = img.shape[:2]
    out = img.copy()
    red = {"median": lambda a: np.sort(a, axis=0)[K * K // 2], "erode": lambda a: a.min(axis=0),
           "dilate": lambda a: a.max(axis=0)}[name[:-1]]
    for y in range(R + 1, H - R):
        for x in range(R + 1, W - R):
            win = img[y - R:y + R + 1, x - R:x + R + 1].reshape(K * K, -1)
            out[y, x] = red(win).reshape(out[y, x].shape)
    return out


@pytest.mark.parametrize("name", ["median3", "median5", "erode5", "dilate3"])
@pytest.mark.parametrize("shape,Cn", [((45, 77), 1), ((20, 31), 3)])
def test_skip_border(C, m, rng, name, shape, Cn):
    img = rng.integers(0, 256, size=_full(shape, Cn), dtype=np.uint8)
    want = _skip_mirror(img, name)
    assert (C.golden_apply(img, name + "@skip", "reflect101", True) == want).all()
    assert (m.ops.apply(img, name + "@skip") == want).all()


# ---- host executor vs golden --------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (37, 130), (64, 1000)])
@pytest.mark.parametrize("Cn", [1, 3])
def test_host_executor_matches_golden(C, m, rng, name, shape, Cn):
    for img in (rng.integers(0, 256, size=_full(shape, Cn), dtype=np.uint8), rng.choice(TIES, size=_full(shape, Cn))):
        for border in BORDERS:
            assert (m.ops.apply(img, name, border) == C.golden_apply(img, name, border, True)).all(), (name, border)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("shape", [(5, 3), (37, 130), (64, 1000)])
def test_host_executor_chains(C, m, rng, chain, shape):
    img = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    assert (m.ops.apply(img, chain) == C.golden_apply(img, chain, "reflect101", True)).all()


# ---- properties ---------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 3])
def test_morphology_properties(m, rng, Cn):
    x = rng.integers(0, 256, size=_full((41, 53), Cn), dtype=np.uint8)
    ops = m.ops
    er, di = ops.erode(x, 3, "replicate"), ops.dilate(x, 3, "replicate")
    assert (er <= x).all() and (x <= di).all()
    op = ops.morph_open(x, 3, "replicate")
    assert (ops.morph_open(op, 3, "replicate") == op).all()
    cl = ops.morph_close(x, 3, "replicate")
    assert (ops.morph_close(cl, 3, "replicate") == cl).all()
    flat = np.full_like(x, 77)
    assert (ops.median(flat, 3) == flat).all() and (ops.median(flat, 5) == flat).all()
    assert (di == 255 - ops.erode(255 - x, 3, "replicate")).all()
    assert (di == ops.apply(x, "invert,erode3,invert", "replicate")).all()
    assert (ops.apply(x, "open3") == ops.apply(x, "erode3,dilate3")).all()


# ---- distributed, host backend ------------------------------------------------------
@pytest.mark.parametrize("chain,iters", [("median5", 1), ("close3", 1), ("erode3", 4)])
@pytest.mark.parametrize("ranks", [3, 8])
def test_distributed_host_matches_one_rank(C, m, chain, iters, ranks):
    """Row stripes of an 83-row frame (no multiple of 3 or 8) stitched from N
    ranks equal the 1-rank result; the iterated erode3 runs the deep halo."""
    W, H = 61, 83
    img = m.utils.synthetic_image(21, W, H, 3)
    one = C.run_local_group(m.Pipeline(chain).config(W, H, 3, "host"), 1, img, iters)
    many = C.run_local_group(m.Pipeline(chain).config(W, H, 3, "host"), ranks, img, iters)
    assert (many == one).all()
    ref = img
    for _ in range(iters):
        ref = C.golden_apply(ref, chain, "reflect101", True)
    assert (one == ref).all()


# ---- compiled kernels (needs the build's resource report) ---------------------------
@pytest.fixture(scope="module")
def report():
    if not os.path.exists(REPORT):
        pytest.skip("build/kernel_resources.json missing (run python tools/build.py)")
    with open(REPORT) as f:
        return json.load(f)


def _window(kernel_name):
    return int(re.search(r"4sdef\d+[A-Za-z]+?(\d)E", kernel_name).group(1))


def test_rank_kernel_resources(report):
    rank = {k: v for k, v in report.items() if "k_rank" in k}
    assert rank, "no k_rank family in the resource report"
    assert not {k: v["SGPRs Spill"] for k, v in rank.items() if v.get("SGPRs Spill", 0) != 0}
    direct3 = [v["Occupancy [waves/SIMD]"] for k, v in report.items()
               if "k_direct" in k and re.search(r"4sdef\d+(Emboss3|Sharpen|Laplace)E", k)]
    assert direct3
    for k, v in rank.items():
        occ = v["Occupancy [waves/SIMD]"]
        if _window(k) == 3:
            assert occ >= min(direct3), (k, occ)
        else:
            assert _window(k) == 5 and occ >= 2, (k, occ)
