"""Cross-channel colour filters (colormatrix, sepia, saturation, swaprb, ycbcr):
parser, chain compiler, golden path, host executor and the distributed host
backend.  The numeric specification is
    out_c = sat_u8((sum_k q[c][k] p_k + qb[c] + 2048) >> 12),  q = rint(m * 4096)
and `color_cases.mirror` evaluates it independently of the extension."""
import json
import os

import numpy as np
import pytest

import color_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "build", "kernel_resources.json")
SHAPES = [(1, 1), (3, 2), (2, 7), (17, 15), (64, 65)]
HOST_SHAPES = [(1, 1), (5, 3), (37, 130), (64, 1000)]


@pytest.fixture(scope="module")
def m():
    import mpi_cuda_imagemanipulation_amd as m

    return m


# ---- parsing ------------------------------------------------------------------------
def test_canonical_spellings(C):
    assert C.parse_chain(" sepia ") == "sepia"
    assert C.parse_chain("swaprb") == "swaprb" and C.parse_chain("bgr") == "swaprb"
    assert C.parse_chain("saturation:1.5") == "saturation:1.5"
    assert C.parse_chain("saturate:0.50") == "saturation:0.5"
    assert C.parse_chain("saturation:2") == "saturation:2"
    assert C.parse_chain("ycbcr") == "ycbcr" and C.parse_chain("ycbcr:inv") == "ycbcr:inv"
    tok = "colormatrix:1;0;0;0;1;0;0;0;1:0;0.5;-3"
    assert C.parse_chain("  " + tok + " ") == tok  # as typed, trimmed
    assert C.parse_chain("invert, colormatrix:1;0;0;0;1;0;0;0;1 ,sepia") == "invert,colormatrix:1;0;0;0;1;0;0;0;1,sepia"


@pytest.mark.parametrize("bad,word", [
    ("colormatrix:1;0;0;0;1;0;0;0", "9 coefficients"),
    ("colormatrix:1;0;0;0;1;0;0;0;1;0", "9 coefficients"),
    ("colormatrix", "colormatrix"),
    ("colormatrix:1;0;0;0;1;0;0;0;1:1;2", "3 offsets"),
    ("colormatrix:1;0;0;0;1;0;0;0;1:1;2;3;4", "3 offsets"),
    ("colormatrix:8;0;0;0;1;0;0;0;1", "out of range"),
    ("colormatrix:1;0;0;0;-8;0;0;0;1", "out of range"),
    ("colormatrix:1;0;0;0;1;0;0;0;1:0;2048.5;0", "out of range"),
    ("colormatrix:1;0;0;0;1;0;0;0;1:0;0;-2049", "out of range"),
    ("colormatrix:1;x;0;0;1;0;0;0;1", "bad number"),
    ("colormatrix:1;0;0;0;1;0;0;0;1:0;;0", "bad number"),
    ("saturation:much", "bad number"),
    ("saturation:40", "out of range"),
    ("sepia:1", "no arguments"),
    ("swaprb:1", "no arguments"),
    ("bgr:x", "no arguments"),
    ("ycbcr:fwd", "ycbcr"),
])
def test_parse_errors_name_the_token(C, bad, word):
    with pytest.raises(Exception) as e:
        C.parse_chain(bad)
    assert word in str(e.value) and bad.split(":")[0] in str(e.value), str(e.value)


def test_unknown_filter_lists_the_new_names(C, m):
    with pytest.raises(Exception) as e:
        C.parse_chain("nosuchfilter")
    msg = str(e.value)
    for name in ("colormatrix", "sepia", "saturation", "swaprb", "ycbcr", "gray", "gaussian3/5/7", "median3 / median5"):
        assert name in msg, name
    text = " ".join(m.ops.FILTERS)
    for name in ("colormatrix", "sepia", "saturation", "swaprb", "ycbcr"):
        assert name in text, name
    for fn in ("color_matrix", "sepia", "saturation", "swap_rb", "rgb_to_ycbcr", "ycbcr_to_rgb"):
        assert fn in m.ops.__all__ and callable(getattr(m.ops, fn))


def test_quantisation(C):
    d = C.color_matrix("sepia")
    assert d["q"] == [[1610, 3150, 774], [1430, 2810, 688], [1114, 2187, 537]]
    assert d["b"] == [0, 0, 0] and d["shift"] == 12
    assert C.color_matrix("swaprb")["q"] == [[0, 0, 4096], [0, 4096, 0], [4096, 0, 0]]
    assert C.color_matrix("ycbcr")["b"] == [0, 128 * 4096, 128 * 4096]
    # ties to even: 0.5 / 4096 * 4096 = 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    t = C.color_matrix("colormatrix:0.0001220703125;0.0003662109375;0.0006103515625;0;0;0;0;0;0")
    assert t["q"][0] == [0, 2, 2]
    for name in cc.NAMES:
        token, (q, qb), _ = cc.CASES[name]
        d = C.color_matrix(token)
        assert d["q"] == q.tolist() and d["b"] == qb.tolist(), name


@pytest.mark.parametrize("s", [0, 0.5, 1, 1.5, 2])
def test_saturation_rows_sum_to_one(C, s):
    q = C.color_matrix(f"saturation:{s}")["q"]
    assert [sum(r) for r in q] == [4096] * 3
    assert q == cc.saturation_q(s).tolist()
    if s == 1:
        assert q == [[4096, 0, 0], [0, 4096, 0], [0, 0, 4096]]
    if s == 0:
        assert q[0] == q[1] == q[2]


def test_needs_three_channels(C):
    with pytest.raises(Exception) as e:
        C.plan_info("gray,sepia", 3)
    assert "3-channel" in str(e.value) and "expand" in str(e.value)
    with pytest.raises(Exception):
        C.plan_info("swaprb", 1)
    C.plan_info("gray,expand,sepia", 3)
    C.plan_info("expand,ycbcr", 1)


# ---- plan ---------------------------------------------------------------------------
def _kinds(info):
    return [p["kind"] for p in info["passes"]]


def test_plans(C):
    p = C.plan_info("invert,sepia,brightness:10", 3)
    assert _kinds(p) == [0] and "pointwise[lut,cmat,lut] 3->3ch" in p["passes"][0]["desc"]
    assert p["passes"][0]["cmat"]
    p = C.plan_info("sepia,gaussian5", 3)
    assert _kinds(p) == [0, 1] and p["passes"][0]["out_margin_px"] == 2
    assert _kinds(C.plan_info("gaussian5,sepia", 3)) == [1, 0]
    p = C.plan_info("sepia,gray,emboss3", 3)
    assert len(p["passes"]) == 2 and "prologue[gray" in p["passes"][1]["desc"]
    p = C.plan_info("saturation:1,gaussian5", 3)
    assert _kinds(p) == [1] and not p["passes"][0]["cmat"]
    assert _kinds(C.plan_info("sepia,sepia", 3)) == [0, 0]
    # a matrix after a pending expand, and gray after a pending matrix, start a new pass
    p = C.plan_info("gray,expand,sepia", 3)
    assert _kinds(p) == [0, 0] and "expand" in p["passes"][0]["desc"] and "cmat" in p["passes"][1]["desc"]
    p = C.plan_info("sepia,gray", 3)
    assert _kinds(p) == [0, 0] and p["cout"] == 1
    # never a stencil epilogue
    p = C.plan_info("gaussian5,sepia,invert", 3)
    assert _kinds(p) == [1, 0] and "epilogue" not in p["passes"][0]["desc"]
    assert "pointwise[cmat,lut]" in p["passes"][1]["desc"]
    # iterated: the trailing matrix pass carries the first stencil's margins
    assert p["passes"][1]["out_margin_px"] == 2


# ---- golden path --------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.NAMES)
def test_golden_equals_integer_mirror(C, rng, name):
    token, (q, qb), _ = cc.CASES[name]
    for shape in SHAPES:
        for img in cc.images(rng, shape):
            got = C.golden_apply(img, token, "reflect101", True)
            assert got.shape == img.shape
            assert (got == cc.mirror(img, q, qb)).all(), (name, shape)


@pytest.mark.parametrize("name", cc.NAMES)
def test_golden_against_float_oracle(C, rng, name):
    """0.5 rounding + 3 * 255 * 2^-13 coefficient quantisation + 2^-13 offset
    quantisation < 0.6; clipping is 1-Lipschitz."""
    token, _, (M, b) = cc.CASES[name]
    for img in cc.images(rng, (64, 65)):
        want = np.clip(np.einsum("ck,...k->...c", M, img.astype(np.float64)) + b, 0, 255)
        got = C.golden_apply(img, token, "reflect101", True).astype(np.float64)
        assert np.abs(got - want).max() <= 0.6, name


def test_float_oracle_random_matrices(C, rng):
    img = rng.integers(0, 256, size=(32, 33, 3), dtype=np.uint8)
    for _ in range(20):
        M = rng.uniform(-2, 2, size=(3, 3))
        b = rng.uniform(-100, 100, size=3)
        token = "colormatrix:" + ";".join(repr(float(v)) for v in M.reshape(-1)) + ":" + ";".join(
            repr(float(v)) for v in b)
        want = np.clip(np.einsum("ck,...k->...c", M, img.astype(np.float64)) + b, 0, 255)
        got = C.golden_apply(img, token, "reflect101", True).astype(np.float64)
        assert np.abs(got - want).max() <= 0.6


# ---- properties ---------------------------------------------------------------------
def test_properties(C, rng):
    img = rng.integers(0, 256, size=(17, 15, 3), dtype=np.uint8)
    g = lambda chain: C.golden_apply(img, chain, "reflect101", True)
    assert (g("colormatrix:1;0;0;0;1;0;0;0;1") == img).all()
    assert (g("swaprb") == img[..., ::-1]).all()
    assert (g("swaprb,swaprb") == img).all()
    assert (g("saturation:1") == img).all()
    s0 = g("saturation:0")
    assert (s0[..., 0] == s0[..., 1]).all() and (s0[..., 1] == s0[..., 2]).all()
    grey = np.repeat(rng.integers(0, 256, size=(9, 11, 1), dtype=np.uint8), 3, axis=2)
    for s in (0, 0.5, 1.5, 2, 3.25):
        assert (C.golden_apply(grey, f"saturation:{s}", "reflect101", True) == grey).all(), s


@pytest.mark.parametrize("chain", cc.CHAINS)
def test_fused_equals_unfused(C, rng, chain):
    for shape in [(17, 15), (64, 65)]:
        for img in cc.images(rng, shape):
            fused = C.golden_apply(img, chain, "reflect101", True)
            assert (fused == C.golden_apply(img, chain, "reflect101", False)).all()
            assert (fused == C.golden_apply_unfused(img, chain, "reflect101")).all()


def test_ops_wrappers(m, rng):
    ops, C = m.ops, m._C
    x = rng.integers(0, 256, size=(12, 19, 3), dtype=np.uint8)
    g = lambda chain: C.golden_apply(x, chain, "reflect101", True)
    assert (ops.sepia(x) == g("sepia")).all()
    assert (ops.swap_rb(x) == x[..., ::-1]).all()
    assert (ops.saturation(x, 1.5) == g("saturation:1.5")).all()
    assert (ops.rgb_to_ycbcr(x) == g("ycbcr")).all()
    assert (ops.ycbcr_to_rgb(x) == g("ycbcr:inv")).all()
    q, qb = cc.quantise(cc.MIXED, cc.MIXED_B)
    assert (ops.color_matrix(x, cc.MIXED, cc.MIXED_B) == cc.mirror(x, q, qb)).all()
    assert (ops.color_matrix(x, cc.SEPIA) == g("sepia")).all()
    with pytest.raises(ValueError):
        ops.color_matrix(x, np.eye(2))
    with pytest.raises(ValueError):
        ops.color_matrix(x, np.eye(3), [1, 2])
    # a YCbCr round trip stays within the two roundings
    rt = ops.ycbcr_to_rgb(ops.rgb_to_ycbcr(x)).astype(int)
    assert np.abs(rt - x.astype(int)).max() <= 2


# ---- host executor ------------------------------------------------------------------
@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_host_executor_equals_golden(C, rng, shape):
    chains = [cc.CASES[n][0] for n in cc.NAMES] + cc.CHAINS
    for img in cc.images(rng, shape):
        for chain in chains:
            want = C.golden_apply(img, chain, "reflect101", True)
            assert (C.cpu_apply(img, chain, "reflect101", True) == want).all(), (chain, shape)
            assert (C.cpu_apply(img, chain, "reflect101", False) == want).all(), (chain, shape)


# ---- distributed, host backend ------------------------------------------------------
@pytest.mark.parametrize("chain,iters", [("sepia,gaussian5", 3), ("swaprb", 1)])
@pytest.mark.parametrize("ranks", [3, 8])
def test_distributed_host_matches_one_rank(C, m, chain, iters, ranks):
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
def test_colormix_kernel_resources():
    if not os.path.exists(REPORT):
        pytest.skip("build/kernel_resources.json missing (run python tools/build.py)")
    with open(REPORT) as f:
        report = json.load(f)
    fam = {k: v for k, v in report.items() if "k_colormix" in k}
    assert len(fam) >= 2, "k_colormix (nt and default stores) missing from the report"
    for k, v in fam.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v.get("Dynamic Stack", "False") == "False", k
        assert v["Occupancy [waves/SIMD]"] >= 4 and v["VGPRs"] <= 128, (k, v)
