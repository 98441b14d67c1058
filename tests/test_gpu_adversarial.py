"""HIP kernels vs the golden path on saturated and structured frames
(tests/patterns.py), bit-exact: the integer stencils and rank filters, their
fused prologue / epilogue forms, the small float conv, constant borders behind
a pointwise run that moves the zero pixel, and the pointwise kernels at row
lengths past one workgroup."""
import numpy as np
import pytest

import patterns

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STENCILS = ["gaussian3", "gaussian5", "gaussian7", "box3", "box5", "emboss3", "emboss5", "sharpen", "laplace",
            "sobel", "sobel_l2"]
RANKS = ["median3", "median5", "erode3", "erode5", "dilate3", "dilate5"]
BORDERS = ("reflect101", "replicate", "constant")
POINTWISE = 0  # PassKind::Pointwise
# the post maps of test_gray_ref_post_affine_matches_golden (affine and table forms)
POST = ["contrast:3.5", "contrast:0.25,invert", "brightness:-17", "contrast:1.7", "threshold:100"]
PROLOGUES = ["invert", "brightness:40", "threshold:0", "gray,invert", "gray:ref,brightness:25"]
FAMILIES = ["gaussian5", "box5", "sobel", "emboss3", "median3", "erode3"]


@pytest.fixture(scope="module")
def m():
    import mpi_cuda_imagemanipulation_amd as m

    assert torch.cuda.is_available()
    return m


def _run_frames(m, frames, chain, border):
    """ops.apply on a stack of equally shaped frames (one engine, frame by frame)."""
    x = np.stack(frames)
    if x.ndim == 3:
        x = x[..., None]
    y = m.ops.apply(torch.from_numpy(np.ascontiguousarray(x)).cuda(), chain, border)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _check(m, labelled, chain, border, ref_fn=None):
    got = _run_frames(m, [im for _, im in labelled], chain, border)
    for (label, img), g in zip(labelled, got):
        ref = ref_fn(img) if ref_fn else m._C.golden_apply(img, chain, border, True)
        assert g.shape == ref.shape, (chain, border, label, g.shape, ref.shape)
        bad = np.argwhere(g != ref)
        assert bad.size == 0, (f"{chain} {border} {label} {img.shape}: {len(bad)} mismatches, first {bad[:5].tolist()}, "
                               f"got {g[tuple(bad[0])]} want {ref[tuple(bad[0])]}")


def _full(shape, C):
    return tuple(shape) + ((3,) if C == 3 else ())


# ---- every stencil and rank filter on every pattern ---------------------------------
@pytest.mark.parametrize("name", STENCILS + RANKS)
@pytest.mark.parametrize("C", [1, 3])
def test_stencil_patterns_exact(m, name, C):
    for shape in patterns.shapes(C):
        labelled = list(patterns.patterns(*shape, C))
        for border in BORDERS:
            _check(m, labelled, name, border)


# ---- fused forms: gray / gray:ref prologues with affine and table post maps ---------
# RGB frames whose gray rows straddle the 992- and 1024-byte seams
GRAY_SHAPES = [(1, 1), (3, 2), (5, 70), (2, 993), (13, 1025)]


@pytest.mark.parametrize("F", STENCILS + RANKS)
def test_fused_prologue_forms(m, F):
    chains = [(f"gray,{F},expand", BORDERS), (f"gray:ref,contrast:3.5,{F}@skip,expand", ("reflect101",))]
    chains += [(f"gray:ref,{pw},{F}", BORDERS) for pw in POST]
    for chain, borders in chains:
        for border in borders:
            if border != "constant":  # under constant a zero-moving post map is a pass of its own
                assert len(m._C.plan_info(chain, 3, border)["passes"]) == 1, (chain, border)
        for shape in GRAY_SHAPES:
            labelled = patterns.saturated(*shape, 3)
            for border in borders:
                _check(m, labelled, chain, border)


@pytest.mark.parametrize("F", STENCILS + RANKS)
@pytest.mark.parametrize("C", [1, 3])
def test_fused_epilogue_lut(m, F, C):
    chain = f"{F},invert"
    assert m._C.plan_info(chain, C)["passes"][0]["epi_lut"]
    for shape in [(1, 1), (3, 2), (5, 70), (2, patterns.WIDTHS[C][0]), (13, patterns.WIDTHS[C][-2])]:
        labelled = patterns.saturated(*shape, C)
        for border in BORDERS:
            _check(m, labelled, chain, border)


@pytest.mark.parametrize("F", ["gaussian5", "emboss5", "sobel", "median3"])
@pytest.mark.parametrize("C", [1, 3])
def test_skip_border_patterns(m, F, C):
    for shape in [(1, 1), (3, 2), (5, 70), (2, patterns.WIDTHS[C][0]), (13, patterns.WIDTHS[C][-2])]:
        _check(m, patterns.saturated(*shape, C), f"{F}@skip", "reflect101")


# ---- small float conv (k_conv_small) with integer weights ---------------------------
def _int_weights(K, kind):
    n = K * K
    if kind == "ones":  # one sign, saturated f32 sums
        return np.ones((K, K))
    if kind == "neg":
        return -np.ones((K, K))
    if kind == "shift":  # one sign, one tap: a mirrored or transposed window shows
        w = np.zeros((K, K))
        w[0, K - 1] = 1
        return w
    w = (np.arange(n, dtype=np.float64) - n // 2).reshape(K, K)  # mixed sign, asymmetric, sum 1
    w[K // 2, K // 2] = 1
    return w


@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("kind", ["ones", "neg", "shift", "mixed"])
@pytest.mark.parametrize("C", [1, 3])
def test_small_conv_integer_weights(m, K, kind, C):
    """Integer weights on bytes: every sum is an integer below 2^24, exact in
    f32 in any order and never at a rounding tie, so the comparison is exact."""
    w = _int_weights(K, kind)
    spec = f"conv:{K}:" + ";".join(repr(float(v)) for v in w.reshape(-1))
    assert "(direct)" in m._C.plan_info(spec, C)["passes"][0]["desc"]
    for shape in [(1, 1), (3, 2), (5, 70), (13, patterns.WIDTHS[C][0])]:
        labelled = [(l, im) for l, im in patterns.patterns(*shape, C) if l.startswith(("uniform255", "checker"))]
        for border in BORDERS:
            _check(m, labelled, spec, border, ref_fn=lambda img: m.ops.conv2d(img, w, border))


# ---- constant border behind a prologue that moves the zero pixel --------------------
@pytest.mark.parametrize("F", FAMILIES)
@pytest.mark.parametrize("pro", PROLOGUES)
def test_constant_border_after_prologue(m, rng, pro, F):
    """The border is zero after the pointwise run: `invert,gaussian5` sees 0
    outside the frame, not invert(0) = 255.  The all-0 frame makes a cooked
    margin stand out most."""
    for shape in ((5, 70, 3), (13, 331, 3)):
        labelled = [("random", rng.integers(0, 256, size=shape, dtype=np.uint8)), ("zeros", np.zeros(shape, np.uint8))]
        _check(m, labelled, f"{pro},{F}", "constant")
        _check(m, labelled, f"{pro},{F}@constant", "reflect101")


@pytest.mark.parametrize("chain,iters", [("invert,gaussian5", 1), ("invert,gaussian5", 3), ("brightness:40,median3", 2),
                                         ("gray:ref,brightness:25,emboss3", 1)])
def test_constant_border_chains_local_ranks(m, chain, iters):
    """3 logical ranks on one GPU: the pointwise pass zeroes the frame's
    x-margins only, halo rows between stripes carry its pixels."""
    W, H = 61, 83
    img = m.utils.synthetic_image(21, W, H, 3)
    ref = img
    for _ in range(iters):
        ref = m._C.golden_apply(ref, chain, "constant", True)
    for ranks in (3, 1):
        cfg = m.Pipeline(chain, "constant").config(W, H, 3, "device", device=0)
        got = m._C.run_local_group(cfg, ranks, img, iters)
        bad = np.argwhere(got != ref)
        assert got.shape == ref.shape and bad.size == 0, (chain, iters, ranks, len(bad), bad[:5].tolist())


# ---- pointwise kernels --------------------------------------------------------------
# k_pointwise_flat: 4 groups of 16 B per lane, 256 lanes apart, 16 KiB of a row per
# workgroup; rows of 4095 .. 16400 B reach the 2nd to 4th group and a 2nd workgroup
FLAT_WIDTHS = {1: (4095, 4097, 16383, 16385, 16400), 3: (1365, 1366, 5461, 5462, 5467)}


def _pw_images(rng, full):
    return [("random", rng.integers(0, 256, size=full, dtype=np.uint8)), ("all255", np.full(full, 255, np.uint8)),
            ("extremes", rng.choice(patterns.EXTREMES, size=full))]


@pytest.mark.parametrize("chain", ["invert", "brightness:-40", "contrast:3.5", "threshold:77"])
@pytest.mark.parametrize("C", [1, 3])
def test_pointwise_lut_rows(m, rng, chain, C):
    assert [p["kind"] for p in m._C.plan_info(chain, C)["passes"]] == [POINTWISE]
    for shape in [(1, 1), (3, 2)] + [(3, w) for w in FLAT_WIDTHS[C]]:
        labelled = _pw_images(rng, _full(shape, C))
        for border in BORDERS:
            _check(m, labelled, chain, border)


@pytest.mark.parametrize("chain", ["gray", "gray:ref", "gray,expand", "invert,gray,contrast:3.5,expand"])
def test_pointwise_channel_changing_rows(m, rng, chain):
    # k_pointwise: 16 px per lane, 4096 px per workgroup
    assert [p["kind"] for p in m._C.plan_info(chain, 3)["passes"]] == [POINTWISE]
    for shape in [(1, 1), (3, 2), (3, 4095), (3, 4097), (3, 4112)]:
        labelled = _pw_images(rng, _full(shape, 3))
        for border in BORDERS:
            _check(m, labelled, chain, border)


@pytest.mark.parametrize("chain,C,widths,borders", [
    ("invert,gray,gaussian5", 3, (4095, 4097, 4112), BORDERS),
    ("gray,expand,box3", 3, (4095, 4097, 4112), BORDERS),
    ("invert,gaussian5@constant", 1, (4095, 4097, 16385), ("reflect101",)),
    ("invert,gaussian5@constant", 3, (1365, 1366, 5462), ("reflect101",)),
])
def test_pointwise_pass_feeds_stencil(m, rng, chain, C, widths, borders):
    """The stencil reads the right margin that the pointwise pass wrote at these row lengths."""
    for border in borders:
        kinds = [p["kind"] for p in m._C.plan_info(chain, C, border)["passes"]]
        assert kinds[0] == POINTWISE and len(kinds) == 2 and kinds[1] != POINTWISE, (chain, border, kinds)
    for w in widths:
        labelled = _pw_images(rng, _full((3, w), C)) + [("zeros", np.zeros(_full((3, w), C), np.uint8))]
        for border in borders:
            _check(m, labelled, chain, border)
