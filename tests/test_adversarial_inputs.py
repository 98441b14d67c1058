"""Host paths on saturated and structured frames (tests/patterns.py).

The golden path against the numpy mirror, the host executor against the golden
path, closed forms on uniform frames, and chains whose leading pointwise run
moves the zero pixel under a constant border: the border is zero AFTER that
run, so such a run is a pass of its own there (csrc/core/chain.cpp) and is
fused into the stencil's load path only under the other borders.
"""
import numpy as np
import pytest

import np_ref
import patterns

STENCILS = ["gaussian3", "gaussian5", "gaussian7", "box3", "box5", "emboss3", "emboss5", "sharpen", "laplace",
            "sobel", "sobel_l2"]
RANKS = ["median3", "median5", "erode3", "erode5", "dilate3", "dilate5"]
BORDERS = ("reflect101", "replicate", "constant")
POINTWISE = 0  # PassKind::Pointwise

# leading pointwise runs that do not keep the zero pixel at zero
PROLOGUES = ["invert", "brightness:40", "threshold:0", "gray,invert", "gray:ref,brightness:25"]
# one filter per kernel family: k_sep (binomial, box), k_sobel_rp, k_direct, k_rank (median, min)
FAMILIES = ["gaussian5", "box5", "sobel", "emboss3", "median3", "erode3"]


def _frames(C):
    for shape in patterns.host_shapes(C):
        for label, img in patterns.patterns(*shape, C):
            yield shape, label, img


def _first_bad(got, ref):
    bad = np.argwhere(got != ref)
    return f"{len(bad)} mismatches, first {bad[:5].tolist()}"


# ---- golden vs numpy mirror, host executor vs golden --------------------------------
@pytest.mark.parametrize("name", STENCILS)
@pytest.mark.parametrize("Cn", [1, 3])
def test_stencils_on_patterns(C, name, Cn):
    for shape, label, img in _frames(Cn):
        for border in BORDERS + ("skip",):
            chain = f"{name}@{border}"
            ref = C.golden_apply(img, chain, "reflect101", True)
            want = np_ref.stencil(img, name, border)
            assert ref.shape == want.shape and (ref == want).all(), \
                f"golden {chain} {label} {img.shape}: {_first_bad(ref, want)}"
            for threads in (1, 3):
                got = C.cpu_apply(img, chain, "reflect101", True, threads)
                assert got.shape == ref.shape and (got == ref).all(), \
                    f"cpu {chain} {label} {img.shape} threads={threads}: {_first_bad(got, ref)}"


@pytest.mark.parametrize("name", RANKS)
@pytest.mark.parametrize("Cn", [1, 3])
def test_rank_filters_on_patterns(C, name, Cn):
    for shape, label, img in _frames(Cn):
        for border in BORDERS + ("skip",):
            chain = f"{name}@{border}"
            ref = C.golden_apply(img, chain, "reflect101", True)
            if border != "skip":
                want = _np_rank(img, name, border)
                assert (ref == want).all(), f"golden {chain} {label} {img.shape}: {_first_bad(ref, want)}"
            for threads in (1, 3):
                got = C.cpu_apply(img, chain, "reflect101", True, threads)
                assert got.shape == ref.shape and (got == ref).all(), \
                    f"cpu {chain} {label} {img.shape} threads={threads}: {_first_bad(got, ref)}"


# ---- closed forms on uniform frames -------------------------------------------------
@pytest.mark.parametrize("name", STENCILS + RANKS)
@pytest.mark.parametrize("Cn", [1, 3])
def test_uniform_frames_closed_form(C, name, Cn):
    """Taps that sum to 1 after the division keep a uniform frame; derivative
    filters give 0.  Under reflect101 and replicate every window is uniform;
    under constant that holds R pixels from the edge."""
    R = C.stencil_weights(name)["K"] // 2
    zero = name in ("laplace", "sobel", "sobel_l2")
    for shape in ((13, 70), (7, 9), (1, 1), (2, 3)):
        for v in patterns.UNIFORM:
            img = np.full(shape + ((3,) if Cn == 3 else ()), v, np.uint8)
            want = 0 if zero else v
            for border in BORDERS:
                for out in (C.golden_apply(img, name, border, True), C.cpu_apply(img, name, border, True, 2)):
                    if border == "constant":
                        out = out[R:shape[0] - R, R:shape[1] - R]
                    assert (out == want).all(), (name, Cn, shape, v, border)


# ---- non-zero-preserving prologue under a constant border ---------------------------
def _np_rank(img, name, border):
    fam, K = name[:-1], int(name[-1])
    R = K // 2

    def one(ch):
        H, W = ch.shape
        p = np.pad(ch, R, mode={"reflect101": "reflect", "replicate": "edge", "constant": "constant"}[border])
        win = np.stack([p[dy:dy + H, dx:dx + W] for dy in range(K) for dx in range(K)])
        return {"median": lambda a: np.sort(a, axis=0)[K * K // 2], "erode": lambda a: a.min(axis=0),
                "dilate": lambda a: a.max(axis=0)}[fam](win)

    return one(img) if img.ndim == 2 else np.stack([one(img[..., c]) for c in range(3)], axis=-1)


def _np_chain(img, chain, border):
    """Composition of the numpy primitives, op by op; borders are applied to each stencil's own input."""
    x = img
    for op in chain.split(","):
        op, _, b = op.partition("@")
        name, _, arg = op.partition(":")
        if name == "gray":
            if x.ndim == 3:
                x = np_ref.gray_ref(x) if arg == "ref" else np_ref.gray_bt601(x)
        elif name == "invert":
            x = np_ref.invert(x)
        elif name == "brightness":
            x = np_ref.brightness(x, int(arg))
        elif name == "threshold":
            x = np.where(x >= int(arg), 255, 0).astype(np.uint8)
        elif name in RANKS:
            x = _np_rank(x, name, b or border)
        else:
            x = np_ref.stencil(x, name, b or border)
    return x


def _chain_images(rng, Cn):
    for shape in ((13, 70), (5, 70), (3, 2)):
        full = shape + ((3,) if Cn == 3 else ())
        yield "random", rng.integers(0, 256, size=full, dtype=np.uint8)
        yield "zeros", np.zeros(full, np.uint8)
        yield "extremes", rng.choice(patterns.EXTREMES, size=full)


@pytest.mark.parametrize("F", FAMILIES)
@pytest.mark.parametrize("pro", PROLOGUES)
def test_constant_border_after_prologue(C, rng, pro, F):
    for Cn in ((3,) if pro.startswith("gray") else (1, 3)):
        for label, img in _chain_images(rng, Cn):
            # as the default border, and as the stencil's own @constant under another default
            for chain, border in ((f"{pro},{F}", "constant"), (f"{pro},{F}@constant", "reflect101")):
                want = _np_chain(img, chain, border)
                fused = C.golden_apply(img, chain, border, True)
                unfused = C.golden_apply(img, chain, border, False)
                assert (fused == unfused).all(), f"{chain} {label} {img.shape}: {_first_bad(fused, unfused)}"
                assert (fused == want).all(), f"{chain} {label} {img.shape}: {_first_bad(fused, want)}"
                assert (C.golden_apply_unfused(img, chain, border) == want).all(), (chain, label)
                for fuse in (True, False):
                    got = C.cpu_apply(img, chain, border, fuse, 2)
                    assert (got == want).all(), f"cpu {chain} fuse={fuse} {label} {img.shape}: {_first_bad(got, want)}"


@pytest.mark.parametrize("chain,iters", [("invert,gaussian5", 1), ("invert,gaussian5", 3), ("brightness:40,median3", 2),
                                         ("gray:ref,brightness:25,emboss3", 1)])
def test_constant_border_chains_row_stripes_host(C, chain, iters):
    """Row stripes of 3 ranks: the pointwise pass zeroes the frame's x-margins
    only, halo rows between stripes carry its pixels; iterated, the stencil
    keeps the margins its own pointwise pass reads."""
    import mpi_cuda_imagemanipulation_amd as m

    W, H = 61, 83
    img = m.utils.synthetic_image(21, W, H, 3)
    got = C.run_local_group(m.Pipeline(chain, "constant").config(W, H, 3, "host"), 3, img, iters)
    ref = img
    for _ in range(iters):
        ref = C.golden_apply(ref, chain, "constant", True)
    assert got.shape == ref.shape and (got == ref).all(), f"{chain} x{iters}: {_first_bad(got, ref)}"


# ---- what the chain compiler fuses --------------------------------------------------
def _kinds(C, chain, cin, border):
    return [p["kind"] for p in C.plan_info(chain, cin, border, True)["passes"]]


@pytest.mark.parametrize("F", FAMILIES)
@pytest.mark.parametrize("pro", PROLOGUES)
def test_plan_flushes_zero_moving_prologue_under_constant(C, pro, F):
    chain = f"{pro},{F}"
    for border in ("reflect101", "replicate"):
        info = C.plan_info(chain, 3, border, True)
        assert len(info["passes"]) == 1 and "prologue[" in info["passes"][0]["desc"], (chain, border)
    assert len(C.plan_info(f"{pro},{F}@skip", 3, "constant", True)["passes"]) == 1
    for ch, border in ((chain, "constant"), (f"{pro},{F}@constant", "reflect101")):
        info = C.plan_info(ch, 3, border, True)
        assert len(info["passes"]) == 2, (ch, border, info)
        assert info["passes"][0]["kind"] == POINTWISE and info["passes"][1]["kind"] != POINTWISE
        assert "prologue[" not in info["passes"][1]["desc"]
        # the pointwise pass owes the stencil its (zero) margins
        assert info["passes"][0]["out_margin_px"] == info["passes"][1]["R"]


@pytest.mark.parametrize("chain", [
    "gray:ref,contrast:3.5,emboss3", "gray,gaussian5", "gray:ref,contrast:3.5,median3", "brightness:-40,box5",
    "threshold:1,sobel", "contrast:3.5,erode3", "gray:ref,contrast:3.5,emboss3,expand",
])
def test_plan_keeps_zero_preserving_prologue_under_constant(C, chain):
    for ch, border in ((chain, "constant"), (chain.replace("emboss3", "emboss3@constant"), "reflect101")):
        info = C.plan_info(ch, 3, border, True)
        assert len(info["passes"]) == 1 and "prologue[" in info["passes"][0]["desc"], (ch, border, info)


def test_plan_mid_chain_lut_under_constant(C):
    # the LUT between two stencils is the second one's prologue: same rule
    assert _kinds(C, "gaussian5,invert,gaussian5", 3, "reflect101") == [1, 1]
    assert _kinds(C, "gaussian5,invert,gaussian5", 3, "constant") == [1, POINTWISE, 1]
    assert _kinds(C, "gaussian5,invert,gaussian5@constant", 3, "reflect101") == [1, POINTWISE, 1]
    assert _kinds(C, "gaussian5@constant,invert,gaussian5", 3, "reflect101") == [1, 1]
    # a trailing LUT is an epilogue of the stencil's own pixels: no border involved
    info = C.plan_info("gaussian5,invert", 3, "constant", True)
    assert len(info["passes"]) == 1 and info["passes"][0]["epi_lut"]
