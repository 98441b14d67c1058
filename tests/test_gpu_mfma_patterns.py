"""The float MFMA kernels (k_blur_pl, k_conv_mfma, k_conv_i8) against torch fp64
on the saturated / structured frames of tests/patterns.py with impulses at
these kernels' own seams, with weights whose outputs clamp at both ends, with
integer weights (bit-exact, no tolerance), at forced band depths, on the
cold-policy kernels, on the worst case of the conv `:lsb` bound and inside
chains.  Cases and weight recipes: tests/mfma_cases.py.  The CPU tests at the
end keep the GPU tests honest (tie-band occupancy, integer sums, the bounds of
the worst-case weights, the golden path on the integer recipes).
"""
import numpy as np
import pytest

import mfma_cases as mc
import oracle
import patterns

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu
PATH_IDS = [mc.path_id(p) for p in mc.PATHS]


@pytest.fixture(scope="module")
def m():
    import mpi_cuda_imagemanipulation_amd as m

    return m


def _run_frames(m, frames, chain, border):
    """ops.apply on a stack of equally shaped frames (one engine, frame by frame)."""
    x = np.stack(frames)
    if x.ndim == 3:
        x = x[..., None]
    y = m.ops.apply(torch.from_numpy(np.ascontiguousarray(x)).cuda(), chain, border)
    torch.cuda.synchronize()
    return y.cpu().numpy().reshape(np.stack(frames).shape)


def _sums(labelled, w, border, device):
    """fp64 sums of every frame of one shape (one oracle call for the whole stack)."""
    if device == "cpu":  # the same sums, an order of magnitude faster there (test_block_sums_match_torch)
        return mc.unstack(mc.block_sums(mc.stack(labelled), w, border), labelled)
    return mc.unstack(oracle.torch_sums(mc.stack(labelled), w, border, device=device), labelled)


def _assert_exact(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (f"{what}: {len(bad)} mismatches, first {bad[:5].tolist()}, "
                           f"got {[int(got[tuple(b)]) for b in bad[:5]]} want {[int(ref[tuple(b)]) for b in bad[:5]]}")


def _assert_desc(m, chain, C, path, K):
    kind, lsb = mc.expected_desc(path, C, K)
    desc = m._C.plan_info(chain, C)["passes"][0]["desc"]
    assert kind in desc and desc.endswith(" lsb") == lsb, (path, K, C, desc)


# ---- a. integer weights, bit-exact --------------------------------------------------
@gpu
@pytest.mark.parametrize("path,K,C", mc.PATHS, ids=PATH_IDS)
def test_mfma_int_weights_exact(m, path, K, C):
    """Integer taps on bytes: every sum is an integer below 2^24, exact in f16
    hi + lo, in single f16 parts, in i8 digits and in f32 in any order, and
    never at a tie: no tolerance, in the exact and the `:lsb` modes."""
    for recipe in mc.int_recipes(path):
        chain, w = mc.path_case(path, K, recipe)
        _assert_desc(m, chain, C, path, K)
        for H, W in mc.path_shapes(path, C):
            labelled = mc.frames(H, W, C)
            for border in mc.BORDERS:
                got = _run_frames(m, [im for _, im in labelled], chain, border)
                for (label, img), g, s in zip(labelled, got, _sums(labelled, w, border, "cuda")):
                    _assert_exact(g, oracle.finish(s), f"{path} K={K} {recipe} {border} {label} {img.shape}")


# ---- b. float weights whose outputs clamp, tie-aware --------------------------------
@gpu
@pytest.mark.parametrize("path,K,C", mc.PATHS, ids=PATH_IDS)
def test_mfma_float_weights_clamped(m, path, K, C):
    """`unit`, `gain3` / `neg3` (the upper / lower clamp on most of a saturated
    frame) and `hp` (zero sum: the lower clamp on about half of a textured
    frame).  Exact modes: no mismatch outside the tie band; `:lsb`: every output
    within 1 LSB.  The clamps are checked to be reached from the fp64 sums
    alone: of all pixels compared under `gain3` and `hp` at least 20 % lie
    above 255, of all compared under `neg3` and `hp` at least 20 % below 0."""
    lsb = path.endswith("_lsb")
    n = {"gain3": 0, "neg3": 0, "hp": 0}
    below, above = dict(n), dict(n)
    for recipe in mc.FLOAT_RECIPES:
        chain, w = mc.path_case(path, K, recipe)
        _assert_desc(m, chain, C, path, K)
        band = mc.scaled_band(w)
        for H, W in mc.path_shapes(path, C):
            labelled = mc.frames(H, W, C)
            for border in ("reflect101", "constant"):
                got = _run_frames(m, [im for _, im in labelled], chain, border)
                for (label, img), g, s in zip(labelled, got, _sums(labelled, w, border, "cuda")):
                    r = oracle.compare(g, s, band)
                    what = (path, K, C, recipe, border, label, img.shape, r)
                    assert r["max_diff"] <= 1, what
                    assert lsb or r["mismatch_outside_ties"] == 0, what
                    if recipe != "unit":
                        n[recipe] += s.size
                        below[recipe] += int((s < 0).sum())
                        above[recipe] += int((s > 255).sum())
    _assert_clamps_reached(path, K, C, n, below, above)


def _assert_clamps_reached(path, K, C, n, below, above):
    lo = (below["neg3"] + below["hp"]) / (n["neg3"] + n["hp"])
    hi = (above["gain3"] + above["hp"]) / (n["gain3"] + n["hp"])
    print(f"{path} K={K} C={C}: {lo:.3f} of the neg3 + hp sums below 0, {hi:.3f} of the gain3 + hp sums above 255")
    assert lo >= 0.2 and hi >= 0.2, (path, K, C, lo, hi)


@gpu
@pytest.mark.parametrize("K", [9, 31, 33])
@pytest.mark.parametrize("lsb", [False, True])
def test_gaussian_blur_patterns(m, K, lsb):
    """blur:K itself (the Gaussian taps the `:lsb` single-part kernel was built
    for: its bound holds, so this is that kernel) on the same frames, RGB."""
    chain = f"blur:{K}" + (":lsb" if lsb else "")
    w = oracle.blur_weights(m._C, K)
    h = np.asarray(m._C.gaussian_1d(K), np.float32)
    assert mc.sep_lsb_bound(h, h) < 0.45
    for H, W in mc.blur_shapes(3):
        labelled = mc.frames(H, W, 3)
        for border in ("reflect101", "constant"):
            got = _run_frames(m, [im for _, im in labelled], chain, border)
            for (label, img), g, s in zip(labelled, got, _sums(labelled, w, border, "cuda")):
                r = oracle.compare(g, s, mc.GPU_BAND)
                assert r["max_diff"] <= 1 and (lsb or r["mismatch_outside_ties"] == 0), (chain, border, label, img.shape, r)


# ---- c. the largest single-conversion K of the i8 epilogue --------------------------
@gpu
@pytest.mark.parametrize("lsb", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_conv31_uniform_box_saturated(m, rng, lsb, C):
    """K = 31: a top-digit sum over a uniform box on saturated pixels reaches
    961 * 128 * 127 < 2^24, the largest the one-conversion epilogue takes."""
    K = 31
    w = oracle.f32_weights(np.full((K, K), 1.0 / (K * K)))
    img = np.where(rng.random((120, 260)) < 0.5, 0, 255).astype(np.uint8)
    img[:, :130] = 0
    img[:60, 130:] = 255
    frames = [img, np.zeros_like(img), np.full_like(img, 255)]
    if C == 3:
        frames = [np.stack([f, 255 - f, f], axis=-1) for f in frames[:1]] + [np.stack([f] * 3, axis=-1) for f in frames[1:]]
    chain = mc.conv_chain(w, lsb)
    _assert_desc(m, chain, C, "i8_lsb" if lsb else "i8", K)
    got = _run_frames(m, frames, chain, "reflect101")
    r = oracle.compare(got[0], oracle.torch_sums(frames[0], w, "reflect101", device="cuda"), mc.GPU_BAND)
    assert r["max_diff"] <= 1, r
    if not lsb:
        assert r["mismatch_outside_ties"] == 0, r
    assert (got[1] == 0).all() and (got[2] == 255).all(), (np.unique(got[1]), np.unique(got[2]))


# ---- d. worst case of the conv :lsb bound -------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["one", "mixed"])
@pytest.mark.parametrize("K", [13, 31])
@pytest.mark.parametrize("C", [1, 3])
def test_conv_lsb_bound_worst_case(m, K, kind, C):
    """The frame is 255 exactly where the 16-bit weight residual is positive (and
    its complement): sum (x - 128) r reaches the host's bound 128 sum |r| 2^-S.
    Every output lies within 0.5 + bound + band of the clipped fp64 sum.
    Measured on MI355X, worst |got - sums| (rounding included) over the frame
    and its complement: K = 13 (bound 0.2625) 0.568 one sign, 0.518 mixed; K = 31
    (bound 0.3125) 0.798 one sign, 0.549 mixed; the limit is 0.7625 / 0.8125."""
    w = mc.lsb_worst_weights(K, kind)
    bound = mc.conv_quant_bound(w, 2)
    assert 0.25 <= bound < 0.45
    chain = mc.conv_chain(w, True)
    _assert_desc(m, chain, C, "i8_lsb", K)
    H, W = 2 * K + 7, 64 + 2 * K + 3
    frames = [mc.lsb_worst_frame(w, H, W, C, comp) for comp in (False, True)]
    got = _run_frames(m, frames, chain, "reflect101")
    for img, g in zip(frames, got):
        s = oracle.torch_sums(img, w, "reflect101", device="cuda")
        err = np.abs(g.astype(np.float64) - np.clip(s, 0, 255))
        print(f"conv:{K}:lsb {kind} C={C}: worst |got - sums| {err.max():.4f}, 0.5 + bound {0.5 + bound:.4f}")
        assert err.max() <= 0.5 + bound + mc.scaled_band(w), (K, kind, C, err.max(), bound)


# ---- e. deep bands and the cold kernels ---------------------------------------------
def _engine_run(m, chain, img, band, cold):
    H, W = img.shape[:2]
    C = 1 if img.ndim == 2 else 3
    cfg = m.Pipeline(chain).config(W, H, C, "device", device=0)
    cfg.band = band
    cfg.cold = cold
    e = m._C.Engine(cfg)
    e.load_packed(np.ascontiguousarray(img))
    e.run(1)
    e.synchronize()
    return np.asarray(e.store_packed()).reshape(img.shape)


DEEP_CHAINS = ["blur:31", "blur:31:lsb", "int"]


@gpu
@pytest.mark.parametrize("W,C", [(292, 3), (257, 3), (1028, 1), (131, 1)])
@pytest.mark.parametrize("which", DEEP_CHAINS)
def test_blur_deep_bands_and_cold(m, rng, which, W, C):
    """161 rows under forced bands of 64 / 96 / 128 / 160 rows: 2 + 2 + 2, 3 + 3,
    4 + 2 and 5 + 1 groups of 32 rows per band, so the steady-state steps, the
    window-buffer alternation, both tail parities and the prefetch guard run;
    cold = True selects the streaming policy (the early-staging `:lsb` RGB
    kernel, no XCD remap).  Summation is partition-independent: every
    configuration equals band = 0, cold = False byte for byte."""
    H = 161
    if which == "int":
        h, v = mc.sep_weights("int", 9)
        chain, w = mc.sep_chain(h, v), mc.sep_matrix(h, v)
    else:
        chain, w = which, oracle.blur_weights(m._C, 31)
    shape = (H, W) if C == 1 else (H, W, 3)
    checker = dict(mc.frames(H, W, C))["checker0" if C == 1 else "checker0/shift"]
    for label, img in (("random", rng.integers(0, 256, size=shape, dtype=np.uint8)),
                       ("all255", np.full(shape, 255, np.uint8)), ("checker0", checker)):
        base = _engine_run(m, chain, img, 0, False)
        s = oracle.torch_sums(img, w, "reflect101", device="cuda")
        if which == "int":
            _assert_exact(base, oracle.finish(s), f"{chain} {label} {shape}")
        else:
            r = oracle.compare(base, s, mc.GPU_BAND)
            assert r["max_diff"] <= 1 and (which.endswith("lsb") or r["mismatch_outside_ties"] == 0), (which, label, r)
        for band in (0, 64, 96, 128, 160):
            for cold in (False, True):
                if band or cold:
                    _assert_exact(_engine_run(m, chain, img, band, cold), base,
                                  f"{which} {label} {shape} band={band} cold={cold} vs band=0")
        if which == "int" and label == "random":
            # 3 stripes of 53 / 54 rows: row0 is no multiple of 32, the 32-row grid starts above the stripe
            cfg = m.Pipeline(chain).config(W, H, C, "device", device=0)
            cfg.band = 96
            got = np.asarray(m._C.run_local_group(cfg, 3, img, 1)).reshape(shape)
            _assert_exact(got, base, f"{which} {shape} band=96 on 3 local ranks vs one rank")


# ---- f. conv / blur passes inside chains --------------------------------------------
def _chain_filters():
    h, v = mc.sep_weights("int", 9)
    hl, vl = mc.sep_weights("int_lsb_h", 9)
    w = mc.conv_weights("int", 13)
    return {"sepconv9": mc.sep_chain(h, v), "sepconv9_lsb": mc.sep_chain(hl, vl, True),
            "conv13": mc.conv_chain(w), "conv13_lsb": mc.conv_chain(w, True)}


CHAIN_FORMS = ["gaussian5,{F},sobel", "gray,{F},expand", "invert,{F}", "{F},{F}"]


@gpu
@pytest.mark.parametrize("F", list(_chain_filters()))
@pytest.mark.parametrize("form", CHAIN_FORMS)
def test_mfma_pass_inside_chain(m, rng, F, form):
    """The conv / blur pass reads x-margins a stencil or pointwise pass wrote and
    fills its own output margins for the next stencil; integer weights, so the
    golden path (pinned by test_golden_int_recipes_match_oracle) is exact."""
    f = _chain_filters()[F]
    chain = form.format(F=f)
    runs = [(chain, b) for b in mc.BORDERS]
    if form == "invert,{F}":
        runs.append((f"invert,{f}@constant", "reflect101"))
    for shape in ((5, 70, 3), (33, 331, 3), (161, 260, 3)):
        frames = [rng.integers(0, 256, size=shape, dtype=np.uint8), np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)]
        for ch, border in runs:
            got = _run_frames(m, frames, ch, border)
            for label, img, g in zip(("random", "zeros", "all255"), frames, got):
                _assert_exact(g, m._C.golden_apply(img, ch, border, True), f"{form} {F} {border} {label} {shape}")


@gpu
@pytest.mark.parametrize("form,F,border", [("invert,{F}", "sepconv9", "constant"), ("gaussian5,{F},sobel", "conv13_lsb", "reflect101")])
def test_mfma_chain_local_ranks(m, form, F, border):
    W, H = 61, 83
    chain = form.format(F=_chain_filters()[F])
    img = m.utils.synthetic_image(21, W, H, 3)
    ref = m._C.golden_apply(img, chain, border, True)
    for ranks in (3, 1):
        cfg = m.Pipeline(chain, border).config(W, H, 3, "device", device=0)
        _assert_exact(np.asarray(m._C.run_local_group(cfg, ranks, img, 1)), ref, f"{form} {F} {border} on {ranks} ranks")


# ---- CPU checks that keep the GPU tests honest --------------------------------------
# blur / blur_lsb and i8 / i8_lsb share weights and frames: one check per weight set
SUM_CASES = sorted({(p.split("_")[0], K, C) for p, K, C in mc.PATHS})


@pytest.mark.parametrize("path,K,C", SUM_CASES, ids=[mc.path_id(p) for p in SUM_CASES])
def test_float_cases_stay_off_the_tie_band(path, K, C):
    """The tie-aware comparison says nothing about a pixel inside the band: on
    every frame of test_mfma_float_weights_clamped the fp64 sums alone leave at
    most 5 % of the pixels there (a frame above the cap: change the seed)."""
    worst = 0.0
    n = {"gain3": 0, "neg3": 0, "hp": 0}
    below, above = dict(n), dict(n)
    for recipe in mc.FLOAT_RECIPES:
        _, w = mc.path_case(path, K, recipe)
        band = mc.scaled_band(w)
        assert 255.0 * np.abs(w).sum() <= 2400.0, (recipe, K)
        for H, W in mc.path_shapes(path, C):
            labelled = mc.frames(H, W, C)
            for border in ("reflect101", "constant"):
                sums = _sums(labelled, w, border, "cpu")
                if recipe != "unit":
                    n[recipe] += sum(s.size for s in sums)
                    below[recipe] += sum(int((s < 0).sum()) for s in sums)
                    above[recipe] += sum(int((s > 255).sum()) for s in sums)
                if H * W < 20:
                    # (1, 1) and (3, 2): one pixel is more than 5 % of the frame, so
                    # the cap holds for the shape's frames taken together
                    sums = [np.stack(sums)]
                for label, s in zip([l for l, _ in labelled] if len(sums) > 1 else ["all frames"], sums):
                    frac = np.abs(s - np.floor(s) - 0.5)
                    share = float(((frac < band) & (s > -0.5) & (s < 255.5)).mean())
                    worst = max(worst, share)
                    assert share <= 0.05, (path, K, C, recipe, border, label, (H, W), share)
    print(f"{path} K={K} C={C}: at most {worst:.4f} of a frame inside the tie band")
    _assert_clamps_reached(path, K, C, n, below, above)  # the GPU test's own check, known before it runs


def test_block_sums_match_torch(rng):
    for (H, W, C), K in (((1, 1, 1), 9), ((3, 2, 3), 33), ((37, 67, 3), 13), ((33, 131, 1), 31)):
        labelled = [("random", rng.integers(0, 256, size=(H, W) if C == 1 else (H, W, 3), dtype=np.uint8))] + mc.frames(H, W, C)[:8]
        w = mc.conv_weights("hp", K)
        for border in mc.BORDERS:
            a, b = oracle.torch_sums(mc.stack(labelled), w, border), mc.block_sums(mc.stack(labelled), w, border)
            assert a.shape == b.shape and np.abs(a - b).max() < 1e-9, (H, W, C, K, border, np.abs(a - b).max())


@pytest.mark.parametrize("K", [7, 9, 11, 13, 17, 31, 33])
def test_int_recipes_are_integer_and_bounded(K):
    cases = [mc.conv_weights("int", K)]
    w = cases[0]
    assert (w == np.rint(w)).all() and np.abs(w).max() <= 64 and w.sum() == 1 and (w < 0).any()
    assert not (w == w.T).all() and not (w == w[::-1, ::-1]).all()
    if K >= 9:
        for recipe in ("int", "int_lsb_h", "int_lsb_v"):
            h, v = mc.sep_weights(recipe, K)
            assert (h == np.rint(h)).all() and (v == np.rint(v)).all() and h.sum() == 1 and v.sum() == 1
            assert np.abs(h).sum() <= 16 and np.abs(v).sum() <= 16 and not (h == v).all() and not (h == h[::-1]).all()
            # which kernel `:lsb` runs: the single-part one only below 0.45 LSB
            assert (mc.sep_lsb_bound(h, v) < 0.45) == (recipe != "int"), (recipe, mc.sep_lsb_bound(h, v))
            cases.append(mc.sep_matrix(h, v))
    for w in cases:
        assert 255.0 * np.abs(w).sum() < 2 ** 24
        assert mc.conv_quant_bound(w, 2) == 0 and mc.conv_quant_bound(w, 3) == 0  # whole digits
        for C, borders in ((1, mc.BORDERS), (3, ("reflect101",))):
            labelled = mc.frames(33, 129, C)
            for border in borders:
                for s in _sums(labelled, w, border, "cpu"):
                    assert (s == np.rint(s)).all() and np.abs(s).max() < 2 ** 24


@pytest.mark.parametrize("kind", ["one", "mixed"])
@pytest.mark.parametrize("K", [13, 31])
def test_lsb_worst_case_weights(K, kind):
    w = mc.lsb_worst_weights(K, kind)
    bound = mc.conv_quant_bound(w, 2)
    assert 0.25 <= bound < 0.45 and mc.conv_shift(w, 2) == 15, bound
    r = mc.conv_residuals(w, 2)
    assert np.abs(r).max() < 0.41 and ((r > 0).any() and (r < 0).any()) == (kind == "mixed")
    assert 0 < 255.0 * w[w > 0].sum() < 255.0 and w.max() == 0.5
    # on the aligned window of the frame the residual term reaches the bound
    img = mc.lsb_worst_frame(w, 3 * K, 3 * K, 1, complement=(kind == "one"))
    x = img[:K, :K].astype(np.float64) - 128.0
    assert abs(np.ldexp(np.abs((x * r).sum()), -15)) >= 0.99 * bound


@pytest.mark.parametrize("C", [1, 3])
def test_golden_int_recipes_match_oracle(m, C):
    """The golden path on the integer recipes equals sat(rne(fp64 sums)) exactly,
    on every pattern: it is the reference of test_mfma_pass_inside_chain."""
    h, v = mc.sep_weights("int", 9)
    hl, vl = mc.sep_weights("int_lsb_h", 9)
    w13 = mc.conv_weights("int", 13)
    for chain, w in ((mc.sep_chain(h, v), mc.sep_matrix(h, v)), (mc.sep_chain(hl, vl, True), mc.sep_matrix(hl, vl)),
                     (mc.conv_chain(w13), w13), (mc.conv_chain(w13, True), w13)):
        for H, W in patterns.host_shapes(C):
            labelled = list(patterns.patterns(H, W, C, seams=mc.seams(C)))
            for border in mc.BORDERS:
                for (label, img), s in zip(labelled, _sums(labelled, w, border, "cpu")):
                    _assert_exact(m._C.golden_apply(img, chain, border, True), oracle.finish(s),
                                  f"golden K={w.shape[0]} {border} {label} {img.shape}")
