"""Two-image ops on the host: hold / swap, the combine ops and their sugar
(gradient, tophat, blackhat, unsharp, threshold:adaptive).

Every rule is integer arithmetic (csrc/include/stripe/filters.h), so every
comparison here is bit-exact.  The oracle of the combine ops is `mirror`, a
numpy transcription of the rule table; the oracle of whole chains is the golden
path applied op by op, whose hold / swap are two assignments.  No GPU."""
import numpy as np
import pytest

import mpi_cuda_imagemanipulation_amd as m

C = m._C

# every combine token, the lincomb / blend coefficients with saturating ones at both ends
COMBINE_TOKENS = [
    "add", "sub", "rsub", "absdiff", "min", "max",
    "lincomb:0.5:0.5", "lincomb:-1:2", "lincomb:7.9:7.9", "lincomb:-7.9:0:2048", "lincomb:1.25:-0.75:-3.5",
    "lincomb:0:0:0.5", "lincomb:-7.9:-7.9:-2048",
    "blend:0", "blend:1", "blend:0.25", "blend:0.3",
    "above", "above:7", "above:-7", "above:255", "above:-255",
]
SUGAR = {
    "gradient3": "hold,dilate3,swap,erode3,sub",
    "gradient5": "hold,dilate5,swap,erode5,sub",
    "tophat3": "hold,erode3,dilate3,sub",
    "tophat5": "hold,erode5,dilate5,sub",
    "blackhat3": "hold,dilate3,erode3,rsub",
    "blackhat5": "hold,dilate5,erode5,rsub",
    "unsharp": "hold,gaussian5,lincomb:-1:2",
    "unsharp:1.5:3": "hold,gaussian3,lincomb:-1.5:2.5",
    "unsharp:6.9:7": "hold,gaussian7,lincomb:-6.9:7.9",
    "threshold:adaptive:3": "hold,box3,above",
    "threshold:adaptive:5:7": "hold,box5,above:7",
    "threshold:adaptive:5:-3": "hold,box5,above:-3",
    "gradient3@replicate": "hold,dilate3@replicate,swap,erode3@replicate,sub",
    "tophat5@constant": "hold,erode5@constant,dilate5@constant,sub",
    "unsharp@constant": "hold,gaussian5@constant,lincomb:-1:2",
    "threshold:adaptive:3:2@replicate": "hold,box3@replicate,above:2",
}
LONG = "hold,gaussian7@constant,swap,emboss5,add,gaussian3"
LONG_PLAIN = "hold,gaussian7,swap,emboss5,add,gaussian3"  # every stencil on the default border
CHAINS = ["gradient3", "gradient5", "tophat3", "tophat5", "blackhat3", "blackhat5", "unsharp", "unsharp:2.5:7",
          "threshold:adaptive:3", "threshold:adaptive:5:7", LONG, LONG_PLAIN]
# slot actions followed by a run that normalises to the identity: no pass of the chain's own is left to
# carry them, so the compiler emits a copy pass (the image they make current is the result)
IDENTITY_TAILS = ["hold,gaussian3,swap,invert,invert", "hold,gaussian3,swap,brightness:0",
                  "hold,gray,swap,brightness:0", "hold,gaussian3,swap,invert,invert,hold,box3,add",
                  "hold,gaussian5,swap,brightness:0,swap,emboss3,sub"]
BORDERS = ["reflect101", "replicate", "constant"]
WIDTHS = [1, 2, 3, 15, 17, 1025]


def q12(v):
    return int(np.rint(4096.0 * float(v)))


def mirror(token, X, H):
    """The rule table of the issue / filters.h in numpy (int64 arithmetic)."""
    X = X.astype(np.int64)
    H = H.astype(np.int64)
    name, *args = token.split(":")
    if name == "add":
        v = np.minimum(255, X + H)
    elif name == "sub":
        v = np.maximum(0, H - X)
    elif name == "rsub":
        v = np.maximum(0, X - H)
    elif name == "absdiff":
        v = np.abs(X - H)
    elif name == "min":
        v = np.minimum(X, H)
    elif name == "max":
        v = np.maximum(X, H)
    elif name in ("lincomb", "blend"):
        if name == "blend":
            qa = q12(args[0])
            qb, qc = 4096 - qa, 0
        else:
            qa, qb = q12(args[0]), q12(args[1])
            qc = q12(args[2]) if len(args) > 2 else 0
        v = np.clip((qa * X + qb * H + qc + 2048) >> 12, 0, 255)  # >> on int64: floor
    elif name == "above":
        d = int(args[0]) if args else 0
        v = np.where(H - X + d > 0, 255, 0)
    else:
        raise AssertionError(token)
    return v.astype(np.uint8)


@pytest.fixture(scope="module")
def pairs():
    x = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)  # x[i, j] = i
    return x, np.ascontiguousarray(x.T)                                  # h[i, j] = j


# ---- parser -------------------------------------------------------------------
def test_tokens_parse():
    for tok in COMBINE_TOKENS:
        assert C.parse_chain("hold," + tok).startswith("hold,"), tok
    assert C.parse_chain("save,gaussian3,swap,invert,add") == "hold,gaussian3,swap,invert,add"
    assert C.parse_chain("hold,blend:0.25") == "hold,lincomb:0.25:0.75"
    assert C.parse_chain("hold,above:0") == "hold,above"
    # the canonical spelling parses back to itself
    for tok in COMBINE_TOKENS:
        s = C.parse_chain("hold," + tok)
        assert C.parse_chain(s) == s


@pytest.mark.parametrize("sugar", sorted(SUGAR))
def test_sugar_expands(sugar):
    assert C.parse_chain(sugar) == C.parse_chain(SUGAR[sugar])


def test_adaptive_before_numeric_threshold():
    assert C.parse_chain("threshold:adaptive:3") == "hold,box3,above"
    assert C.parse_chain("threshold:otsu") == "threshold:otsu" and C.parse_chain("threshold:20") == "threshold:20"


@pytest.mark.parametrize("chain,cin,needle", [
    ("sub", 3, "sub"),                        # combine with nothing held
    ("gaussian3,swap,invert", 3, "swap"),     # swap with nothing held
    ("hold,gray,sub", 3, "sub"),              # channel counts differ
    ("hold,gray,swap,gaussian3,add", 3, "add"),
    ("hold,invert", 3, "hold"),               # a hold no later op reads
    ("hold,invert,hold,sub", 3, "hold"),
    ("hold,gaussian5,swap", 3, "swap"),       # swap as the last op
    ("hold@constant,sub", 3, "hold@constant"),         # @border on a slot / combine op
    ("hold,gaussian3,swap@replicate,sub", 3, "swap@replicate"),
    ("hold,gaussian3,sub@constant", 3, "sub@constant"),
    ("hold,lincomb:1", 3, "lincomb:1"),       # argument counts and ranges
    ("hold,lincomb:9:0", 3, "lincomb:9:0"),
    ("hold,lincomb:1:1:3000", 3, "lincomb:1:1:3000"),
    ("hold,blend", 3, "blend"),
    ("hold,blend:1.5", 3, "blend:1.5"),
    ("hold,above:300", 3, "above:300"),
    ("hold,above:1.5", 3, "above:1.5"),
    ("hold,add:3", 3, "add:3"),
    ("hold:1,add", 3, "hold:1"),
    ("unsharp:0", 3, "unsharp:0"),
    ("unsharp:7", 3, "unsharp:7"),
    ("unsharp:1:9", 3, "unsharp:1:9"),
    ("unsharp:1:5:2", 3, "unsharp:1:5:2"),
    ("threshold:adaptive", 1, "threshold:adaptive"),
    ("threshold:adaptive:7", 1, "threshold:adaptive:7"),
    ("threshold:adaptive:3:0.5", 1, "threshold:adaptive:3:0.5"),
    ("gradient7", 3, "gradient7"),
    ("tophat", 3, "tophat"),
    ("blackhat3:2", 3, "blackhat3:2"),
])
def test_errors_carry_the_token(chain, cin, needle):
    with pytest.raises(RuntimeError) as e:
        C.plan_info(chain, cin)
    assert "'" + needle + "'" in str(e.value), str(e.value)


def test_unknown_filter_lists_the_new_names():
    with pytest.raises(RuntimeError) as e:
        C.parse_chain("nonsuch")
    msg = str(e.value)
    for name in ["hold", "swap", "add", "sub", "rsub", "absdiff", "min", "max", "lincomb:a:b[:c]", "blend:t",
                 "above[:d]", "gradient3 / gradient5", "tophat3 / tophat5", "blackhat3 / blackhat5",
                 "unsharp[:S[:K]]", "threshold:adaptive:K[:C]", "threshold:otsu", "median3 / median5"]:
        assert name in msg, name
    text = " ".join(m.ops.FILTERS)
    for name in ["hold", "swap", "absdiff", "lincomb", "blend", "above", "gradient3", "tophat3", "blackhat3",
                 "unsharp", "threshold:adaptive"]:
        assert name in text, name
    for fn in ["unsharp_mask", "morph_gradient", "top_hat", "black_hat", "adaptive_threshold", "combine", "absdiff",
               "add", "subtract", "blend", "minimum", "maximum"]:
        assert fn in m.ops.__all__ and callable(getattr(m.ops, fn))


# ---- combine_u8 over every byte pair ----------------------------------------------
@pytest.mark.parametrize("token", COMBINE_TOKENS)
def test_combine_u8_all_pairs(pairs, token):
    x, h = pairs
    got = C.combine_u8(token, x, h)
    assert got.dtype == np.uint8 and got.shape == x.shape
    assert (got == mirror(token, x, h)).all(), token


@pytest.mark.parametrize("S", [0.01, 0.5, 1.0, 2.5, 6.9])
def test_unsharp_coefficients(pairs, S):
    x, h = pairs
    tok = C.parse_chain(f"unsharp:{S}").split(",")[-1]
    qa = -q12(S)
    assert tok.startswith("lincomb:-") and C.parse_chain("hold," + tok) == "hold," + tok
    want = np.clip((qa * x.astype(np.int64) + (4096 - qa) * h.astype(np.int64) + 2048) >> 12, 0, 255)
    assert (C.combine_u8(tok, x, h) == want).all()
    flat = np.arange(256, dtype=np.uint8)
    assert (C.combine_u8(tok, flat, flat) == flat).all()  # flat regions are fixed points


def test_fixed_points_and_symmetry(pairs):
    x, h = pairs
    v = np.arange(256, dtype=np.uint8)
    for t in ("blend:0", "blend:0.3", "blend:0.5", "blend:1"):
        assert (C.combine_u8(t, v, v) == v).all(), t
    assert (C.combine_u8("blend:1", x, h) == x).all() and (C.combine_u8("blend:0", x, h) == h).all()
    assert (C.combine_u8("sub", x, h) == C.combine_u8("rsub", h, x)).all()
    assert (C.combine_u8("absdiff", x, h) == C.combine_u8("absdiff", h, x)).all()
    # both ends saturate: sums far above 255 << 12 and far below 0
    assert (C.combine_u8("lincomb:7.9:7.9", x, h)[40:, 40:] == 255).all()
    assert (C.combine_u8("lincomb:-7.9:0:2048", x, h)[:200] == 255).all()
    assert (C.combine_u8("lincomb:-7.9:-7.9:-2048", x, h) == 0).all()
    with pytest.raises(RuntimeError):
        C.combine_u8("invert", x, h)


# ---- planner ------------------------------------------------------------------
def kinds(chain, cin=3, **kw):
    return [p["kind"] for p in C.plan_info(chain, cin, **kw)["passes"]]


def test_plan_lut_after_combine_folds():
    info = C.plan_info("hold,gaussian5,absdiff,threshold:20", 3)
    assert [p["kind"] for p in info["passes"]] == [1, 4]
    assert info["passes"][0]["slots"] == ["hold"] and info["passes"][1]["slots"] == []
    assert info["passes"][1]["combine"] == "absdiff" and info["passes"][1]["post_lut"]
    assert info["branched"] and not info["data_dependent"]
    text = C.describe_chain("hold,gaussian5,absdiff,threshold:20", 3)
    assert "[hold]" in text and "combine absdiff" in text and "post[lut]" in text
    # unfused: the LUT keeps a pass of its own
    assert kinds("hold,gaussian5,absdiff,threshold:20", fuse=False) == [1, 4, 0]


def test_plan_pending_run_is_flushed_by_hold():
    info = C.plan_info("invert,hold,gaussian5,sub", 3)
    assert [p["kind"] for p in info["passes"]] == [0, 1, 4]      # the LUT in a pass of its own
    assert info["passes"][0]["slots"] == [] and info["passes"][1]["slots"] == ["hold"]
    info = C.plan_info("gaussian5,invert,hold,gaussian3,sub", 3)
    assert [p["kind"] for p in info["passes"]] == [1, 1, 4]      # ... or the previous stencil's epilogue
    assert info["passes"][0]["epi_lut"] and info["passes"][1]["slots"] == ["hold"]


def test_plan_slot_ops_break_fusion():
    # a LUT behind a swap works on another image than the last pass wrote: never its epilogue / post table
    assert kinds("hold,gaussian5,swap,invert,add") == [1, 0, 4]
    info = C.plan_info("hold,gaussian5,absdiff,swap,invert,gaussian3,add", 3)
    assert [p["kind"] for p in info["passes"]] == [1, 4, 1, 4] and not info["passes"][1]["post_lut"]
    assert info["passes"][2]["slots"] == ["swap"]
    # a pointwise run before a combine: an epilogue of the stencil, or its own pass; never part of the combine pass
    assert kinds("hold,gaussian5,invert,absdiff") == [1, 4]
    assert kinds("hold,invert,absdiff") == [0, 4]
    # a statistic op after a combine opens a new run
    info = C.plan_info("hold,gaussian5,absdiff,equalize", 3)
    assert [p["kind"] for p in info["passes"]] == [1, 4, 0] and info["passes"][2]["stat"] == "equalize"
    assert info["data_dependent"] and info["branched"]


def test_plan_branched_and_margins():
    for chain in CHAINS + list(SUGAR):
        info = C.plan_info(chain, 3)
        assert info["branched"], chain
        assert info["in_margin_px"] == 0 and all(p["out_margin_px"] == 0 for p in info["passes"]), chain
        for p in info["passes"]:
            assert p["fill_in"] == (p["R"] > 0), (chain, p["desc"])
    for chain in ["gaussian5", "gaussian5,gaussian3", "invert", "open3", "gray,equalize,gaussian5"]:
        info = C.plan_info(chain, 3)
        assert not info["branched"] and not any(p["fill_in"] or p["slots"] for p in info["passes"]), chain
    two = C.plan_info("gaussian5,gaussian3", 3)  # the straight-line contract is what it was
    assert two["in_margin_px"] == 2 and [p["out_margin_px"] for p in two["passes"]] == [1, 2]


def test_plan_identity_tail_keeps_its_slot_actions():
    info = C.plan_info("hold,gaussian3,swap,invert,invert", 3)
    assert [p["kind"] for p in info["passes"]] == [1, 0]
    assert info["passes"][0]["slots"] == ["hold"] and info["passes"][1]["slots"] == ["swap"]
    assert "copy" in info["passes"][1]["desc"]
    info = C.plan_info("hold,gray,swap,brightness:0", 3)
    assert info["cin"] == 3 and info["cout"] == 3
    assert [(p["cin"], p["cout"], p["slots"]) for p in info["passes"]] == [(3, 1, ["hold"]), (3, 3, ["swap"])]
    # in the middle of a chain the actions wait for the next pass, in order
    info = C.plan_info("hold,gaussian3,swap,invert,invert,hold,box3,add", 3)
    assert [p["slots"] for p in info["passes"]] == [["hold"], ["swap", "hold"], []]


@pytest.mark.parametrize("chain", IDENTITY_TAILS)
def test_identity_tail_fused_unfused_and_host(rng, chain):
    for W in (1, 17, 131):
        img = rng.integers(0, 256, size=(9, W, 3), dtype=np.uint8)
        ref = C.golden_apply_unfused(img, chain, "reflect101")
        assert ref.shape == img.shape
        for fuse in (True, False):
            assert (C.golden_apply(img, chain, "reflect101", fuse) == ref).all(), (chain, W, fuse)
            assert (C.cpu_apply(img, chain, "reflect101", fuse) == ref).all(), (chain, W, fuse)
        cfg = m.Pipeline(chain).config(W, 9, 3, "host")
        assert (C.run_local_group(cfg, 2, img, 1) == ref).all(), (chain, W)
    if chain.endswith(("invert,invert", "brightness:0")):  # the swap brings the original back
        assert (ref == img).all()


def test_plan_external_held():
    info = C.plan_info("absdiff", 3, held_channels=3)
    assert [p["kind"] for p in info["passes"]] == [4] and info["branched"]
    assert kinds("gaussian5,blend:0.5,invert", 1, held_channels=1) == [1, 4]
    with pytest.raises(RuntimeError):
        C.plan_info("absdiff", 3)
    with pytest.raises(RuntimeError):
        C.plan_info("absdiff", 3, held_channels=1)


# ---- golden fused / unfused, host executor ------------------------------------------
def _frames(rng, W, cc, Hh=7):
    shape = (Hh, W) if cc == 1 else (Hh, W, cc)
    yield rng.integers(0, 256, size=shape, dtype=np.uint8)
    yy, xx = np.mgrid[0:Hh, 0:W]
    chk = (((yy + xx) & 1) * 255).astype(np.uint8)
    yield np.ascontiguousarray(chk if cc == 1 else np.repeat(chk[:, :, None], 3, axis=2))


@pytest.mark.parametrize("cc", [1, 3])
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("chain", CHAINS)
def test_golden_fused_unfused_and_host(rng, chain, border, cc):
    for W in WIDTHS:
        for img in _frames(rng, W, cc):
            ref = C.golden_apply_unfused(img, chain, border)
            assert ref.shape == img.shape
            assert (C.golden_apply(img, chain, border, True) == ref).all(), (chain, border, W)
            assert (C.golden_apply(img, chain, border, False) == ref).all(), (chain, border, W)
            assert (C.cpu_apply(img, chain, border, True) == ref).all(), (chain, border, W)
            assert (m.ops.apply(img, chain, border) == ref).all()


def test_sugar_against_its_definition(rng):
    """The named filters against their formulas on the stencils' own outputs."""
    img = rng.integers(0, 256, size=(33, 70, 3), dtype=np.uint8)
    g = lambda ch: C.golden_apply(img, ch, "reflect101", True).astype(np.int64)  # noqa: E731
    x = img.astype(np.int64)
    assert (g("gradient3") == g("dilate3") - g("erode3")).all()
    assert (g("tophat5") == x - g("open5")).all() and (g("blackhat3") == g("close3") - x).all()
    assert (g("unsharp") == np.clip(2 * x - g("gaussian5"), 0, 255)).all()
    assert (g("threshold:adaptive:5:7") == np.where(x > g("box5") - 7, 255, 0)).all()
    assert (m.ops.unsharp_mask(img, 1.0, 5) == g("unsharp")).all()
    assert (m.ops.morph_gradient(img) == g("gradient3")).all() and (m.ops.top_hat(img, 5) == g("tophat5")).all()
    assert (m.ops.black_hat(img) == g("blackhat3")).all()
    assert (m.ops.adaptive_threshold(img, 5, 7) == g("threshold:adaptive:5:7")).all()


def test_held_image_on_the_host(rng):
    a = rng.integers(0, 256, size=(9, 131, 3), dtype=np.uint8)
    b = rng.integers(0, 256, size=(9, 131, 3), dtype=np.uint8)
    for tok in ("absdiff", "add", "blend:0.25", "lincomb:-7.9:0:2048", "above:3"):
        want = mirror(tok, a, b)
        assert (m.ops.combine(a, b, tok) == want).all(), tok
        assert (C.golden_apply(a, tok, "reflect101", True, b) == want).all()
        assert (C.golden_apply_unfused(a, tok, "reflect101", b) == want).all()
    assert (m.ops.absdiff(a, b) == mirror("absdiff", a, b)).all()
    assert (m.ops.subtract(a, b) == mirror("rsub", a, b)).all() and (m.ops.add(a, b) == mirror("add", a, b)).all()
    assert (m.ops.minimum(a, b) == np.minimum(a, b)).all() and (m.ops.maximum(a, b) == np.maximum(a, b)).all()
    assert (m.ops.blend(a, b, 0.25) == mirror("blend:0.25", a, b)).all()
    # the held image behind a stencil and a swap
    ch = "gaussian3,swap,gaussian5@constant,add"
    want = mirror("add", C.golden_apply(b, "gaussian5@constant"), C.golden_apply(a, "gaussian3"))
    assert (m.ops.combine(a, b, ch) == want).all()
    with pytest.raises(ValueError):
        m.ops.combine(a, b[:, :50], "add")
    with pytest.raises(RuntimeError):
        C.golden_apply(a, "gaussian5", "reflect101", True, b[:, :, 0])  # held channels differ


# ---- host backend: ranks --------------------------------------------------------
def test_host_three_ranks_one_idle(rng):
    """H = 2 over 3 host ranks (one idles), run(3) of a chain with a swap and two held images."""
    chain, W, Hh = "gradient3,unsharp", 131, 2
    img = rng.integers(0, 256, size=(Hh, W, 3), dtype=np.uint8)
    ref = img
    for _ in range(3):
        ref = C.golden_apply(ref, chain, "reflect101", True)
    cfg = m.Pipeline(chain).config(W, Hh, 3, "host")
    one = C.run_local_group(cfg, 1, img, 3)
    three = C.run_local_group(cfg, 3, img, 3)
    assert (one == ref).all() and (three == ref).all()
    tall = rng.integers(0, 256, size=(41, W, 1), dtype=np.uint8)[:, :, 0]
    cfg = m.Pipeline(LONG).config(W, 41, 1, "host")
    assert (C.run_local_group(cfg, 3, tall, 1) == C.golden_apply(tall, LONG, "reflect101", True)).all()


def test_host_engine_external_held(rng):
    a = rng.integers(0, 256, size=(12, 77, 3), dtype=np.uint8)
    b = rng.integers(0, 256, size=(12, 77, 3), dtype=np.uint8)
    cfg = m.Pipeline("blend:0.25").config(77, 12, 3, "host")
    cfg.held_input = True
    e = C.Engine(cfg)
    e.load_packed(a)
    e.load_held_packed(b)
    e.run(3)  # no hold or swap: the held image stays, the chain iterates
    want = a
    for _ in range(3):
        want = mirror("blend:0.25", want, b)
    assert (e.store_packed() == want).all()
    cfg = m.Pipeline("gaussian3,swap,add").config(77, 12, 3, "host")
    cfg.held_input = True
    e = C.Engine(cfg)
    e.load_packed(a)
    e.load_held_packed(b)
    with pytest.raises(RuntimeError, match="hold or swap"):
        e.run(2)
    # a chain that holds may overwrite the external image's buffer: it is spent after one run
    ch = "add,hold,gaussian3,add"
    cfg = m.Pipeline(ch).config(77, 12, 3, "host")
    cfg.held_input = True
    e = C.Engine(cfg)
    for _ in range(2):
        e.load_packed(a)
        e.load_held_packed(b)
        e.run(1)
        assert (e.store_packed() == C.golden_apply(a, ch, "reflect101", True, b)).all()
    e.load_packed(a)
    with pytest.raises(RuntimeError, match="held"):
        e.run(1)
    cfg = m.Pipeline("add").config(77, 12, 3, "host")
    cfg.held_input = True
    with pytest.raises(RuntimeError, match="held"):
        C.run_local_group(cfg, 1, a, 1)
    with pytest.raises(RuntimeError, match="held"):  # a combine with no held image loaded
        e = C.Engine(cfg)
        e.load_packed(a)
        e.run(1)


# ---- CLI: a second image as the held one -----------------------------------------
def test_cli_held_image(tmp_path):
    import os
    import subprocess

    from mpi_cuda_imagemanipulation_amd import utils

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "stripe")
    assert os.path.exists(exe), "bin/stripe not built"

    def run(*args):
        return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300,
                              env=dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", "")))

    a, b, out = tmp_path / "a.ppm", tmp_path / "b.ppm", tmp_path / "out.ppm"
    for path, seed in ((a, 5), (b, 6)):
        assert run("gen", "--synthetic", "131x37x3", "--seed", seed, "--output", path).returncode == 0
    r = run("run", "--input", a, "--held", b, "--output", out, "--chain", "absdiff,threshold:20", "--backend", "host")
    assert r.returncode == 0, r.stdout + r.stderr
    x, h = utils.read_image(a), utils.read_image(b)
    want = np.where(mirror("absdiff", x, h) >= 20, 255, 0)
    assert (utils.read_image(out) == want).all()
    # iterated: the held image stays
    r = run("run", "--input", a, "--held", b, "--output", out, "--chain", "blend:0.5", "--iterations", 2,
            "--backend", "host")
    assert r.returncode == 0, r.stdout + r.stderr
    assert (utils.read_image(out) == mirror("blend:0.5", mirror("blend:0.5", x, h), h)).all()
    r = run("run", "--input", a, "--held", b, "--output", out, "--chain", "add", "--ranks", 2, "--backend", "host")
    assert r.returncode != 0 and "--held" in r.stderr
    small = tmp_path / "small.ppm"
    assert run("gen", "--synthetic", "64x37x3", "--seed", 7, "--output", small).returncode == 0
    r = run("run", "--input", a, "--held", small, "--output", out, "--chain", "add", "--backend", "host")
    assert r.returncode != 0 and "--held" in r.stderr
    # without --held a bare combine op is a compile-time error that names the token
    r = run("run", "--input", a, "--output", out, "--chain", "add", "--backend", "host")
    assert r.returncode != 0 and "'add'" in r.stderr
