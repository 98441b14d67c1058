"""Bilateral filters (bilateral3/5[:S]) on the HIP kernel (k_bilateral,
csrc/hip/bilateral_kernels.h) vs the golden path, bit-exact."""
import numpy as np
import pytest

from bilateral_util import frames

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mpi_cuda_imagemanipulation_amd._native import C as _C  # noqa: E402

# every bilateral filter of the stencil catalogue: a new one is covered without an edit here
NAMES = [n for n in _C.stencil_names() if _C.stencil_weights(n)["bilateral"]]
assert {"bilateral3", "bilateral5"} <= set(NAMES)
SIGMAS = [3, 25]
BORDERS = ("reflect101", "replicate", "constant")
# the rank tests' seam shapes.  (7, 992) / (7, 993): a gray row ends exactly on
# a 992-byte output tile / one byte past it; (6, 331): an RGB pixel lies astride
# the tile edge.  17, 37 and 130 rows cross the 12-row band with remainders.
SHAPES = [(1, 1), (3, 2), (2, 7), (17, 15), (64, 65), (37, 1365), (130, 4100), (7, 992), (7, 993), (6, 331)]
CHAINS = ["gray:ref,contrast:3.5,bilateral5:20,expand", "equalize,bilateral3:10", "hold,bilateral5:30,absdiff",
          "bilateral3:10@skip,median3"]


@pytest.fixture(scope="module")
def m():
    import mpi_cuda_imagemanipulation_amd as m

    assert torch.cuda.is_available()
    return m


def _run(m, img, chain, border="reflect101"):
    x = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    y = m.ops.apply(x, chain, border)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("S", SIGMAS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_bilateral_exact(m, rng, name, S, shape, C):
    tok = f"{name}:{S}"
    for kind, img in frames(rng, shape, C).items():
        for border in BORDERS:
            got = _run(m, img, tok, border)
            ref = m._C.golden_apply(img, tok, border, True)
            assert got.shape == ref.shape
            assert (got == ref).all(), (tok, kind, shape, C, border, int((got != ref).sum()))


@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("shape,C", [((64, 65), 1), ((37, 1365), 3), ((130, 4100), 1)])
def test_bilateral_large_sigma_is_the_gaussian_kernel(m, rng, K, shape, C):
    """Every range weight 255: D is at its maximum, and k_bilateral's sums and
    division must give k_sep's gaussianK bit for bit, both on the GPU."""
    img = frames(rng, shape, C)["uniform"]
    for border in BORDERS:
        assert (_run(m, img, f"bilateral{K}:8192", border) == _run(m, img, f"gaussian{K}", border)).all(), border


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape,C", [((45, 77), 1), ((20, 31), 3)])
def test_bilateral_skip_border(m, rng, name, shape, C):
    for kind, img in frames(rng, shape, C).items():
        got = _run(m, img, name + ":25@skip")
        ref = m._C.golden_apply(img, name + ":25@skip", "reflect101", True)
        assert (got == ref).all(), (name, kind, shape)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", [(17, 15), (9, 5000)])
def test_bilateral_expand_epilogue(m, rng, name, shape):
    img = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    chain = f"gray,{name}:12,expand"
    assert m._C.plan_info(chain, 3)["passes"][0]["epi_expand"]
    got = _run(m, img, chain)
    ref = m._C.golden_apply(img, chain, "reflect101", True)
    assert got.shape == ref.shape == shape + (3,)
    assert (got == ref).all()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("shape", [(33, 47), (128, 1000)])
def test_bilateral_chains(m, rng, chain, shape):
    img = frames(rng, shape, 3)["step"]
    got = _run(m, img, chain)
    ref = m._C.golden_apply(img, chain, "reflect101", True)
    assert (got == ref).all(), chain


@pytest.mark.parametrize("chain,iters", [("bilateral5:25", 1), ("bilateral3:10", 5)])
def test_bilateral_local_ranks(m, chain, iters):
    """3 logical ranks on one GPU vs 1 rank, bit-identical; the iterated
    bilateral3 runs the deep-halo schedule at its automatic depth."""
    W, H = 61, 83
    img = m.utils.synthetic_image(21, W, H, 3)
    res = []
    for ranks in (3, 1):
        cfg = m.Pipeline(chain).config(W, H, 3, "device", device=0)
        res.append(m._C.run_local_group(cfg, ranks, img, iters))
    assert (res[0] == res[1]).all()
    ref = img
    for _ in range(iters):
        ref = m._C.golden_apply(ref, chain, "reflect101", True)
    assert (res[0] == ref).all()


@pytest.mark.parametrize("nt", ["0", "1"])
def test_bilateral_both_store_policies(m, rng, monkeypatch, nt):
    monkeypatch.setenv("STRIPE_NT", nt)  # read at every launch
    for C, shape in [(3, (37, 1365)), (1, (130, 4100))]:
        img = frames(rng, shape, C)["uniform"]
        for tok in ("bilateral3:10", "bilateral5:25@replicate"):
            assert (_run(m, img, tok) == m._C.golden_apply(img, tok, "reflect101", True)).all(), (nt, tok)


def test_bilateral_autotune_exact(m):
    C = m._C
    W, H = 2100, 256
    img = m.utils.synthetic_image(5, W, H, 3)
    cfg = m.Pipeline("bilateral3:20").config(W, H, 3, "device", device=0, autotune=True)
    e = C.Engine(cfg)
    e.load_packed(np.ascontiguousarray(img))
    e.run(1)
    e.synchronize()
    bands = e.bands
    assert len(bands) == 1 and bands[0] in (0, 4, 8, 12, 16, 24, 32), bands
    assert (e.store_packed() == C.golden_apply(img, "bilateral3:20", "reflect101", True)).all()


def test_bilateral_deterministic(m, rng):
    img = rng.integers(0, 256, size=(512, 2100, 3), dtype=np.uint8)
    a = _run(m, img, "bilateral5:25")
    b = _run(m, img, "bilateral5:25")
    assert a.tobytes() == b.tobytes()
