"""Rank filters (median3/5, erode3/5, dilate3/5, open/close) on the HIP kernels
(k_rank, csrc/hip/rank_kernels.h) vs the golden path, bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mpi_cuda_imagemanipulation_amd._native import C as _C  # noqa: E402

# every rank filter of the stencil catalogue: a new one is covered without an edit here
NAMES = [n for n in _C.stencil_names() if _C.stencil_weights(n)["rank"] != "none"]
assert {"median3", "median5", "erode3", "erode5", "dilate3", "dilate5"} <= set(NAMES)
BORDERS = ("reflect101", "replicate", "constant")
# (7, 992) / (7, 993): a gray row ends exactly on a 992-byte output tile / one
# byte past it; (6, 331): an RGB pixel lies astride the tile edge.  17, 37 and
# 130 rows cross the 12-row band with remainders 5, 1 and 10.
SHAPES = [(1, 1), (3, 2), (2, 7), (17, 15), (64, 65), (37, 1365), (130, 4100), (9, 5000), (7, 992), (7, 993),
          (6, 331)]
CHAINS = ["gray:ref,contrast:3.5,median3,expand", "median3,threshold:128,open3", "gaussian5,dilate5@constant,invert",
          "erode3@skip,median5"]
TIES = np.array([0, 1, 2, 253, 254, 255], np.uint8)


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


def _images(rng, shape, C):
    full = shape + (3,) if C == 3 else shape
    # uniform bytes, and a tie image: equal keys and the byte extremes are where
    # a compare-exchange network goes wrong
    return [rng.integers(0, 256, size=full, dtype=np.uint8), rng.choice(TIES, size=full)]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_rank_exact(m, rng, name, shape, C):
    for img in _images(rng, shape, C):
        for border in BORDERS:
            got = _run(m, img, name, border)
            ref = m._C.golden_apply(img, name, border, True)
            assert got.shape == ref.shape
            assert (got == ref).all(), (name, shape, C, border, int((got != ref).sum()))


@pytest.mark.parametrize("name", ["median3", "median5", "erode5", "dilate3"])
@pytest.mark.parametrize("shape,C", [((45, 77), 1), ((20, 31), 3)])
def test_rank_skip_border(m, rng, name, shape, C):
    for img in _images(rng, shape, C):
        got = _run(m, img, name + "@skip")
        ref = m._C.golden_apply(img, name + "@skip", "reflect101", True)
        assert (got == ref).all(), (name, shape)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", [(17, 15), (9, 5000)])
def test_rank_expand_epilogue(m, rng, name, shape):
    img = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    chain = f"gray,{name},expand"
    assert m._C.plan_info(chain, 3)["passes"][0]["epi_expand"]
    got = _run(m, img, chain)
    ref = m._C.golden_apply(img, chain, "reflect101", True)
    assert got.shape == ref.shape == shape + (3,)
    assert (got == ref).all()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("shape", [(33, 47), (128, 1000)])
def test_rank_chains(m, rng, chain, shape):
    img = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    got = _run(m, img, chain)
    ref = m._C.golden_apply(img, chain, "reflect101", True)
    assert (got == ref).all(), chain


@pytest.mark.parametrize("chain,iters", [("median5", 1), ("close3", 1), ("erode3", 5)])
def test_rank_local_ranks(m, chain, iters):
    """3 logical ranks on one GPU vs 1 rank, bit-identical; the iterated erode3
    runs the deep-halo schedule at its automatic depth."""
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


def test_rank_autotune_exact(m):
    C = m._C
    W, H = 2100, 256
    img = m.utils.synthetic_image(5, W, H, 3)
    cfg = m.Pipeline("median3").config(W, H, 3, "device", device=0, autotune=True)
    e = C.Engine(cfg)
    e.load_packed(np.ascontiguousarray(img))
    e.run(1)
    e.synchronize()
    bands = e.bands
    assert len(bands) == 1 and bands[0] in (0, 4, 8, 12, 16, 24, 32), bands
    assert (e.store_packed() == C.golden_apply(img, "median3", "reflect101", True)).all()


def test_rank_deterministic(m, rng):
    img = rng.integers(0, 256, size=(512, 2100, 3), dtype=np.uint8)
    a = _run(m, img, "median5")
    b = _run(m, img, "median5")
    assert a.tobytes() == b.tobytes()
