"""Every host launch path under both store policies (STRIPE_NT=0 / 1, set
in-process: it is read at every launch), on frames a few wave tiles wide: the
argument blocks (fill_tile_args), the launch descriptor of the stencil
dispatch and the LDS reservations must launch correctly whichever kernel
instance the policy picks.  Which instance runs is tests/test_launch_policy.py's
business; here the outputs must equal the golden path bit for bit, the float
paths within the bounds of tests/test_oracle_conv.py.

Shapes: 333 RGB pixels are 999 bytes, one 16-byte chunk past one 992-byte wave
tile; 997 for the 1-channel rows; 21 rows are one full 12-row band and a
partial one."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H = 21
GPU_BAND = 4e-3  # as tests/test_oracle_conv.py
BORDERS = ("reflect101", "constant")

_rng = np.random.default_rng(20260)
RGB = _rng.integers(0, 256, size=(H, 333, 3), dtype=np.uint8)
RGB_WIDE = _rng.integers(0, 256, size=(H, 997, 3), dtype=np.uint8)  # 997 gray bytes a row
GRAY = _rng.integers(0, 256, size=(H, 997), dtype=np.uint8)


def _weights(K):
    w = np.random.default_rng(K).uniform(-0.5, 1.0, (K, K))
    w[0, -1] = 0.9  # asymmetric, as tests/test_oracle_conv.py
    w /= w.sum()
    return oracle.f32_weights(w)


def _conv_chain(w):
    return f"conv:{w.shape[0]}:" + ";".join(repr(float(v)) for v in w.reshape(-1))


# name -> (chain, image): one chain per launch path
EXACT = {
    "k_sep": ("gaussian5", RGB),
    "k_sobel_rp": ("sobel", GRAY),
    "k_direct": ("emboss3", RGB),
    "k_rank": ("median3", RGB),
    "flat": ("invert", RGB),
    "gray_ref": ("gray:ref", RGB_WIDE),
    "gray_expand": ("gray,expand", RGB_WIDE),
    "k_colormix": ("sepia", RGB),
}
# name -> (K, is a blur): k_conv_small, k_blur_pl, and the two branches of the
# MFMA conv (K = 9 runs the f16 kernel, K = 13 the i8 weight-digit kernel)
FLOAT = {"k_conv_small": (3, False), "k_blur_pl": (9, True), "conv_mfma_9": (9, False), "conv_mfma_13": (13, False)}


@pytest.fixture(scope="module")
def m():
    import mpi_cuda_imagemanipulation_amd as m

    assert torch.cuda.is_available()
    return m


@pytest.fixture(scope="module")
def refs(m):
    """Golden outputs / float64 oracle sums, computed once for both policies."""
    r = {}
    for name, (chain, img) in EXACT.items():
        for border in BORDERS:
            r[name, border] = m._C.golden_apply(img, chain, border, True)
    for name, (K, blur) in FLOAT.items():
        w = oracle.blur_weights(m._C, K) if blur else _weights(K)
        for border in BORDERS:
            r[name, border] = oracle.torch_sums(RGB, w, border, device="cuda")
    return r


def _gpu(m, img, chain, border):
    x = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    y = m.ops.apply(x, chain, border)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("name", list(EXACT))
def test_exact_paths(m, refs, monkeypatch, name, border, nt):
    monkeypatch.setenv("STRIPE_NT", nt)
    chain, img = EXACT[name]
    got = _gpu(m, img, chain, border)
    ref = refs[name, border]
    assert got.shape == ref.shape
    assert (got == ref).all(), (name, border, nt, int((got != ref).sum()))


@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("name", list(FLOAT))
def test_float_paths(m, refs, monkeypatch, name, border, nt):
    monkeypatch.setenv("STRIPE_NT", nt)
    K, blur = FLOAT[name]
    chain = f"blur:{K}" if blur else _conv_chain(_weights(K))
    got = _gpu(m, RGB, chain, border)
    r = oracle.compare(got, refs[name, border], GPU_BAND)
    assert r["mismatch_outside_ties"] == 0 and r["max_diff"] <= 1, (name, border, nt, r)
    assert r["mismatch"] <= max(2, r["n"] // 2000), (name, border, nt, r)
