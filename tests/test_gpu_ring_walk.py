"""The register-ring row walk, in both its copies (k_direct's own body and
ring_task, which k_rank wraps: csrc/hip/stencil_kernels.h), under forced band
heights and both store policies (the nt-store instances, SAUX = kNtAux, are otherwise picked for large frames
only), bit-exact against the golden path.

Frame 1000 x 23: a gray row is 1000 bytes, one full 992-byte wave tile plus an
8-byte last tile that tile_base starts early; an RGB row is 3000 bytes, four
tiles.  23 rows are no multiple of K = 3, K = 5 or either band, so the last
unrolled round and the last band are partial.  The chains cover both
bodies at C = 1 and C = 3, the LUT prologue with an epilogue LUT, and the
gray-LUT / gray prologues with the expand epilogue."""
import pytest

import mpi_cuda_imagemanipulation_amd as m

C = m._C
W, H = 1000, 23

CASES = [(f, Cc) for f in ("emboss5", "sharpen", "median3", "erode5") for Cc in (1, 3)] + [
    ("brightness:10,emboss3,invert", 3),
    ("gray:ref,contrast:3.5,emboss3,expand", 3),
    ("gray,median3,expand", 3),
]


@pytest.mark.gpu
@pytest.mark.parametrize("border", ["reflect101", "skip"])
@pytest.mark.parametrize("chain,Cc", CASES)
def test_ring_walk_bands_nt_exact_gpu(chain, Cc, border):
    img = C.synth_rows(11, W, Cc, 0, H)
    ref = C.golden_apply(img, chain, border, True)
    pipe = m.models.Pipeline(chain, border=border)
    n = len(C.Engine(pipe.config(W, H, Cc, "device", device=0)).bands)
    for band in (4, 8):
        for nt in (0, 1):
            e = C.Engine(pipe.config(W, H, Cc, "device", device=0))
            e.set_tuning([band] * n, [-1] * n, [nt] * n, [0] * n)
            e.load_synthetic(11)
            e.run(1)
            assert (e.store_packed() == ref).all(), (chain, Cc, border, band, nt)
