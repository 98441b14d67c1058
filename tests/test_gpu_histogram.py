"""The histogram kernel (k_hist, csrc/hip/histogram.hip) and the statistic ops on
the GPU: counts against np.bincount, chains bit-exact against the golden path,
and every schedule that assumes a static chain falling back to the plain
per-pass path.  A wave reads 16 bytes per lane (1 KiB per instruction) and
4 KiB per step; the row lengths sit on those edges."""
import threading

import numpy as np
import pytest

from test_histogram import CHAINS, chain_image, half_dark, mirror_chain, np_hist

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# row bytes W * C of 1, 15, 16, 17, 1023, 1024, 1025 and 3073 (gray), and the
# nearest RGB widths on both sides of the same edges (3, 15, 18, 1023, 1026,
# 3072 and 3075 bytes: group starts in all three channel phases)
WIDTHS = {1: [1, 15, 16, 17, 1023, 1024, 1025, 3073], 3: [1, 5, 6, 341, 342, 1024, 1025]}
HEIGHTS = [1, 2, 33, 257]


@pytest.fixture(scope="module")
def m():
    import mpi_cuda_imagemanipulation_amd as m

    assert torch.cuda.is_available()
    return m


def _hist(m, img):
    return m.ops.histogram(torch.from_numpy(np.ascontiguousarray(img)).cuda())


def _engine(m, chain, W, H, cc, **kw):
    cfg = m.Pipeline(chain).config(W, H, cc, "device", device=0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return m._C.Engine(cfg)


@pytest.mark.parametrize("cc", [1, 3])
@pytest.mark.parametrize("H", HEIGHTS)
def test_histogram_equals_bincount(m, rng, cc, H):
    for W in WIDTHS[cc]:
        shape = (H, W) if cc == 1 else (H, W, cc)
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        got = _hist(m, img)
        assert got.dtype == np.int64 and got.shape == (cc, 256)
        assert (got == np_hist(img)).all(), (cc, H, W)
        last = np.zeros(shape, np.uint8)  # only the last pixel of the last row is not zero
        last[-1, -1] = 201 if cc == 1 else (7, 8, 9)
        assert (_hist(m, last) == np_hist(last)).all(), (cc, H, W)


@pytest.mark.parametrize("cc", [1, 3])
def test_flat_frames(m, cc):
    """All 64 lanes on one bin, and a bin beyond 65535."""
    shape = (300, 300) if cc == 1 else (300, 300, 3)
    for v in (0, 255):
        img = np.full(shape, v, np.uint8)
        got = _hist(m, img)
        assert (got == np_hist(img)).all() and int(got[0, v]) == 90000


def test_batch_and_determinism(m, rng):
    x = rng.integers(0, 256, size=(3, 33, 1030, 3), dtype=np.uint8)
    t = torch.from_numpy(x).cuda()
    a, b = m.ops.histogram(t), m.ops.histogram(t)
    assert a.shape == (3, 3, 256) and (a == b).all()
    for i in range(3):
        assert (a[i] == np_hist(x[i])).all()
    assert m.ops.otsu_level(t[0]) == m.ops.otsu_level(x[0])


@pytest.mark.parametrize("cc,W", [(3, 1030), (1, 1025), (3, 5), (1, 17)])
def test_margins_and_padding_are_not_counted(m, rng, cc, W):
    """After a gaussian5 step the x-margins of the output hold reflected pixel
    copies and the bytes up to the pitch whatever the kernels stored there."""
    H = 37
    shape = (H, W) if cc == 1 else (H, W, cc)
    for img in (rng.integers(0, 256, size=shape, dtype=np.uint8), np.full(shape, 255, np.uint8)):
        e = _engine(m, "gaussian5", W, H, cc)
        e.load_packed(np.ascontiguousarray(img))
        assert (e.histogram(False) == np_hist(img)).all()  # the loaded input (its margins are filled too)
        e.run(1)
        ref = m._C.golden_apply(img, "gaussian5", "reflect101", True)
        assert (e.histogram(False) == np_hist(ref)).all()
        assert (e.histogram(True) == np_hist(ref)).all()  # one rank: no communication


def test_engine_histogram_local_ranks(m):
    """3 `local` ranks sharing the GPU over a 2-row frame (one rank idle): the
    local counts sum to the global ones, which every rank receives."""
    C = m._C
    img = half_dark(2, 1030, 3)
    comms = C.make_local_comms(3, True)
    res, errs = {}, []

    def body(r):
        try:
            cfg = m.Pipeline("invert").config(1030, 2, 3, "device", device=0)
            e = C.Engine(cfg, comms[r])
            row0, rows = e.stripe
            e.load_packed(np.ascontiguousarray(img[row0:row0 + rows]))
            res[r] = (rows, e.histogram(False), e.histogram(True))
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
            comms[r].abort(str(ex))

    th = [threading.Thread(target=body, args=(r,)) for r in range(3)]
    [t.start() for t in th]
    [t.join(120) for t in th]
    assert not errs, errs
    ref = np_hist(img)
    assert sorted(res[r][0] for r in range(3)) == [0, 1, 1]
    assert (sum(res[r][1] for r in range(3)) == ref).all()
    one = _engine(m, "invert", 1030, 2, 3)
    one.load_packed(np.ascontiguousarray(img))
    assert (one.histogram(True) == ref).all()
    for r in range(3):
        assert (res[r][2] == ref).all(), r


def _run(m, img, chain, border="reflect101"):
    y = m.ops.apply(torch.from_numpy(np.ascontiguousarray(img)).cuda(), chain, border)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("chain", CHAINS)
def test_chains_exact(m, rng, chain):
    imgs = [chain_image(3), (rng.normal(100, 40, size=(67, 1030, 3))).clip(0, 255).astype(np.uint8)]
    for img in imgs:
        ref = m.ops.reference(img, chain)
        got = _run(m, img, chain)
        assert got.shape == ref.shape and (got == ref).all(), (chain, img.shape, int((got != ref).sum()))
    assert (ref == mirror_chain(m._C, imgs[1], chain)).all()  # and the golden path is the mirror's


def test_wrappers_on_tensors(m):
    img = chain_image(3)
    x = torch.from_numpy(img).cuda()
    assert (m.ops.equalize(x).cpu().numpy() == m.ops.equalize(img)).all()
    assert (m.ops.autocontrast(x, 1.0).cpu().numpy() == m.ops.autocontrast(img, 1.0)).all()
    assert (m.ops.threshold_otsu(x).cpu().numpy() == m.ops.threshold_otsu(img)).all()


@pytest.mark.parametrize("ranks", [2, 3, 8])
def test_local_ranks_equal_one_rank(m, ranks):
    chain = "gray,equalize,gaussian5"
    img = half_dark(64, 131, 3)
    cfg = m.Pipeline(chain).config(131, 64, 3, "device", device=0)
    got = m._C.run_local_group(cfg, ranks, img, 1)
    ref = m._C.golden_apply(img, chain, "reflect101", True)
    assert (got == ref).all()
    assert (got == m._C.run_local_group(cfg, 1, img, 1)).all()


def test_local_ranks_iterated(m):
    """run(3) on 3 ranks: a static chain would take the deep halo here."""
    chain = "equalize,gaussian3"
    img = half_dark(96, 131, 3)
    ref = img
    for _ in range(3):
        ref = m._C.golden_apply(ref, chain, "reflect101", True)
    got = m._C.run_local_group(m.Pipeline(chain).config(131, 96, 3, "device", device=0), 3, img, 3)
    assert (got == ref).all()


def test_static_schedules_decline(m):
    """graphs, autotune, run_dist, run_e2e and run_to_host on a data-dependent
    single-pass chain: each takes its plain form and equals golden."""
    C = m._C
    chain, W, H = "equalize,gaussian5", 1030, 67
    assert len(C.plan_info(chain, 3)["passes"]) == 1
    img = half_dark(H, W, 3)
    ref = C.golden_apply(img, chain, "reflect101", True)
    ref6 = img
    for _ in range(6):
        ref6 = C.golden_apply(ref6, chain, "reflect101", True)
    # graph replay
    e = _engine(m, chain, W, H, 3, graphs=True)
    e.load_packed(img)
    e.run(6)
    assert (e.store_packed() == ref6).all() and e.graph_launches == 0
    # autotune: times the pass with the static table, no collective
    e = _engine(m, chain, W, H, 3, autotune=True)
    e.load_packed(img)
    e.run(1)
    assert (e.store_packed() == ref).all()
    assert e.halo_depth == 0 and not e.posts_halo
    # run_dist on one rank with root buffers: not the direct root -> root form
    e = _engine(m, chain, W, H, 3, root_buffers=True)
    assert not e.dist_direct and e.dist_chunks(4) == 0
    e.load_root(img)
    e.run_dist(4)
    assert (e.store_root() == ref).all()
    # e2e: upload all, run, download all
    e = _engine(m, chain, W, H, 3)
    e.alloc_host_io()
    e.host_input()[...] = img
    e.run_e2e(4)
    e.synchronize()
    assert (e.host_output() == ref).all()
    # run_to_host
    e = _engine(m, chain, W, H, 3)
    e.load_packed(img)
    host = torch.empty(H * W * 3, dtype=torch.uint8, pin_memory=True)
    e.run_to_host_ptr(host.data_ptr(), 4)
    e.synchronize()
    assert (host.numpy().reshape(H, W, 3) == ref).all()


def test_self_halo(m):
    """With self_halo the stripe is a vertically periodic frame: the table is of
    the stripe's own pixels, the stencil reads the exchanged rows."""
    import os

    from test_r6_selfhalo import torus_golden

    from mpi_cuda_imagemanipulation_amd import parallel
    from mpi_cuda_imagemanipulation_amd.models import Pipeline

    saved = {k: os.environ.pop(k) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK") if k in os.environ}
    try:
        ctx = parallel.init("rccl")
    finally:
        os.environ.update(saved)
    W, H = 517, 96
    img = m._C.synth_rows(11, W, 3, 0, H)
    d = parallel.DistributedPipeline(ctx, Pipeline("equalize,gaussian5", halo_depth=1, self_halo=True), W, H, 3)
    assert d.engine.self_halo
    d.load_synthetic(11)
    d.run(1)
    d.synchronize()
    lut = np.array(m._C.stat_lut("equalize", np_hist(img)), dtype=np.uint8)
    assert (d.result_stripe() == torus_golden(lut[img], "gaussian5", 1)).all()
