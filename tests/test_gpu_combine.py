"""Two-image ops on the GPU: the combine kernel (k_combine, csrc/hip/combine.hip)
against the numpy mirror of the rule table, chains with hold / swap against the
golden path, and every schedule that assumes a static two-buffer chain taking
the plain per-pass path.  Every comparison is bit-exact.

A lane moves 16 bytes, a wave's instruction 1 KiB, a workgroup 16 KiB (4
groups per lane): the row byte lengths W * C sit on those edges."""
import numpy as np
import pytest

from test_combine import CHAINS, COMBINE_TOKENS, IDENTITY_TAILS, LONG, LONG_PLAIN, mirror

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WIDTHS = {1: [1, 15, 16, 17, 1023, 1024, 1025, 16383, 16385], 3: [1, 5, 341, 342, 1365, 5462]}
BORDERS = ["reflect101", "replicate", "constant"]
# one token per kernel op, plus the saturating lincomb forms
KERNEL_TOKENS = ["add", "sub", "rsub", "absdiff", "min", "max", "lincomb:1.25:-0.75:-3.5", "lincomb:7.9:7.9",
                 "lincomb:-7.9:0:2048", "blend:0.3", "above", "above:-7", "above:255"]


@pytest.fixture(scope="module")
def m():
    import mpi_cuda_imagemanipulation_amd as m

    assert torch.cuda.is_available()
    return m


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _combine(m, x, y, op, border="reflect101"):
    out = m.ops.combine(_t(x), _t(y), op, border)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _apply(m, x, chain, border="reflect101"):
    out = m.ops.apply(_t(x), chain, border)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _engine(m, chain, W, H, cc, **kw):
    cfg = m.Pipeline(chain).config(W, H, cc, "device", device=0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return m._C.Engine(cfg)


def _checker(shape, phase=0):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    c = ((((yy + xx + phase) & 1) * 255)).astype(np.uint8)
    return c if len(shape) == 2 else np.ascontiguousarray(np.repeat(c[:, :, None], shape[2], axis=2))


def _input_pairs(rng, shape):
    r1 = rng.integers(0, 256, size=shape, dtype=np.uint8)
    r2 = rng.integers(0, 256, size=shape, dtype=np.uint8)
    zero, full = np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)
    return [(r1, r2), (zero, r2), (r1, zero), (full, r2), (r1, full), (zero, full), (full, full),
            (_checker(shape), _checker(shape, 1)), (_checker(shape), r2)]


@pytest.mark.parametrize("token", KERNEL_TOKENS)
def test_every_op_on_every_edge(m, rng, token):
    for cc, widths in WIDTHS.items():
        for W in widths:
            shape = (3, W) if cc == 1 else (3, W, cc)
            for x, h in _input_pairs(rng, shape):
                got = _combine(m, x, h, token)
                want = mirror(token, x, h)
                assert got.shape == want.shape and (got == want).all(), (token, cc, W, int((got != want).sum()))


@pytest.mark.parametrize("nt", [None, "0", "1"])
def test_all_pairs_frame(m, monkeypatch, nt):
    """x[i, j] = i, y[i, j] = j: every byte pair through the kernel, every token, both store policies."""
    if nt is None:
        monkeypatch.delenv("STRIPE_NT", raising=False)
    else:
        monkeypatch.setenv("STRIPE_NT", nt)
    x = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    y = np.ascontiguousarray(x.T)
    x3, y3 = (np.ascontiguousarray(np.repeat(a[:, :, None], 3, axis=2)) for a in (x, y))
    for token in COMBINE_TOKENS:
        assert (_combine(m, x, y, token) == mirror(token, x, y)).all(), (token, nt)
        assert (_combine(m, x3, y3, token) == mirror(token, x3, y3)).all(), (token, nt, "rgb")
    # the instances with a post table
    for chain in ("absdiff,threshold:20", "add,invert", "lincomb:-1:2,brightness:-40"):
        want = m._C.golden_apply(x3, chain, "reflect101", True, y3)
        assert (_combine(m, x3, y3, chain) == want).all(), (chain, nt)


@pytest.mark.parametrize("chain", ["hold,gaussian5,absdiff,threshold:20", "hold,box3,add,invert",
                                   "hold,invert,absdiff", "hold,gaussian5,absdiff,equalize"])
def test_folded_post_lut(m, rng, chain):
    for shape in [(9, 1025, 3), (9, 5000), (5, 17, 3)]:
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        want = m.ops.reference(img, chain)
        assert (_apply(m, img, chain) == want).all(), (chain, shape)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("chain", ["hold,gaussian5,lincomb:-1:2,gaussian7", "gradient5,box5", LONG_PLAIN, LONG])
def test_margins(m, rng, chain, border):
    """Stencils that read an image kept across passes, or a combine pass's output, see the right x-border."""
    for cc in (1, 3):
        for W in (1, 2, 3, 15, 1024, 1025):
            shape = (9, W) if cc == 1 else (9, W, cc)
            for img in (rng.integers(0, 256, size=shape, dtype=np.uint8), _checker(shape)):
                want = m.ops.reference(img, chain, border)
                got = _apply(m, img, chain, border)
                assert (got == want).all(), (chain, border, cc, W, int((got != want).sum()))


@pytest.mark.parametrize("chain", CHAINS)
def test_every_sugar(m, rng, chain):
    for shape in [(37, 1365, 3), (9, 5000)]:
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        want = m.ops.reference(img, chain)
        got = _apply(m, img, chain)
        assert got.shape == want.shape and (got == want).all(), (chain, shape, int((got != want).sum()))
        assert (_apply(m, img, chain) == got).all()  # two runs, bitwise equal


@pytest.mark.parametrize("chain", IDENTITY_TAILS)
def test_identity_tail(m, rng, chain):
    """Slot actions whose run normalised to the identity reach the engine as a copy pass."""
    for shape in [(9, 1030, 3), (5, 17, 3)]:
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        want = m.ops.reference(img, chain)
        got = _apply(m, img, chain)
        assert got.shape == want.shape and (got == want).all(), (chain, shape)


def test_wrappers_on_tensors(m, rng):
    img = rng.integers(0, 256, size=(37, 1365, 3), dtype=np.uint8)
    x = _t(img)
    assert (m.ops.unsharp_mask(x, 1.5, 3).cpu().numpy() == m.ops.unsharp_mask(img, 1.5, 3)).all()
    assert (m.ops.morph_gradient(x, 5).cpu().numpy() == m.ops.morph_gradient(img, 5)).all()
    assert (m.ops.top_hat(x).cpu().numpy() == m.ops.top_hat(img)).all()
    assert (m.ops.black_hat(x).cpu().numpy() == m.ops.black_hat(img)).all()
    assert (m.ops.adaptive_threshold(x, 5, 7).cpu().numpy() == m.ops.adaptive_threshold(img, 5, 7)).all()


def test_iterated(m, rng):
    """run(5) of unsharp against five golden applications: the held slot starts every iteration empty."""
    W, H = 1030, 67
    img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    ref = img
    for _ in range(5):
        ref = m._C.golden_apply(ref, "unsharp", "reflect101", True)
    e = _engine(m, "unsharp", W, H, 3)
    e.load_packed(img)
    e.run(5)
    assert (e.store_packed() == ref).all()


@pytest.mark.parametrize("chain,cc", [("gradient3", 3), ("gray,threshold:adaptive:5:7", 3), (LONG, 1)])
def test_local_ranks_with_an_idle_one(m, rng, chain, cc):
    W, H = 131, 2
    img = rng.integers(0, 256, size=(H, W) if cc == 1 else (H, W, cc), dtype=np.uint8)
    cfg = m.Pipeline(chain).config(W, H, cc, "device", device=0)
    ref = m._C.golden_apply(img, chain, "reflect101", True)
    assert (m._C.run_local_group(cfg, 1, img, 1) == ref).all()
    assert (m._C.run_local_group(cfg, 3, img, 1) == ref).all()
    tall = rng.integers(0, 256, size=(64, W) if cc == 1 else (64, W, cc), dtype=np.uint8)
    cfg = m.Pipeline(chain).config(W, 64, cc, "device", device=0)
    assert (m._C.run_local_group(cfg, 3, tall, 1) == m._C.golden_apply(tall, chain, "reflect101", True)).all()


def test_static_schedules_decline(m, rng):
    """graphs, deep halo, run_dist, run_e2e and run_to_host on a branched chain: each takes its plain form."""
    C = m._C
    chain, W, H = "unsharp", 1030, 96
    img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    ref = C.golden_apply(img, chain, "reflect101", True)
    ref4 = img
    for _ in range(4):
        ref4 = C.golden_apply(ref4, chain, "reflect101", True)
    # graph replay
    e = _engine(m, chain, W, H, 3, graphs=True)
    e.load_packed(img)
    e.run(4)
    assert (e.store_packed() == ref4).all() and e.graph_launches == 0
    assert e.halo_depth == 0 and not e.posts_halo
    # deep halo requested on 3 local ranks
    cfg = m.Pipeline(chain, halo_depth=4).config(W, H, 3, "device", device=0)
    assert (C.run_local_group(cfg, 3, img, 4) == ref4).all()
    # run_dist: one rank with root buffers (not the direct root -> root form), and chunked over 3 ranks
    e = _engine(m, chain, W, H, 3, root_buffers=True)
    assert not e.dist_direct and e.dist_chunks(4) == 0
    e.load_root(img)
    e.run_dist(4)
    assert (e.store_root() == ref).all()
    cfg = m.Pipeline(chain, dist_chunks=4).config(W, H, 3, "device", device=0)
    assert (C.run_local_group(cfg, 3, img, 1) == ref).all()
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
    # autotune leaves the combine pass alone
    e = _engine(m, chain, W, H, 3, autotune=True)
    e.load_packed(img)
    e.run(1)
    assert (e.store_packed() == ref).all()


def test_external_held_image(m, rng):
    C = m._C
    a = rng.integers(0, 256, size=(37, 1030, 3), dtype=np.uint8)
    b = rng.integers(0, 256, size=(37, 1030, 3), dtype=np.uint8)
    assert (m.ops.absdiff(_t(a), _t(b)).cpu().numpy() == mirror("absdiff", a, b)).all()
    assert (m.ops.blend(_t(a), _t(b), 0.25).cpu().numpy() == mirror("blend:0.25", a, b)).all()
    assert (m.ops.subtract(_t(a), _t(b)).cpu().numpy() == mirror("rsub", a, b)).all()
    g = a[:, :, 0], b[:, :, 1]
    assert (m.ops.maximum(_t(g[0]), _t(g[1])).cpu().numpy() == np.maximum(*g)).all()
    # the held image behind a swap and a stencil of its own
    ch = "gaussian3,swap,gaussian5@constant,add"
    assert (_combine(m, a, b, ch) == C.golden_apply(a, ch, "reflect101", True, b)).all()
    # iterated with the held image kept
    e = _engine(m, "blend:0.25", 1030, 37, 3, held_input=True)
    e.load_packed(a)
    e.load_held_packed(b)
    e.run(3)
    want = a
    for _ in range(3):
        want = mirror("blend:0.25", want, b)
    assert (e.store_packed() == want).all()
    # a chain that holds spends the external image: a second run needs it loaded again
    ch = "add,hold,gaussian3,add"
    e = _engine(m, ch, 1030, 37, 3, held_input=True)
    for _ in range(2):
        e.load_packed(a)
        e.load_held_packed(b)
        e.run(1)
        assert (e.store_packed() == C.golden_apply(a, ch, "reflect101", True, b)).all()
    e.load_packed(a)
    with pytest.raises(RuntimeError, match="held"):
        e.run(1)
    e = _engine(m, "hold,gaussian3,add", 1030, 37, 3, held_input=True)
    e.load_packed(a)
    e.load_held_packed(b)
    with pytest.raises(RuntimeError, match="hold or swap"):
        e.run(2)
