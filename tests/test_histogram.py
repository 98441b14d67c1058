"""Histogram, the statistic ops (equalize, autocontrast[:P], threshold:otsu) and
their chain / engine plumbing on the CPU.

The mirrors of the three table rules below are written from the specification
(csrc/include/stripe/filters.h) with Python integers and, for Otsu, exact
rationals: nothing expected here is computed by the code under test.
"""
import json
import os
import socket
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# mirrors
# ---------------------------------------------------------------------------
def np_hist(img):
    """(C, 256) int64 counts by np.bincount."""
    a = img if img.ndim == 3 else img[:, :, None]
    return np.stack([np.bincount(a[:, :, c].reshape(-1), minlength=256) for c in range(a.shape[2])]).astype(np.int64)


def pooled(hist):
    h = np.asarray(hist, dtype=object)
    h = h.reshape(-1, 256)
    return [int(sum(int(h[c][v]) for c in range(h.shape[0]))) for v in range(256)]


def cdf_of(h):
    out, n = [], 0
    for v in range(256):
        n += h[v]
        out.append(n)
    return out


def mirror_equalize(hist):
    h = pooled(hist)
    N, cdf = sum(h), cdf_of(h)
    if N == 0:
        return list(range(256))
    v0 = next(v for v in range(256) if h[v] > 0)
    c0 = h[v0]
    D = N - c0
    if D == 0:
        return list(range(256))
    return [0 if v < v0 else min(255, (510 * (cdf[v] - c0) + D) // (2 * D)) for v in range(256)]


def mirror_autocontrast(hist, P):
    h = pooled(hist)
    N, cdf = sum(h), cdf_of(h)
    Pq = int(np.rint(100.0 * P))  # nearbyint: ties to even
    cut = N * Pq // 10000
    if N == 0:
        return list(range(256))
    lo = next(v for v in range(256) if cdf[v] > cut)
    hi = max(v for v in range(256) if N - (cdf[v - 1] if v > 0 else 0) > cut)
    if hi <= lo:
        return list(range(256))
    d = hi - lo
    return [0 if v <= lo else 255 if v >= hi else (510 * (v - lo) + d) // (2 * d) for v in range(256)]


def otsu_g(hist):
    """g(t) for t = 1..255 as exact rationals (index t; g[0] unused)."""
    h = pooled(hist)
    N = sum(h)
    S = sum(v * h[v] for v in range(256))
    g = [Fraction(0)] * 256
    n0 = S0 = 0
    for t in range(1, 256):
        n0 += h[t - 1]
        S0 += (t - 1) * h[t - 1]
        n1 = N - n0
        if n0 and n1:
            a = S0 * N - n0 * S
            g[t] = Fraction(a * a, n0 * n1)
    return g


def mirror_otsu_level(hist):
    g = otsu_g(hist)
    best = max(g[1:])
    return next(t for t in range(1, 256) if g[t] == best)


def otsu_gap(hist):
    """Relative gap between the best and the second-best DISTINCT g (None: all equal)."""
    vals = sorted(set(otsu_g(hist)[1:]), reverse=True)
    if len(vals) < 2 or vals[0] == 0:
        return None
    return float((vals[0] - vals[1]) / vals[0])


def mirror_otsu(hist):
    T = mirror_otsu_level(hist)
    return [255 if v >= T else 0 for v in range(256)]


def mirror_lut(token, hist):
    if token == "equalize":
        return mirror_equalize(hist)
    if token == "threshold:otsu":
        return mirror_otsu(hist)
    assert token.startswith("autocontrast")
    return mirror_autocontrast(hist, float(token.split(":")[1]) if ":" in token else 0.0)


def mirror_chain(C, img, chain, border="reflect101"):
    """The chain op by op: statistic ops through the mirrors above (histogram by
    np.bincount of the intermediate image), every other op through the golden
    path of that single op (covered by the existing suites)."""
    cur = img
    for tok in C.parse_chain(chain).split(","):
        if tok in ("equalize", "threshold:otsu") or tok.startswith("autocontrast"):
            lut = np.array(mirror_lut(tok, np_hist(cur)), dtype=np.uint8)
            cur = lut[cur]
        else:
            cur = C.golden_apply(np.ascontiguousarray(cur), tok, border, True)
    return cur


def frames(rng, H, W, C):
    shape = (H, W) if C == 1 else (H, W, C)
    two = np.where(rng.integers(0, 2, size=shape) > 0, 200, 10).astype(np.uint8)
    ramp = (np.arange(H * W * C, dtype=np.int64) % 256).astype(np.uint8).reshape(shape)
    return {
        "random": rng.integers(0, 256, size=shape, dtype=np.uint8),
        "zeros": np.zeros(shape, np.uint8),
        "full": np.full(shape, 255, np.uint8),
        "two": two,
        "ramp": ramp,
    }


SHAPES = [(1, 1), (1, 7), (7, 1), (13, 5), (97, 131), (64, 341)]  # (H, W)


# ---------------------------------------------------------------------------
# histogram
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cc", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_golden_and_cpu_histogram_equal_bincount(C, rng, cc, shape):
    H, W = shape
    for name, img in frames(rng, H, W, cc).items():
        ref = np_hist(img)
        g = C.golden_histogram(img)
        c = C.cpu_histogram(img)
        assert g.dtype == np.int64 and g.shape == (cc, 256), name
        assert (g == ref).all() and (c == ref).all(), name
        assert int(g.sum()) == W * H * cc


HIST_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import mpi_cuda_imagemanipulation_amd as m
C = m._C
rng = np.random.default_rng(7)
out = {}
for (H, W, cc) in json.loads(sys.argv[2]):
    shape = (H, W) if cc == 1 else (H, W, cc)
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    a = img if cc == 3 else img[:, :, None]
    ref = np.stack([np.bincount(a[:, :, c].reshape(-1), minlength=256) for c in range(cc)])
    got = C.cpu_histogram(img)       # threads from STRIPE_CPU_THREADS
    gold = C.golden_histogram(img)
    out["%dx%dx%d" % (H, W, cc)] = bool((got == ref).all() and (gold == ref).all() and got.sum() == H * W * cc)
print(json.dumps(out))
"""


def test_cpu_histogram_thread_counts():
    """STRIPE_CPU_THREADS = 1 and 3, each in a child of its own (the variable may
    be cached per process).  The 1500x600 frames are large enough for the row
    blocks to go to three threads."""
    shapes = [(97, 131, 3), (64, 341, 1), (600, 1500, 3), (600, 1500, 1)]
    procs = {}
    for n in ("1", "3"):
        env = {k: v for k, v in os.environ.items() if not k.startswith("STRIPE_")}
        env["STRIPE_CPU_THREADS"] = n
        procs[n] = subprocess.Popen([sys.executable, "-c", HIST_CHILD, ROOT, json.dumps(shapes)], cwd=ROOT, env=env,
                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for n, p in procs.items():
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, se
        res = json.loads(so.strip().splitlines()[-1])
        assert len(res) == len(shapes) and all(res.values()), (n, res)


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------
def table_histograms(rng):
    big = np.zeros((3, 256), np.int64)  # N = 3 * 2^30, built as an array: u64 arithmetic
    w = rng.integers(1, 1000, size=(3, 256)).astype(np.int64)
    for c in range(3):
        big[c] = w[c] * (2 ** 30 // int(w[c].sum()))
        big[c, 17 * (c + 1)] += 2 ** 30 - int(big[c].sum())
    assert int(big.sum()) == 3 * 2 ** 30

    def only(v, n=1000):
        h = np.zeros(256, np.int64)
        h[v] = n
        return h

    two = np.zeros(256, np.int64)
    two[10], two[200] = 700, 300
    narrow = np.zeros(256, np.int64)  # almost everything on one level: hi <= lo once the ends are clipped
    narrow[99], narrow[100], narrow[101] = 1, 10000, 1
    return {
        "random_gray": np_hist(rng.integers(0, 256, size=(97, 131), dtype=np.uint8)),
        "random_rgb": np_hist(rng.integers(0, 256, size=(97, 131, 3), dtype=np.uint8)),
        "one_level": only(77),
        "two_levels": two,
        "only_0": only(0),
        "only_255": only(255),
        "big": big,
        "narrow": narrow,
    }


TOKENS = ["equalize", "threshold:otsu", "autocontrast", "autocontrast:1", "autocontrast:2.5", "autocontrast:49.99"]


@pytest.mark.parametrize("token", TOKENS)
def test_stat_lut_equals_mirror(C, rng, token):
    for name, h in table_histograms(rng).items():
        got = list(C.stat_lut(token, h))
        assert got == mirror_lut(token, h), (token, name)


def test_stat_lut_special_cases(C, rng):
    hs = table_histograms(rng)
    ident = list(range(256))
    assert list(C.stat_lut("equalize", hs["one_level"])) == ident
    assert list(C.stat_lut("autocontrast", hs["one_level"])) == ident
    assert C.otsu_level(hs["one_level"]) == 1
    assert C.otsu_level(hs["only_0"]) == 1 and C.otsu_level(hs["only_255"]) == 1
    # two levels 10 / 200: g is the same for every t in 11..200, the smallest wins
    g = otsu_g(hs["two_levels"])
    assert len({g[t] for t in range(11, 201)}) == 1 and g[11] > 0 and g[10] == 0 and g[201] == 0
    assert C.otsu_level(hs["two_levels"]) == 11
    # hi <= lo: clipping 1 % per end of the narrow histogram leaves one level
    assert mirror_autocontrast(hs["narrow"], 1.0) == ident
    assert list(C.stat_lut("autocontrast:1", hs["narrow"])) == ident
    assert list(C.stat_lut("autocontrast", hs["narrow"])) != ident
    # equalize on a random frame is the float64 rounding of the OpenCV rule
    h = pooled(hs["random_gray"])
    cdf = np.cumsum(np.array(h, dtype=np.float64))
    v0 = next(v for v in range(256) if h[v])
    ref = np.rint((cdf - h[v0]) * 255.0 / (cdf[-1] - h[v0])).clip(0, 255).astype(int)
    ref[:v0] = 0
    assert list(C.stat_lut("equalize", hs["random_gray"])) == list(ref)


def otsu_inputs(rng):
    r = np.random.default_rng(1234)
    uni = r.integers(0, 256, size=(97, 131), dtype=np.uint8)
    bim = np.where(r.integers(0, 2, size=(97, 131)) > 0, r.normal(70, 12, (97, 131)), r.normal(180, 20, (97, 131)))
    bim = bim.clip(0, 255).astype(np.uint8)
    ramp = (np.arange(97 * 131) % 256).astype(np.uint8).reshape(97, 131)
    hs = table_histograms(rng)
    return {"uniform": np_hist(uni), "bimodal": np_hist(bim), "ramp": np_hist(ramp), "two_levels": hs["two_levels"],
            "big": hs["big"], "random_rgb": hs["random_rgb"]}


def test_otsu_level_equals_exact_mirror(C, rng):
    """C.otsu_level evaluates g in double; the mirror in exact rationals.  They
    must agree wherever the double evaluation cannot reorder the candidates:
    the best and second-best distinct g differ by a relative gap above 1e-9 (a
    double product chain errs by a few 1e-16), or the maximum is an exact tie
    of identical terms, resolved by "smallest t".  No input may be excluded."""
    excluded = 0
    for name, h in otsu_inputs(rng).items():
        gap = otsu_gap(h)
        print(name, "gap", gap)
        if gap is not None and gap <= 1e-9:
            excluded += 1
            continue
        assert C.otsu_level(h) == mirror_otsu_level(h), name
    assert excluded == 0


# ---------------------------------------------------------------------------
# parser and chain compiler
# ---------------------------------------------------------------------------
def test_parse_and_round_trip(C):
    for tok, canon in [("equalize", "equalize"), ("autocontrast", "autocontrast"), ("autocontrast:0", "autocontrast"),
                       ("autocontrast:2.5", "autocontrast:2.5"), ("autocontrast:49.99", "autocontrast:49.99"),
                       ("threshold:otsu", "threshold:otsu"), ("threshold:128", "threshold:128")]:
        assert C.parse_chain(tok) == canon
        assert C.parse_chain(C.parse_chain(tok)) == canon
    chain = "gray,median3,threshold:otsu,open3,expand"
    assert C.parse_chain(C.parse_chain(chain)) == C.parse_chain(chain)


@pytest.mark.parametrize("bad", ["autocontrast:50", "autocontrast:-1", "threshold:otsu:1", "equalize@replicate",
                                 "equalize:3", "autocontrast:1:2", "threshold:otsu@constant"])
def test_parse_refuses(C, bad):
    with pytest.raises(RuntimeError):
        C.parse_chain(bad)


def test_plan_structure(C):
    info = C.plan_info("equalize,gaussian5", 3)
    assert info["data_dependent"] and len(info["passes"]) == 1
    p = info["passes"][0]
    assert p["kind"] == 1 and p["stat"] == "equalize" and "prologue[stat:equalize,lut]" in p["desc"]
    # a run-time table counts as moving the zero pixel: a pass of its own under a constant border
    info = C.plan_info("equalize,gaussian5@constant", 3)
    assert [q["kind"] for q in info["passes"]] == [0, 1]
    assert info["passes"][0]["stat"] == "equalize" and info["passes"][1]["stat"] == ""
    assert len(C.plan_info("equalize,gaussian5", 3, "constant")["passes"]) == 2
    # never an epilogue: its histogram is of that pass's output
    info = C.plan_info("gaussian5,equalize", 3)
    assert [q["kind"] for q in info["passes"]] == [1, 0]
    assert info["passes"][0]["stat"] == "" and not info["passes"][0]["epi_lut"]
    assert info["passes"][1]["stat"] == "equalize"
    # the pending run is flushed first, exactly as a chain's tail: here as the stencil's epilogue
    info = C.plan_info("gaussian5,invert,equalize,invert", 3)
    assert [q["kind"] for q in info["passes"]] == [1, 0] and info["passes"][0]["epi_lut"]
    info = C.plan_info("gray,equalize", 3)
    assert [(q["kind"], q["cin"], q["cout"], q["stat"]) for q in info["passes"]] == [(0, 3, 1, ""), (0, 1, 1, "equalize")]
    assert info["passes"][1]["desc"].startswith("pointwise[stat:equalize")
    # later static ops compose onto it; two statistic ops are two passes
    assert len(C.plan_info("equalize,invert,brightness:3,gaussian5", 3)["passes"]) == 1
    assert len(C.plan_info("equalize,equalize", 3)["passes"]) == 2
    assert not C.plan_info("gaussian5,invert", 3)["data_dependent"]
    assert "stat:otsu" in C.describe_chain("threshold:otsu", 1)


# ---------------------------------------------------------------------------
# chain equivalence
# ---------------------------------------------------------------------------
CHAINS = [
    "equalize",
    "gray,equalize,expand",
    "equalize,gaussian5",
    "gaussian5,equalize,invert",
    "brightness:40,autocontrast:1,sobel",
    "gray,median3,threshold:otsu,open3,expand",
    "equalize,equalize",
    "invert,equalize,gaussian5@constant",
]


def chain_image(cc):
    """Structured and skewed (not flat-histogram) so every table is far from the identity."""
    r = np.random.default_rng(99 + cc)
    H, W = (97, 131) if cc == 3 else (53, 40)
    shape = (H, W) if cc == 1 else (H, W, cc)
    x = (r.normal(90, 35, size=shape) + np.linspace(0, 60, W).reshape((1, W) + (1,) * (cc == 3))).clip(0, 255)
    return x.astype(np.uint8)


@pytest.fixture(scope="module")
def chain_refs():
    """The mirror result of every (chain, channels) case, computed once."""
    import mpi_cuda_imagemanipulation_amd as m

    refs = {}
    for cc in (3, 1):
        img = chain_image(cc)
        for chain in CHAINS:
            if cc == 1 and "expand" in chain and not chain.startswith("gray"):
                continue
            refs[(chain, cc)] = (img, mirror_chain(m._C, img, chain))
    return refs


@pytest.mark.parametrize("cc", [3, 1])
@pytest.mark.parametrize("chain", CHAINS)
def test_chain_equals_mirror(C, chain_refs, chain, cc):
    img, ref = chain_refs[(chain, cc)]
    assert ref.shape != img.shape or not (ref == img).all()  # the chain does something to this image
    for name, got in [("golden fused", C.golden_apply(img, chain, "reflect101", True)),
                      ("golden unfused plan", C.golden_apply(img, chain, "reflect101", False)),
                      ("golden op by op", C.golden_apply_unfused(img, chain, "reflect101")),
                      ("cpu", C.cpu_apply(img, chain, "reflect101", True)),
                      ("cpu 3 threads", C.cpu_apply(img, chain, "reflect101", True, 3))]:
        assert got.shape == ref.shape and (got == ref).all(), (chain, cc, name)


def test_iterated_recomputes_the_table(C):
    """run(n > 1) recomputes the table every iteration, as golden iterated does."""
    import mpi_cuda_imagemanipulation_amd as m

    img = chain_image(3)
    ref = img
    for _ in range(3):
        ref = mirror_chain(C, ref, "equalize,gaussian3")
    got = m.models.Pipeline("equalize,gaussian3").run_distributed(img, 1, backend="host", iterations=3)
    assert (got == ref).all()


# ---------------------------------------------------------------------------
# host-backend distributed runs
# ---------------------------------------------------------------------------
def half_dark(H, W, cc, seed=5):
    """Upper half dark, lower half bright: a stripe-local table differs visibly from the global one."""
    r = np.random.default_rng(seed)
    shape = (H, W) if cc == 1 else (H, W, cc)
    img = r.integers(0, 60, size=shape, dtype=np.uint8)
    img[H // 2:] = r.integers(150, 256, size=img[H // 2:].shape, dtype=np.uint8)
    return img


DIST_CHAINS = ["gray,equalize,gaussian5", "threshold:otsu"]


def test_half_dark_frame_can_catch_a_missing_all_reduce(C):
    """In the mirror, the stripe-local result of the half-dark frame differs from the global one."""
    img = half_dark(64, 48, 3)
    for chain in DIST_CHAINS:
        glob = mirror_chain(C, img, chain)
        local = np.concatenate([mirror_chain(C, img[:32], chain), mirror_chain(C, img[32:], chain)])
        assert (glob != local).mean() > 0.05, chain


@pytest.mark.parametrize("chain", DIST_CHAINS)
@pytest.mark.parametrize("ranks", [1, 2, 3, 5])
def test_host_ranks_equal_one_rank_golden(C, chain, ranks):
    import mpi_cuda_imagemanipulation_amd as m

    img = half_dark(64, 48, 3)
    ref = mirror_chain(C, img, chain)
    assert (C.golden_apply(img, chain, "reflect101", True) == ref).all()
    got = m.models.Pipeline(chain).run_distributed(img, ranks, backend="host")
    assert got.shape == ref.shape and (got == ref).all(), (chain, ranks)


@pytest.mark.parametrize("chain", DIST_CHAINS)
def test_host_ranks_with_idle_ranks(C, chain):
    """A 64x5 frame on 8 ranks: some ranks own no rows and take no part in the all-reduce."""
    import mpi_cuda_imagemanipulation_amd as m

    img = half_dark(5, 64, 3)
    parts, active = C.plan_rows(5, 8, max(1, C.plan_info(chain, 3)["max_radius"]), False)
    assert active < 8 and any(rows == 0 for _, rows in parts)
    ref = mirror_chain(C, img, chain)
    got = m.models.Pipeline(chain).run_distributed(img, 8, backend="host")
    assert (got == ref).all()


def test_host_ranks_iterated_and_legacy(C):
    import mpi_cuda_imagemanipulation_amd as m

    img = half_dark(64, 48, 3)
    ref = img
    for _ in range(3):
        ref = mirror_chain(C, ref, "equalize,gaussian3")
    got = m.models.Pipeline("equalize,gaussian3").run_distributed(img, 3, backend="host", iterations=3)
    assert (got == ref).all()
    # a legacy partition drops H mod N rows: the histogram covers the rows it keeps
    pipe = m.models.Pipeline("equalize", legacy_partition=True)
    got = pipe.run_distributed(img[:62], 4, backend="host")
    assert (got[:60] == mirror_chain(C, img[:60], "equalize")).all()


def test_engine_histogram_host_ranks(C):
    """Engine.histogram on 3 host ranks (one thread each) over a 2-row frame: one
    rank is idle.  The local counts sum to the global ones, which every rank,
    the idle one included, receives."""
    import threading

    img = half_dark(2, 37, 3)
    comms = C.make_local_comms(3, False)
    res, errs = {}, []

    def body(r):
        try:
            cfg = C.EngineConfig()
            cfg.W, cfg.H, cfg.C, cfg.chain, cfg.backend = 37, 2, 3, "invert", C.Backend.host
            e = C.Engine(cfg, comms[r])
            row0, rows = e.stripe
            e.load_packed(np.ascontiguousarray(img[row0:row0 + rows]))
            res[r] = (rows, e.histogram(False), e.histogram(True))
            e.run(1)  # ...and of the last run()'s output
            res[r] += (e.histogram(True),)
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
    for r in range(3):
        assert (res[r][2] == ref).all(), r
        assert (res[r][3] == np_hist(255 - img)).all(), r


GLOO_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["STRIPE_ROOT"])
import torch.distributed as dist
from mpi_cuda_imagemanipulation_amd import parallel, models
ctx = parallel.init("gloo")
img = np.load(os.environ["IN"])
H, W = img.shape[:2]
dp = parallel.DistributedPipeline(ctx, models.Pipeline(os.environ["CHAIN"]), W, H, 3, root_buffers=True)
dp.load_root(img)
dp.scatter()
dp.run(1)
dp.gather()
out = dp.result_root()
h = dp.engine.histogram(True)
if ctx.rank == 0:
    np.save(os.environ["OUT"], out)
    np.save(os.environ["OUT"] + ".hist.npy", h)
dist.barrier()
dist.destroy_process_group()
'''


def test_gloo_two_processes(tmp_path, C):
    """One process per rank over gloo (the callback communicator), world size 2."""
    chain = "gray,equalize,gaussian5"
    img = half_dark(64, 48, 3)
    src, out = tmp_path / "in.npy", tmp_path / "out.npy"
    np.save(src, img)
    script = tmp_path / "worker.py"
    script.write_text(GLOO_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), STRIPE_ROOT=ROOT, CHAIN=chain, IN=str(src), OUT=str(out),
                   CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        o, _ = p.communicate(timeout=240)
        logs.append(o.decode(errors="replace"))
        assert p.returncode == 0, "\n".join(logs)
    ref = mirror_chain(C, img, chain)
    assert (np.load(out) == ref).all()
    assert (np.load(str(out) + ".hist.npy") == np_hist(ref)).all()


def test_cli_ranks_agree(tmp_path, C):
    """bin/stripe run on 3 host ranks writes the same file as on 1."""
    import mpi_cuda_imagemanipulation_amd as m

    exe = os.path.join(ROOT, "bin", "stripe")
    assert os.path.exists(exe), "bin/stripe is built with the extension"
    img = half_dark(64, 48, 3)
    src = tmp_path / "in.ppm"
    m.utils.write_image(str(src), img)
    outs = []
    for n in (1, 3):
        dst = tmp_path / f"out{n}.ppm"
        r = subprocess.run([exe, "run", "--input", str(src), "--output", str(dst), "--chain",
                            "gray,equalize,threshold:otsu,expand", "--ranks", str(n), "--backend", "host"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(dst.read_bytes())
    assert outs[0] == outs[1]
    assert (m.utils.read_image(str(tmp_path / "out3.ppm")) ==
            mirror_chain(C, img, "gray,equalize,threshold:otsu,expand")).all()


# ---------------------------------------------------------------------------
# Python API
# ---------------------------------------------------------------------------
def test_ops_histogram_numpy(rng):
    import torch

    import mpi_cuda_imagemanipulation_amd as m

    rgb = rng.integers(0, 256, size=(33, 41, 3), dtype=np.uint8)
    gray = rng.integers(0, 256, size=(33, 41), dtype=np.uint8)
    h = m.ops.histogram(rgb)
    assert h.dtype == np.int64 and h.shape == (3, 256) and (h == np_hist(rgb)).all()
    assert (m.ops.histogram(gray) == np_hist(gray)).all() and m.ops.histogram(gray).shape == (1, 256)
    assert (m.ops.histogram(torch.from_numpy(rgb)) == np_hist(rgb)).all()
    batch = rng.integers(0, 256, size=(4, 9, 11, 3), dtype=np.uint8)
    hb = m.ops.histogram(batch)
    assert hb.shape == (4, 3, 256) and all((hb[b] == np_hist(batch[b])).all() for b in range(4))
    assert m.ops.histogram(batch[:, :, :, :1]).shape == (4, 1, 256)
    with pytest.raises(TypeError):
        m.ops.histogram(rgb.astype(np.int32))


def test_ops_wrappers_and_catalogue(C):
    import mpi_cuda_imagemanipulation_amd as m

    for fn in ("histogram", "equalize", "autocontrast", "threshold_otsu", "otsu_level"):
        assert fn in m.ops.__all__ and callable(getattr(m.ops, fn))
    for tok in ("equalize", "autocontrast[:P]", "threshold:otsu"):
        assert tok in m.ops.FILTERS
    assert "pooled" in " ".join(m.ops.FILTERS.values()) or "pooled" in open(m.ops.__file__).read()
    img = chain_image(3)
    assert (m.ops.equalize(img) == mirror_chain(C, img, "equalize")).all()
    assert (m.ops.autocontrast(img, 2.5) == mirror_chain(C, img, "autocontrast:2.5")).all()
    assert (m.ops.autocontrast(img) == mirror_chain(C, img, "autocontrast")).all()
    T = m.ops.otsu_level(img)
    assert isinstance(T, int) and T == mirror_otsu_level(np_hist(img))
    assert (m.ops.threshold_otsu(img) == np.where(img >= T, 255, 0)).all()
