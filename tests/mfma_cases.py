"""Cases for the float MFMA kernels (k_blur_pl, k_conv_mfma, k_conv_i8): weight
recipes, the frame shapes that reach each of their seams, the frames of
tests/patterns.py with impulses at those seams, chain strings, and numpy mirrors
of the host-side error bounds.  No tests here (tests/test_gpu_mfma_patterns.py).

Seams of these kernels, in pixels: 16 (x-tile), 32 (RGB blur strip), 64 (conv
tile), 128 (gray blur strip), 256 (RGB blur window), 1024 (gray blur window);
in rows: 32 (blur group), 16 MT (conv row tile: 32 .. 160).
"""
from __future__ import annotations

import functools

import numpy as np

import oracle
import patterns

GPU_BAND = 4e-3  # tests/test_oracle_conv.py: f32 accumulation at |sum| <= ~600
BORDERS = ("reflect101", "replicate", "constant")
PX_SEAMS = (16, 32, 64, 128, 256)


def seams(C):
    """The kernels' x seams as byte periods of a row of C-channel pixels."""
    return tuple(p * C for p in PX_SEAMS) + ((1024,) if C == 1 else ())


# 161 rows: one past 160 and 128 and past a multiple of 32, 64, 80 and 96, so
# every conv row tile (16 MT rows) and the 32-row blur group have a second,
# partial tile; 129 / 65 / 130 px: one or two past the 64- and 128-px tiles
BASE_SHAPES = ((1, 1), (3, 2), (33, 129), (161, 65), (161, 130))
# blur widths: RGB 260 / 292 (W % 4 == 0, two 256-px windows), 257 / 131 (W % 4
# != 0: the NW = 8 lsb and NW = 4 exact edge kernels); gray 1028 (two 1024-px
# windows), 131 (the per-wave edge kernel)
BLUR_WIDTHS = {1: (1028, 131), 3: (260, 292, 257, 131)}


def conv_shapes(C):
    return list(BASE_SHAPES)


def blur_shapes(C):
    return list(BASE_SHAPES) + [(33, w) for w in BLUR_WIDTHS[C]]


@functools.lru_cache(maxsize=None)
def _frames(H, W, C):
    out = list(patterns.patterns(H, W, C, seams=seams(C)))
    for _, im in out:
        im.setflags(write=False)
    return out


def frames(H, W, C):
    """[(label, image)]: patterns.patterns with impulses at these kernels' seams (shared, read-only)."""
    return _frames(H, W, C)


def stack(labelled):
    """Frames of one shape as H x W x (N C): oracle.torch_sums takes any number of planes."""
    return np.concatenate([im.reshape(im.shape[0], im.shape[1], -1) for _, im in labelled], axis=-1)


def unstack(a, labelled):
    """The inverse of `stack` for an array of per-plane results."""
    out, k = [], 0
    for _, im in labelled:
        n = 1 if im.ndim == 2 else im.shape[2]
        out.append(a[..., k] if im.ndim == 2 else a[..., k:k + n])
        k += n
    return out


def block_sums(stacked, w, border, bx=32):
    """The fp64 sums of oracle.torch_sums for H x W x N planes on the CPU, as
    matrix products: row dy of the window is a banded Toeplitz matrix applied to
    blocks of `bx` output columns.  Same sums in another order (equal to ~1e-10,
    test_block_sums_match_torch); equal planes are computed once."""
    K = w.shape[0]
    R = K // 2
    H, W, N = stacked.shape
    planes = np.ascontiguousarray(np.moveaxis(stacked, -1, 0))
    first, inv = {}, []
    for i in range(N):
        inv.append(first.setdefault(planes[i].tobytes(), i))
    uniq = sorted(set(inv))
    inv = [uniq.index(i) for i in inv]
    x = planes[uniq].astype(np.float64)
    mode = {"reflect101": "reflect", "replicate": "edge", "constant": "constant"}[border]
    xp = np.pad(x, ((0, 0), (R, R), (R, R)), mode=mode)
    T = np.zeros((K, bx + 2 * R, bx))
    for dx in range(K):
        T[:, np.arange(bx) + dx, np.arange(bx)] = w[:, dx:dx + 1]
    out = np.zeros((len(x), H, W))
    for x0 in range(0, W, bx):
        nb = min(bx, W - x0)
        for dy in range(K):
            out[:, :, x0:x0 + nb] += xp[:, dy:dy + H, x0:x0 + nb + 2 * R] @ T[dy, :nb + 2 * R, :nb]
    return np.moveaxis(out[inv], 0, -1)


# ---- weight recipes -----------------------------------------------------------------
# neg3 mirrors gain3: `hp` alone reaches below 0 on the textured frames only and never
# above 255 (sum |w| = 4 on bytes: |sum| <= 510, ~N(0, 64) on the 0 / 255 draws)
FLOAT_RECIPES = ("unit", "gain3", "neg3", "hp")


def _rng(recipe, K, salt):
    return np.random.default_rng([salt, K, sum(map(ord, "gain3" if recipe == "neg3" else recipe))])  # neg3 = -gain3


def _unit2d(rng, K):
    w = rng.uniform(-0.5, 1.0, (K, K))
    w[0, -1] = 0.9  # asymmetric on purpose: transposes / mirrors show up
    return w / w.sum()


def _fix_sum(w, rng, lim):
    """Integer array `w` moved to sum 1 by +-1 steps at seeded positions, |w| <= lim kept."""
    flat = w.reshape(-1)
    d = 1 - int(flat.sum())
    order = rng.permutation(flat.size)
    i = 0
    while d != 0:
        j = order[i % flat.size]
        i += 1
        s = 1 if d > 0 else -1
        if abs(flat[j] + s) <= lim:
            flat[j] += s
            d -= s
    return w


def conv_weights(recipe, K):
    """K x K weights of a `conv:K` token (f64 values of the f32 weights)."""
    rng = _rng(recipe, K, 1)
    if recipe == "unit":
        w = _unit2d(rng, K)
    elif recipe == "gain3":  # the upper clamp is active on most of a saturated frame
        w = 3.0 * _unit2d(rng, K)
    elif recipe == "neg3":  # and the lower one
        w = -3.0 * _unit2d(rng, K)
    elif recipe == "hp":  # sums to zero, sum |w| = 4: the lower clamp on about half of every frame
        w = _unit2d(rng, K)
        w -= w.mean()
        w *= 4.0 / np.abs(w).sum()
    elif recipe == "int":
        # integer taps, |w| <= 64 (spread so that 255 sum |w| < 2^24 at K = 33), mixed
        # signs, asymmetric, sum 1: every sum of bytes is an integer below 2^24
        w = rng.integers(-40, 41, (K, K)).astype(np.int64)
        w[0, -1], w[-1, 0] = 64, -64
        w = _fix_sum(w, rng, 64).astype(np.float64)
    else:
        raise ValueError(recipe)
    return oracle.f32_weights(w)


def _place(K, rng, vals):
    """`vals` on both end taps and seeded inner taps of a K vector (the centre stays 0)."""
    v = np.zeros(K)
    inner = [i for i in range(1, K - 1) if i != K // 2]
    pos = [0, K - 1] + list(rng.permutation(inner)[:len(vals) - 2])
    v[pos] = vals
    return v


def sep_weights(recipe, K):
    """(h, v) of a `sepconv:K` token, K >= 9."""
    rng = _rng(recipe, K, 2)

    def unit(end):
        t = rng.uniform(-0.5, 1.0, K)
        t[end] = 0.9
        return t / t.sum()

    if recipe in FLOAT_RECIPES:
        h, v = unit(-1), unit(0)
        if recipe in ("gain3", "neg3"):
            v = (3.0 if recipe == "gain3" else -3.0) * v
        if recipe == "hp":  # zero-sum rows, sum |v (x) h| = 4
            h -= h.mean()
            h *= 4.0 / (np.abs(h).sum() * np.abs(v).sum())
    elif recipe == "int":  # two different integer vectors, sum 1, sum |.| = 15
        h, v = _place(K, rng, [5, -3, 2, -2, 1, -1, -1]), _place(K, rng, [-3, 4, 3, -2, 1, -1, -1])
    elif recipe == "int_lsb_h":
        # integer taps small enough for the single-part `:lsb` kernel (sep_lsb_bound
        # = sum |h| sum |v| / 16 + ~1e-3 < 0.45): mixed signs along x, one off-centre row
        h, v = _place(K, rng, [2, -1, 1, -1]), _place(K, rng, [0, 1])
    elif recipe == "int_lsb_v":
        h, v = _place(K, rng, [1, 0]), _place(K, rng, [-1, 2, -1, 1])
    else:
        raise ValueError(recipe)
    return oracle.f32_weights(h), oracle.f32_weights(v)


def sep_matrix(h, v):
    """The K x K weights of sepconv: the f32 product v[dy] * h[dx] (filters.cpp)."""
    return oracle.f32_weights(np.outer(v, h))


def _nums(a):
    return ";".join(repr(float(x)) for x in np.asarray(a).reshape(-1))


def conv_chain(w, lsb=False):
    return f"conv:{w.shape[0]}:{_nums(w)}" + (":lsb" if lsb else "")


def sep_chain(h, v, lsb=False):
    return f"sepconv:{len(h)}:{_nums(h)}:{_nums(v)}" + (":lsb" if lsb else "")


def scaled_band(w):
    """GPU_BAND is documented for |sum| <= ~600; the f32 epilogue and split
    errors grow linearly with the magnitude 255 sum |w|."""
    return GPU_BAND * max(1.0, 255.0 * float(np.abs(w).sum()) / 600.0)


# ---- kernel paths: (path, K, C) -> what runs there -------------------------------------
# path: blur (k_blur_pl), blur_lsb, f16 (k_conv_mfma), i8 (k_conv_i8), i8_lsb, small (k_conv_small)
PATHS = ([("blur", K, C) for K in (9, 31, 33) for C in (1, 3)] +
         [("blur_lsb", K, 3) for K in (9, 31, 33)] +
         [("f16", K, C) for K in (9, 11) for C in (1, 3)] +
         [("i8", 7, 3)] + [("i8", K, C) for K in (13, 17, 31, 33) for C in (1, 3)] +
         [("i8_lsb", K, C) for K in (13, 31) for C in (1, 3)] +
         [("small", 7, 1)])


def path_id(p):
    return f"{p[0]}-K{p[1]}-C{p[2]}"


def path_shapes(path, C):
    return blur_shapes(C) if path.startswith("blur") else conv_shapes(C)


def path_case(path, K, recipe):
    """(chain, K x K oracle weights) of `recipe` on `path`."""
    lsb = path.endswith("_lsb")
    if path.startswith("blur"):
        h, v = sep_weights(recipe, K)
        return sep_chain(h, v, lsb), sep_matrix(h, v)
    w = conv_weights(recipe, K)
    return conv_chain(w, lsb), w


def int_recipes(path):
    # `int` under :lsb falls back to the hi + lo kernel (its bound is ~14 LSB); the
    # two small recipes stay on the single-part kernel
    return ("int", "int_lsb_h", "int_lsb_v") if path == "blur_lsb" else ("int",)


def expected_desc(path, C, K):
    """Substrings plan_info's pass description must / must not hold on `path`."""
    kind = {"blur": "(mfma-separable)", "blur_lsb": "(mfma-separable)", "small": "(direct)"}.get(path, "(mfma)")
    return kind, path.endswith("_lsb")


# ---- numpy mirrors of the host-side bounds ------------------------------------------
def conv_shift(w, ND):
    """conv.hip conv_shift: the fixed-point exponent S of ND-digit weights."""
    wmax = (1 << 23) - (1 << 15) if ND == 3 else (1 << 15) - (1 << 7)
    maxw = float(np.abs(w).max())
    return int(np.floor(np.log2((wmax - 1) / maxw))) if maxw > 0 else 0


def conv_residuals(w, ND):
    """w 2^S - round(w 2^S), in units of 2^-S (llround: half away from zero)."""
    v = np.ldexp(np.asarray(w, np.float64), conv_shift(w, ND))
    return v - np.sign(v) * np.floor(np.abs(v) + 0.5)


def conv_quant_bound(w, ND):
    """conv.hip conv_quant_bound: 128 sum |r| 2^-S."""
    return 128.0 * float(np.ldexp(np.abs(conv_residuals(w, ND)).sum(), -conv_shift(w, ND)))


def sep_lsb_bound(h, v):
    """blur_sep.hip sep_lsb_bound."""
    h, v = np.asarray(h, np.float64), np.asarray(v, np.float64)
    f16 = lambda a: a.astype(np.float16).astype(np.float64)  # noqa: E731
    sh, dh = np.abs(h).sum(), np.abs(h - f16(h)).sum()
    sv, dv, svr = np.abs(v).sum(), np.abs(v - f16(v)).sum(), np.abs(f16(v)).sum()
    e1 = 128.0 * dh
    xmax = 128.0 * sh + e1
    if xmax >= 60000.0:
        return 1e30
    e2 = xmax * 2.0 ** -11
    return float(svr * (e1 + e2) + dv * 128.0 * sh + 1e-3 + 2.0 * len(h) * np.ldexp(xmax * (1.0 + sv), -24))


# ---- worst case of the conv :lsb bound ----------------------------------------------
def lsb_worst_weights(K, kind):
    """One dominant tap (0.5 at the centre, a whole number of 2^-S steps) and
    small taps (n +- 0.4) 2^-S, S = 15 the 2-digit exponent: each small tap leaves
    a residual of 0.4 steps, all of one sign (`kind` "one") or of seeded signs
    ("mixed").  168 (K = 13) or 200 small taps put the mirrored bound 128 sum |r|
    2^-S at 0.2625 / 0.3125, inside [0.25, 0.45): the kernel stays on two digits."""
    rng = np.random.default_rng([3, K, len(kind)])
    n_small = min(K * K - 1, 200)
    w = np.zeros(K * K)
    idx = [i for i in rng.permutation(K * K) if i != (K * K) // 2][:n_small]
    sign = np.ones(n_small) if kind == "one" else rng.choice([-1.0, 1.0], n_small)
    w[idx] = np.ldexp(rng.integers(1, 4, n_small) + 0.4 * sign, -15)
    w[(K * K) // 2] = 0.5
    return oracle.f32_weights(w.reshape(K, K))


def lsb_worst_frame(w, H, W, C, complement=False):
    """The K x K sign pattern of the 2-digit residuals tiled over the frame: 255 where r > 0, else 0."""
    K = w.shape[0]
    pat = np.where(conv_residuals(w, 2) > 0, 255, 0).astype(np.uint8)
    if complement:
        pat = 255 - pat
    # window (y - R .. y + R) of pixel y lines up with the pattern where (y - R) % K == 0
    img = np.tile(pat, (H // K + 2, W // K + 2))[:H, :W]
    return img if C == 1 else np.stack([img, np.roll(img, 1, axis=1), np.roll(img, 2, axis=0)], axis=-1)
