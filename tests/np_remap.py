"""The mesh warp rule (csrc/include/stripe/remap.h) in numpy, written from the
rule: `np_remap` is golden_remap's mirror on int64 arrays; `mesh_positions`
is the interpolated mesh position of every pixel in float64 (exact: P is an
integer below 2^43); `float_sample` samples bilinearly in float64 at exact
positions, for the error bounds; the exact maps of the builders follow."""
import numpy as np

SPACINGS = (1, 2, 4, 8, 16, 32, 64)


def grid(n, S):
    s = S.bit_length() - 1
    return ((n - 1) >> s) + 2


def _taps(a, iy, ix, border, fill):
    """a[iy, ix] per channel with the border rule; a is H x W x C."""
    H, W = a.shape[:2]
    cy, cx = np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)
    v = a[cy, cx].astype(np.int64)
    if border == "constant":
        out = (ix < 0) | (iy < 0) | (ix >= W) | (iy >= H)
        v[out] = fill
    return v


def mesh_P(mesh, S, W2, H2):
    """P of both coordinates for every output pixel: int64 (H2, W2, 2), Q(12 + 2s)."""
    s = S.bit_length() - 1
    M = np.asarray(mesh).astype(np.int64)
    assert M.shape == (grid(H2, S), grid(W2, S), 2), (M.shape, S, W2, H2)
    y, x = np.mgrid[0:H2, 0:W2].astype(np.int64)
    j, tx, i, ty = x >> s, (x & (S - 1))[:, :, None], y >> s, (y & (S - 1))[:, :, None]
    return ((S - tx) * (S - ty) * M[i, j] + tx * (S - ty) * M[i, j + 1] + (S - tx) * ty * M[i + 1, j] +
            tx * ty * M[i + 1, j + 1])


def np_remap(a, mesh, S, W2, H2, mode="bilinear", border="constant", fill=0):
    a3 = a[:, :, None] if a.ndim == 2 else a
    s = S.bit_length() - 1
    P = mesh_P(mesh, S, W2, H2)
    assert np.abs(P).max() < 1 << 43
    if mode == "nearest":
        I = (P + (1 << (11 + 2 * s))) >> (12 + 2 * s)
        out = _taps(a3, I[:, :, 1], I[:, :, 0], border, fill)
    else:
        Q = (P + (1 << (3 + 2 * s))) >> (4 + 2 * s)
        ix, iy = Q[:, :, 0] >> 8, Q[:, :, 1] >> 8
        fx, fy = (Q[:, :, 0] & 255)[:, :, None], (Q[:, :, 1] & 255)[:, :, None]
        top = (256 - fx) * _taps(a3, iy, ix, border, fill) + fx * _taps(a3, iy, ix + 1, border, fill)
        bot = (256 - fx) * _taps(a3, iy + 1, ix, border, fill) + fx * _taps(a3, iy + 1, ix + 1, border, fill)
        out = ((256 - fy) * top + fy * bot + 32768) >> 16
    assert out.min() >= 0 and out.max() <= 255
    out = out.astype(np.uint8)
    return out[:, :, 0] if a.ndim == 2 else out


def mesh_positions(mesh, S, W2, H2):
    """(sx, sy) in pixels the mesh gives every output pixel, float64 (exact)."""
    s = S.bit_length() - 1
    P = mesh_P(mesh, S, W2, H2).astype(np.float64) / float(1 << (12 + 2 * s))
    return P[:, :, 0], P[:, :, 1]


def float_sample(a, sx, sy, border="constant", fill=0):
    """Bilinear sampling in float64 at the positions (sx, sy), no rounding."""
    a3 = a[:, :, None] if a.ndim == 2 else a
    ix, iy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = (sx - ix)[:, :, None], (sy - iy)[:, :, None]
    t = lambda dy, dx: _taps(a3, iy + dy, ix + dx, border, fill).astype(np.float64)  # noqa: E731
    out = (1 - fy) * ((1 - fx) * t(0, 0) + fx * t(0, 1)) + fy * ((1 - fx) * t(1, 0) + fx * t(1, 1))
    return out[:, :, 0] if a.ndim == 2 else out


def bound(S):
    """Largest distance of the rule from `float_sample` at the exact map, in levels: the final rounding plus
    bilinear's slope of at most 255 a pixel on each axis times the position error: the Q8 rounding (2^-9), the
    interpolation between the nodes (2^-10, none at S = 1) and the node rounding (2^-13)."""
    return 0.5 + 510 * (2.0 ** -9 + (2.0 ** -10 if S > 1 else 0.0) + 2.0 ** -13)


POSITION_BOUND = 2.0 ** -10 + 2.0 ** -13


def perspective_positions(Hinv, W2, H2):
    """The exact positions of the inverse 3 x 3 matrix (destination -> source), float64."""
    q = np.asarray(Hinv, np.float64).reshape(3, 3)
    y, x = np.mgrid[0:H2, 0:W2].astype(np.float64)
    w = q[2, 0] * x + q[2, 1] * y + q[2, 2]
    return (q[0, 0] * x + q[0, 1] * y + q[0, 2]) / w, (q[1, 0] * x + q[1, 1] * y + q[1, 2]) / w


def radial_positions(k1, k2, f, cx, cy, W, H):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    xn, yn = (x - cx) / f, (y - cy) / f
    r2 = xn * xn + yn * yn
    k = 1 + k1 * r2 + k2 * r2 * r2
    return cx + f * xn * k, cy + f * yn * k


def mesh_of(fn, S, W2, H2):
    """The mesh of a map fn(x, y) -> (sx, sy) on float64 arrays: rint(4096 pos) at the nodes."""
    i, j = np.mgrid[0:grid(H2, S), 0:grid(W2, S)].astype(np.float64)
    sx, sy = fn(j * S, i * S)
    return np.stack([np.rint(4096.0 * sx), np.rint(4096.0 * sy)], axis=2).astype(np.int32)


def identity_mesh(S, W2, H2):
    return mesh_of(lambda x, y: (x, y), S, W2, H2)


def translation_mesh(S, W2, H2, dx, dy):
    """out(x, y) = in(x + dx, y + dy)"""
    return mesh_of(lambda x, y: (x + dx, y + dy), S, W2, H2)


def rotation_mesh(S, W2, H2, deg, cx, cy):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return mesh_of(lambda x, y: (cx + c * (x - cx) - s * (y - cy), cy + s * (x - cx) + c * (y - cy)), S, W2, H2)


def random_mesh(S, W2, H2, seed, spread=None):
    """Seeded nodes within +-spread pixels of the identity, or (spread None) anywhere in +-2^18 pixels."""
    rng = np.random.default_rng(seed)
    shape = (grid(H2, S), grid(W2, S), 2)
    if spread is None:
        lim = (1 << 30) - 1
        return rng.integers(-lim, lim + 1, shape, dtype=np.int64).astype(np.int32)
    return (identity_mesh(S, W2, H2).astype(np.int64) + rng.integers(-spread * 4096, spread * 4096 + 1, shape)).astype(np.int32)


KEYSTONE_MILD = [1.02, 0.03, -3.0, 0.01, 1.05, -2.0, 2e-5, 4e-5, 1.0]      # destination -> source
KEYSTONE_STRONG = [0.9, 0.1, 2.0, -0.05, 1.1, 1.0, 2.5e-3, 1.5e-3, 1.0]
AFFINE_H = [0.8, -0.3, 12.5, 0.25, 0.9, -7.25, 0.0, 0.0, 1.0]
