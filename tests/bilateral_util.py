"""Shared by the bilateral tests: the test frames and a numpy mirror of the rule
written from its definition (filters.h), not from the C++:

  ws(dy,dx) = g[dy] g[dx], g the binomial taps (1 2 1 / 1 4 6 4 1)
  r[d] = rint(255 exp(-d^2 / (2 S^2))), d = 0..255
  w = ws r[|p - c|], D = sum w, N = sum w p, out = (N + (D >> 1)) // D
per channel, on the border-extended image.
"""
import numpy as np

TAPS = {3: (1, 2, 1), 5: (1, 4, 6, 4, 1)}
TIES = np.array([0, 1, 2, 253, 254, 255], np.uint8)
SHAPES = [(1, 1), (3, 2), (2, 7), (17, 15), (64, 65)]


def table(S):
    d = np.arange(256, dtype=np.float64)
    return np.rint(255.0 * np.exp(-(d * d) / (2.0 * S * S))).astype(np.int64)


def _border_index(i, n, border):
    """Source index of position i on an axis of n pixels, -1: a zero pixel."""
    if 0 <= i < n:
        return i
    if border == "constant":
        return -1
    if border == "replicate":
        return 0 if i < 0 else n - 1
    if n == 1:  # reflect101
        return 0
    period = 2 * (n - 1)
    j = i % period
    return j if j < n else period - j


def extend(x, R, border):
    """x (H, W, C) with R border pixels on every side."""
    H, W = x.shape[:2]
    out = np.zeros((H + 2 * R, W + 2 * R, x.shape[2]), x.dtype)
    ys = [_border_index(y - R, H, border) for y in range(H + 2 * R)]
    xs = [_border_index(c - R, W, border) for c in range(W + 2 * R)]
    for j, sy in enumerate(ys):
        if sy < 0:
            continue
        for i, sx in enumerate(xs):
            if sx >= 0:
                out[j, i] = x[sy, sx]
    return out


def _windows(img, K, border):
    x = img.reshape(img.shape[0], img.shape[1], -1).astype(np.int64)
    H, W = x.shape[:2]
    ext = extend(x, K // 2, border)
    g = TAPS[K]
    for dy in range(K):
        for dx in range(K):
            yield x, g[dy] * g[dx], ext[dy:dy + H, dx:dx + W]


def mirror(img, K, S, border="reflect101", skip=False):
    """The integer rule.  skip: the @skip border (pixels with x <= R, y <= R,
    x >= W - R or y >= H - R keep their value)."""
    r = table(S)
    D = N = 0
    for x, ws, p in _windows(img, K, border):
        w = ws * r[np.abs(p - x)]
        D = D + w
        N = N + w * p
    out = (N + (D >> 1)) // D
    if skip:
        R = K // 2
        H, W = x.shape[:2]
        yy, xx = np.mgrid[0:H, 0:W]
        keep = (xx <= R) | (yy <= R) | (xx >= W - R) | (yy >= H - R)
        out[keep] = x[keep]
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8).reshape(img.shape)


def real_valued(img, K, S, border="reflect101"):
    """float64 bilateral: the same binomial taps, the exp range kernel itself."""
    D = N = 0.0
    for x, ws, p in _windows(img, K, border):
        w = ws * np.exp(-((p - x) ** 2) / (2.0 * S * S))
        D = D + w
        N = N + w * p
    return (N / D).reshape(img.shape)


def frames(rng, shape, C):
    """name -> frame: uniform bytes, a noisy 60 | 180 step, the tie set, and a
    pair frame (each 16 x 16 block draws from one pair (a, a + k), k running
    over 0..255 with the block index, so the blocks of a large frame use every
    table entry as a weight)."""
    full = shape + (3,) if C == 3 else shape
    H, W = shape
    step = np.where(np.arange(W) < W // 2, 60.0, 180.0)[None, :, None] + rng.normal(0.0, 12.0, size=(H, W, C))
    by, bx = np.mgrid[0:H, 0:W] // 16
    k = (by * ((W + 15) // 16) + bx) % 256
    a = _block_const(rng.integers(0, 256, size=(H, W)) % (256 - k), 16)  # one a per block, a + k <= 255
    pair = a[..., None] + k[..., None] * rng.integers(0, 2, size=(H, W, C))
    return {
        "uniform": rng.integers(0, 256, size=full, dtype=np.uint8),
        "step": np.clip(np.rint(step), 0, 255).astype(np.uint8).reshape(full),
        "ties": rng.choice(TIES, size=full),
        "pair": pair.astype(np.uint8).reshape(full),
    }


def _block_const(a, B):
    """a with every B x B block set to its top-left value."""
    H, W = a.shape
    yy, xx = np.mgrid[0:H, 0:W]
    return a[(yy // B) * B, (xx // B) * B]
