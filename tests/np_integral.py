"""An independent numpy reference of stripe/integral.h, written from the rule:
index maps give the border extension, cumsum in u64 masked to 32 bits gives the
wrapping tables, wrapped four-corner differences give the window sums, and the
five rules are computed in Python integers with math.isqrt.  scipy's
correlate1d on int64 with ones gives a second source for the window sums."""
import math

import numpy as np

OPS = ("box", "std", "mean", "niblack", "sauvola")
BORDERS = ("reflect101", "replicate", "constant")
SCIPY_MODE = {"reflect101": "mirror", "replicate": "nearest", "constant": "constant"}
MASK = np.uint64(0xFFFFFFFF)


def border_index(i, n, border):
    """The project's border_index on an array of coordinates; -1 for constant."""
    i = np.asarray(i, dtype=np.int64)
    if border == "constant":
        return np.where((i >= 0) & (i < n), i, -1)
    if border == "replicate":
        return np.clip(i, 0, n - 1)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    j = np.mod(i, period)
    return np.where(j < n, j, period - j)


def extend(a, R, border):
    """The frame extended by R on every side, (H + 2R) x (W + 2R) uint8."""
    H, W = a.shape
    ys = border_index(np.arange(-R, H + R), H, border)
    xs = border_index(np.arange(-R, W + R), W, border)
    P = a[np.maximum(ys, 0)][:, np.maximum(xs, 0)].copy()
    P[ys < 0, :] = 0
    P[:, xs < 0] = 0
    return P


def table(P, squared=False):
    """The wrapping u32 integral of P: (h + 1) x (w + 1) uint64 values below 2^32, row 0 and column 0 zero."""
    v = P.astype(np.uint64)
    if squared:
        v = v * v
    t = np.zeros((P.shape[0] + 1, P.shape[1] + 1), np.uint64)
    t[1:, 1:] = np.cumsum(np.cumsum(v, axis=0, dtype=np.uint64), axis=1, dtype=np.uint64) & MASK
    return t


def integral(a, squared=False):
    """The public form: int32, two's complement."""
    return table(a, squared).astype(np.uint32).view(np.int32)


def window_sums(a, K, border, squared=False):
    """H x W window sums over the extended frame from the wrapped table: d - b - c + a modulo 2^32."""
    H, W = a.shape
    t = table(extend(a, K // 2, border), squared)
    s = t[K:K + H, K:K + W] - t[:H, K:K + W] - t[K:K + H, :W] + t[:H, :W]  # uint64 wraps modulo 2^64
    return s & MASK


def scipy_sums(a, K, border, squared=False):
    from scipy import ndimage

    v = a.astype(np.int64)
    if squared:
        v = v * v
    ones = np.ones(K, np.int64)
    mode = SCIPY_MODE[border]
    return ndimage.correlate1d(ndimage.correlate1d(v, ones, axis=0, mode=mode), ones, axis=1, mode=mode)


def kq_of(k):
    return int(np.rint(4096.0 * k))  # ties to even


def rule(op, p, A, B, N, c=0, kq=0):
    """One output value from Python integers."""
    if op == "box":
        return (A + N // 2) // N
    if op == "mean":
        return 255 if p > (A + N // 2) // N - c else 0
    V = N * B - A * A
    assert V >= 0
    s = math.isqrt(V)
    if op == "std":
        return s // N
    if op == "niblack":
        return 255 if 4096 * (p * N - A + c * N) > kq * s else 0
    if op == "sauvola":
        return 255 if 4096 * (p * N - A) * N * 128 > kq * A * (s - 128 * N) else 0
    raise ValueError(op)


def window(a, op, K, border="reflect101", c=0, k=None):
    """The window operation on an H x W uint8 frame, uint8."""
    a = np.asarray(a)
    N = K * K
    A = window_sums(a, K, border)
    kq = kq_of(0.2 if k is None else k) if op in ("niblack", "sauvola") else 0
    if op == "box":
        return ((A + np.uint64(N // 2)) // np.uint64(N)).astype(np.uint8)
    if op == "mean":
        m = ((A + np.uint64(N // 2)) // np.uint64(N)).astype(np.int64)
        return ((a.astype(np.int64) > m - c) * 255).astype(np.uint8)
    B = window_sums(a, K, border, squared=True)
    out = np.empty(a.shape, np.uint8)
    for (y, x), p in np.ndenumerate(a):
        out[y, x] = rule(op, int(p), int(A[y, x]), int(B[y, x]), N, c, kq)
    return out


def sauvola_float(a, K, border, k):
    """The float64 formula p > m (1 + k (s / 128 - 1)) with the real mean and standard deviation."""
    N = float(K * K)
    A = window_sums(a, K, border).astype(np.float64)
    B = window_sums(a, K, border, squared=True).astype(np.float64)
    m = A / N
    s = np.sqrt(np.maximum(B / N - m * m, 0.0))
    return ((a.astype(np.float64) > m * (1.0 + k * (s / 128.0 - 1.0))) * 255).astype(np.uint8)
