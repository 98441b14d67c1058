"""The affine warp rule (csrc/include/stripe/warp.h) in numpy: `np_warp` is
golden_warp's mirror in int64 from the six integers of a quantised map
(A00, A01, B0, A10, A11, B1); `float_warp` samples the same way in float64
with the unquantised inverse matrix, for the error bound."""
import numpy as np


def _taps(a, iy, ix, border, fill):
    """a[iy, ix] per channel with the border rule; a is H x W x C."""
    H, W = a.shape[:2]
    cy, cx = np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)
    v = a[cy, cx].astype(np.int64)
    if border == "constant":
        out = (ix < 0) | (iy < 0) | (ix >= W) | (iy >= H)
        v[out] = fill
    return v


def np_warp(a, q, W2, H2, mode="bilinear", border="constant", fill=0):
    a3 = a[:, :, None] if a.ndim == 2 else a
    A00, A01, B0, A10, A11, B1 = (int(v) for v in q)
    y, x = np.mgrid[0:H2, 0:W2].astype(np.int64)
    sx = A00 * x + A01 * y + B0
    sy = A10 * x + A11 * y + B1
    if mode == "nearest":
        out = _taps(a3, (sy + (1 << 23)) >> 24, (sx + (1 << 23)) >> 24, border, fill)
    else:
        X, Y = (sx + (1 << 15)) >> 16, (sy + (1 << 15)) >> 16
        ix, iy = X >> 8, Y >> 8
        fx, fy = (X & 255)[:, :, None], (Y & 255)[:, :, None]
        top = (256 - fx) * _taps(a3, iy, ix, border, fill) + fx * _taps(a3, iy, ix + 1, border, fill)
        bot = (256 - fx) * _taps(a3, iy + 1, ix, border, fill) + fx * _taps(a3, iy + 1, ix + 1, border, fill)
        out = ((256 - fy) * top + fy * bot + 32768) >> 16
    assert out.min() >= 0 and out.max() <= 255
    out = out.astype(np.uint8)
    return out[:, :, 0] if a.ndim == 2 else out


def float_warp(a, minv, W2, H2, border="constant", fill=0):
    """Bilinear sampling in float64 at the exact positions of the unquantised inverse matrix (no rounding)."""
    a3 = a[:, :, None] if a.ndim == 2 else a
    m = np.asarray(minv, np.float64).reshape(2, 3)
    y, x = np.mgrid[0:H2, 0:W2].astype(np.float64)
    sx = m[0, 0] * x + m[0, 1] * y + m[0, 2]
    sy = m[1, 0] * x + m[1, 1] * y + m[1, 2]
    ix, iy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = (sx - ix)[:, :, None], (sy - iy)[:, :, None]
    t = lambda dy, dx: _taps(a3, iy + dy, ix + dx, border, fill).astype(np.float64)
    out = (1 - fy) * ((1 - fx) * t(0, 0) + fx * t(0, 1)) + fy * ((1 - fx) * t(1, 0) + fx * t(1, 1))
    return out[:, :, 0] if a.ndim == 2 else out


ANGLES = (0.01, 1, 30, 45, 135, -77.7, 359.99)


def maps(C, W, H):
    """The maps every layer is tested on, for a W x H source: (name, inverse matrix, W2, H2), the inverse
    matrix unquantised (float64)."""
    out = [("identity", [1, 0, 0, 0, 1, 0], W, H),
           ("shift+3-2", invert([1, 0, 3, 0, 1, -2]), W, H),
           ("shift+0.5+1.25", invert([1, 0, 0.5, 0, 1, 1.25]), W, H),
           ("scale0.5", invert([0.5, 0, 0, 0, 0.5, 0]), max(1, W // 2), max(1, H // 2)),
           ("scale2", invert([2, 0, 0, 0, 2, 0]), min(2 * W, 300), min(2 * H, 300)),
           ("shear", invert([1, 0.3, -4, -0.2, 1, 6]), W + 9, H + 5),
           ("minify8", invert([0.125, 0, 0, 0, 0.125, 0]), max(1, W // 8), max(1, H // 8)),
           ("coef+63.9", [63.9, -63.9, 1.5, 63.9, 63.9, -60.25], 7, 5),
           ("all-outside", invert([1, 0, 10000, 0, 1, -20000]), W, H)]
    for k in range(4):
        out.append((f"rot{90 * k}:fit",) + tuple(C.rotate_matrix(90.0 * k, True, W, H)))
    for deg in ANGLES:
        for fit in (False, True):
            out.append((f"rot{deg}:{'fit' if fit else 'same'}",) + tuple(C.rotate_matrix(float(deg), fit, W, H)))
    return out


def quantise(C, minv, W, H, W2, H2):
    """The six integers of an inverse matrix."""
    return list(C.warp_quantise([float(v) for v in minv], True, W, H, W2, H2)[:6])


def bound(W2, H2):
    """Largest distance of the rule from `float_warp`, in levels: the Q8 position rounding (2^-9) plus the
    coefficient rounding (2^-25 per coefficient, times x, y and 1), times bilinear's slope of at most 255 a
    pixel on each axis, plus the final rounding."""
    return 0.5 + 510 * (2.0 ** -9 + 2.0 ** -25 * (W2 + H2 + 1))


def invert(M):
    """The inverse of a forward 2 x 3 matrix, in float64."""
    a, b, c, d, e, f = (float(v) for v in M)
    det = a * e - b * d
    return [e / det, -b / det, (b * f - c * e) / det, -d / det, a / det, (c * d - a * f) / det]
