"""Test frames of the distance-transform tests (shared by the CPU and the GPU
file): every frame of components_cases plus the ones a distance transform can
get wrong, and the scipy-based oracle in integers."""
import numpy as np

import components_cases as K

NONE = 2 ** 31 - 1
TOS = ("background", "foreground")


def parabola(H, W):
    """Background exactly on y = floor(x^2 / k), clipped to the frame: many sites stay on a row's envelope."""
    a = np.full((H, W), 255, np.uint8)
    k = max(1, (W * W) // max(H, 1))
    xs = np.arange(W)
    ys = (xs * xs) // k
    ok = ys < H
    a[ys[ok], xs[ok]] = 0
    return a


def cases(H, W, seam=None):
    """(name, mask) pairs for an H x W frame; `seam`: a column where a tile or block seam lies."""
    seam = W // 2 if seam is None else min(seam, W - 1)
    out = list(K.cases(H, W, seam))
    full = np.full((H, W), 255, np.uint8)
    for name, (y, x) in (("hole_tl", (0, 0)), ("hole_br", (H - 1, W - 1)), ("hole_centre", (H // 2, W // 2))):
        a = full.copy()
        a[y, x] = 0
        out.append((name, a))
    a = full.copy()
    a[0, 0] = a[H - 1, W - 1] = 0
    out.append(("two_far", a))
    for name, idx in (("bg_column0", (slice(None), 0)), ("bg_column_seam", (slice(None), seam)),
                      ("bg_row0", (0, slice(None))), ("bg_row_last", (H - 1, slice(None)))):
        a = full.copy()
        a[idx] = 0
        out.append((name, a))
    yy, xx = np.mgrid[0:H, 0:W]
    r = min(H, W) / 2 - 1
    out.append(("disc", (((yy - H // 2) ** 2 + (xx - W // 2) ** 2 <= r * r) * 255).astype(np.uint8)))
    out.append(("sparse", K.random_mask(H, W, 0.998, 31 * H + W)))
    out.append(("parabola", parabola(H, W)))
    a = full.copy()
    a[0, ::7] = 0  # six of seven columns have no site at all: "none" beside finite g in every row
    out.append(("none_columns", a))
    return out


def has_site(mask, to):
    return bool((mask != 0).any()) if to == "foreground" else bool((mask == 0).any())


def scipy_d2(mask, to):
    """scipy.ndimage.distance_transform_edt's nearest-site indices, then the squared distance in integers."""
    from scipy import ndimage

    fg = mask != 0
    inp = fg if to == "background" else ~fg
    idx = ndimage.distance_transform_edt(inp, return_distances=False, return_indices=True)
    yy, xx = np.mgrid[0:mask.shape[0], 0:mask.shape[1]]
    dy, dx = idx[0].astype(np.int64) - yy, idx[1].astype(np.int64) - xx
    return (dy * dy + dx * dx).astype(np.int32)


def brute_d2(mask, to):
    """The literal definition over all site pixels (small frames)."""
    site = (mask != 0) if to == "foreground" else (mask == 0)
    H, W = mask.shape
    ys, xs = np.nonzero(site)
    if ys.size == 0:
        return np.full((H, W), NONE, np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[:, :, None] - ys[None, None, :]).astype(np.int64) ** 2 + (xx[:, :, None] - xs[None, None, :]).astype(np.int64) ** 2
    return d.min(axis=2).astype(np.int32)


def numpy_u8(d2):
    r = np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64)
    r -= (r * r > d2)
    r += ((r + 1) * (r + 1) <= d2)
    return np.minimum(r, 255).astype(np.uint8)


def numpy_mask(d2, t, keep_above):
    return (((d2 > t) == keep_above) * 255).astype(np.uint8)


def numpy_float(d2):
    d = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    d[d2 == NONE] = np.inf
    return d


def disc(radius):
    t = int(np.floor(radius * radius))
    k = int(np.floor(np.sqrt(t)))
    yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
    return yy * yy + xx * xx <= t
