"""Test frames of the connected-component tests (shared by the CPU and the GPU
file) and the scipy-based oracle with canonical numbering."""
import numpy as np

DENSITIES = (0.2, 0.5, 0.593, 0.8)


def spiral(H, W):
    """A one-pixel-wide rectangular spiral that fills the frame: one component, the longest path."""
    a = np.zeros((H, W), np.uint8)
    if H == 1 or W == 1:
        a[:] = 255
        return a
    top, left, bottom, right = 0, 0, H - 1, W - 1
    y, x = 0, 0
    a[0, 0] = 255
    # walk right, down, left, up, keeping one background line between the turns
    d = 0
    while True:
        if d == 0:
            tx = right
            if tx <= x:
                break
            a[y, x:tx + 1] = 255
            x = tx
            top += 2
        elif d == 1:
            ty = bottom
            if ty <= y:
                break
            a[y:ty + 1, x] = 255
            y = ty
            right -= 2
        elif d == 2:
            tx = left
            if tx >= x:
                break
            a[y, tx:x + 1] = 255
            x = tx
            bottom -= 2
        else:
            ty = top
            if ty >= y:
                break
            a[ty:y + 1, x] = 255
            y = ty
            left += 2
        d = (d + 1) % 4
    return a


def comb(H, W):
    """Teeth on every other column, joined only at the bottom row: many provisional labels that merge late."""
    a = np.zeros((H, W), np.uint8)
    a[:, ::2] = 255
    a[H - 1, :] = 255
    return a


def u_shape(H, W, seam):
    """A U whose arms lie left and right of column `seam` and meet only in the last row."""
    a = np.zeros((H, W), np.uint8)
    l, r = max(seam - 2, 0), min(seam + 1, W - 1)
    a[:, l] = 255
    a[:, r] = 255
    a[H - 1, l:r + 1] = 255
    return a


def random_mask(H, W, density, seed, value=255):
    rng = np.random.default_rng(seed)
    return ((rng.random((H, W)) < density) * value).astype(np.uint8)


def cases(H, W, seam=None):
    """(name, mask) pairs for an H x W frame; `seam`: a column where a tile or block seam lies."""
    seam = W // 2 if seam is None else min(seam, W - 1)
    z = np.zeros((H, W), np.uint8)
    out = [("background", z.copy()), ("foreground", np.full((H, W), 255, np.uint8))]
    one = z.copy()
    one[H // 2, W // 2] = 255
    out.append(("single", one))
    corners = z.copy()
    corners[0, 0] = corners[0, W - 1] = corners[H - 1, 0] = corners[H - 1, W - 1] = 255
    out.append(("corners", corners))
    yy, xx = np.mgrid[0:H, 0:W]
    out.append(("checkerboard", (((yy + xx) % 2 == 0) * 255).astype(np.uint8)))
    out.append(("hstripes", ((yy % 2 == 0) * 255).astype(np.uint8)))
    out.append(("vstripes", ((xx % 2 == 0) * 255).astype(np.uint8)))
    out.append(("diagonals", (((yy + xx) % 4 == 0) * 255).astype(np.uint8)))
    out.append(("antidiagonals", (((yy - xx) % 4 == 0) * 255).astype(np.uint8)))
    out.append(("spiral", spiral(H, W)))
    out.append(("comb", comb(H, W)))
    border = z.copy()
    border[0, :] = border[H - 1, :] = border[:, 0] = border[:, W - 1] = 255
    out.append(("border", border))
    out.append(("u", u_shape(H, W, seam)))
    for k, d in enumerate(DENSITIES):
        out.append((f"random{d}", random_mask(H, W, d, 1000 * k + 17 * H + W)))
    for v in (1, 2, 128):
        out.append((f"value{v}", random_mask(H, W, 0.55, 77 + v, value=v)))
    return out


def scipy_labels(mask, connectivity):
    """scipy.ndimage.label with the components renumbered in raster order of their first pixel."""
    from scipy import ndimage

    st = ndimage.generate_binary_structure(2, 1) if connectivity == 4 else np.ones((3, 3), int)
    lab, n = ndimage.label(mask != 0, structure=st)
    flat = lab.ravel()
    fg = np.flatnonzero(flat)
    # the first raster index of every label, then their rank
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat[fg], fg)
    order = np.argsort(first[1:], kind="stable")
    renum = np.zeros(n + 1, np.int32)
    renum[order + 1] = np.arange(1, n + 1, dtype=np.int32)
    return renum[lab].astype(np.int32), n


def numpy_stats(labels, n):
    """The (n + 1, 7) table from scipy / numpy primitives."""
    from scipy import ndimage

    H, W = labels.shape
    idx = np.arange(n + 1)
    yy, xx = np.mgrid[0:H, 0:W]
    ones = np.ones_like(labels, dtype=np.int64)
    t = np.zeros((n + 1, 7), np.int64)
    t[:, 0] = ndimage.sum(ones, labels, idx).astype(np.int64)
    t[:, 5] = np.rint(ndimage.sum(xx.astype(np.float64), labels, idx)).astype(np.int64)
    t[:, 6] = np.rint(ndimage.sum(yy.astype(np.float64), labels, idx)).astype(np.int64)
    # find_objects works on labels >= 1: shift by one so that the background gets a slice too
    for l, sl in enumerate(ndimage.find_objects(labels + 1, max_label=n + 1)):
        if sl is not None:
            t[l, 1], t[l, 3] = sl[1].start, sl[1].stop
            t[l, 2], t[l, 4] = sl[0].start, sl[0].stop
    return t


def numpy_area_filter(mask, labels, n, amin, amax=None):
    area = np.bincount(labels.ravel(), minlength=n + 1)
    keep = area >= amin
    if amax is not None:
        keep &= area <= amax
    keep[0] = False
    return np.where(keep[labels] & (mask != 0), mask, 0).astype(np.uint8)
