"""An independent numpy reference of stripe/canny.h, written from the rule:
np_integral's index maps give the border extension (repeated reflection on tiny
frames), shifted slices of the padded arrays give the Sobel gradient and the
neighbours' magnitudes, the sector and survival tests are vectorised masks, and
scipy.ndimage.label plus a flag per label gives the hysteresis."""
import numpy as np

import np_integral as NI

BORDERS = NI.BORDERS
NORMS = ("l1", "l2")
TAN = 13573  # round(tan 22.5 deg * 2^15)
assert TAN == round(np.tan(np.pi / 8) * 2 ** 15)


def gradient(a, border):
    """(Gx, Gy), int64 H x W, from the frame extended by one pixel."""
    P = NI.extend(np.asarray(a), 1, border).astype(np.int64)
    H, W = a.shape

    def at(dy, dx):
        return P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]

    gx = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    gy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    return gx, gy


def magnitude(gx, gy, norm):
    ax, ay = np.abs(gx), np.abs(gy)
    return ax + ay if norm == "l1" else ax * ax + ay * ay


def classes(a, low, high, norm="l1", border="reflect101"):
    """The class plane, uint8 0 / 1 / 2."""
    a = np.asarray(a)
    H, W = a.shape
    gx, gy = gradient(a, border)
    m = magnitude(gx, gy, norm)
    lo, hi = (low, high) if norm == "l1" else (low * low, high * high)
    Mp = np.pad(m, 1)  # a position outside the frame has magnitude 0

    def nb(dy, dx):
        return Mp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]

    ax, ay = np.abs(gx), np.abs(gy)
    horizontal = (ay << 15) < ax * TAN
    vertical = ~horizontal & ((ay << 15) > ax * TAN + (ax << 16))
    diagonal = ~horizontal & ~vertical
    # one zero component lands in the first two sectors; Gx = Gy = 0 falls through, and m = 0 survives nothing
    assert not (diagonal & ((gx == 0) != (gy == 0))).any()
    same = (gx < 0) == (gy < 0)  # s = +1
    survives = np.where(horizontal, (m > nb(0, -1)) & (m >= nb(0, 1)),
                        np.where(vertical, (m > nb(-1, 0)) & (m >= nb(1, 0)),
                                 np.where(same, (m > nb(-1, -1)) & (m > nb(1, 1)), (m > nb(-1, 1)) & (m > nb(1, -1)))))
    keep = survives & (m > lo)
    return np.where(keep, np.where(m > hi, 2, 1), 0).astype(np.uint8)


def hysteresis(cls, connectivity=8):
    """255 where the class is >= 1 and the component among class >= 1 holds a class 2 pixel."""
    from scipy import ndimage

    structure = np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    lab, n = ndimage.label(cls >= 1, structure=structure)
    strong = np.zeros(n + 1, bool)
    strong[lab[cls == 2]] = True
    strong[0] = False
    return np.where(strong[lab], 255, 0).astype(np.uint8)


def canny(a, low, high, norm="l1", border="reflect101"):
    return hysteresis(classes(a, low, high, norm, border), 8)


def pixel_classes(a, low, high):
    a = np.asarray(a)
    return np.where(a > high, 2, np.where(a > low, 1, 0)).astype(np.uint8)


def hysteresis_threshold(a, low, high, connectivity=8):
    return hysteresis(pixel_classes(a, low, high), connectivity)
