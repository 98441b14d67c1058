"""The eight orientations as numpy expressions (the table of stripe/orient.h),
for the orientation tests.  Index i of NAMES is Exif Orientation i + 1."""
import numpy as np

NAMES = ("none", "fliph", "rot180", "flipv", "transpose", "rot90", "transverse", "rot270")
# name -> (T, FX, FY)
BITS = {"none": (0, 0, 0), "fliph": (0, 1, 0), "rot180": (0, 1, 1), "flipv": (0, 0, 1),
        "transpose": (1, 0, 0), "rot90": (1, 0, 1), "transverse": (1, 1, 1), "rot270": (1, 1, 0)}
NP = {
    "none": lambda a: a,
    "fliph": lambda a: a[:, ::-1],
    "rot180": lambda a: a[::-1, ::-1],
    "flipv": lambda a: a[::-1],
    "transpose": lambda a: a.swapaxes(0, 1),
    "rot90": lambda a: np.rot90(a, -1),
    "transverse": lambda a: a[::-1, ::-1].swapaxes(0, 1),
    "rot270": lambda a: np.rot90(a, 1),
}


def np_orient(a, name, crop=None):
    out = NP[name](a)
    if crop is not None:
        x0, y0, w, h = crop
        out = out[y0:y0 + h, x0:x0 + w]
    return np.ascontiguousarray(out)


def coord_frame(W, H, ch, seed=0):
    """Pixels that encode their coordinates (row in the high bits, column in the low bits of the value, the
    channel added), plus noise in the lowest bit."""
    y, x = np.mgrid[0:H, 0:W]
    base = (y * 37 + x * 5) & 0xFE
    noise = np.random.default_rng(seed + W * 7919 + H * 31 + ch).integers(0, 2, (H, W, ch))
    a = ((base[:, :, None] + 64 * np.arange(ch)[None, None, :]) & 0xFE) | noise
    a = a.astype(np.uint8)
    return a[:, :, 0] if ch == 1 else a
