"""Colour matrix cases shared by test_color_matrix.py and test_gpu_color_matrix.py.

Every case is (token, M, b) with the decimal 3x3 matrix M and offsets b the
token stands for; `mirror` evaluates the specified Q12 formula in numpy int64
from those decimals (it never asks the extension for its coefficients).
"""
import numpy as np

LUMA = (0.299, 0.587, 0.114)


def saturation_q(s):
    """Quantised saturation:S matrix: off-diagonals rounded, the diagonal takes
    what is left of 4096."""
    q = np.zeros((3, 3), np.int64)
    for c in range(3):
        for k in range(3):
            if k != c:
                q[c, k] = int(np.rint((1.0 - s) * LUMA[k] * 4096.0))
        q[c, c] = 4096 - q[c].sum()
    return q


def quantise(M, b):
    q = np.rint(np.asarray(M, np.float64) * 4096.0).astype(np.int64)
    qb = np.rint(np.asarray(b, np.float64) * 4096.0).astype(np.int64)
    assert np.abs(q).max() <= 32767 and np.abs(np.asarray(b)).max() <= 2048
    return q, qb


def _token(M, b=None):
    t = "colormatrix:" + ";".join(repr(float(v)) for v in np.asarray(M).reshape(-1))
    if b is not None:
        t += ":" + ";".join(repr(float(v)) for v in b)
    return t


def _sat_matrix(s):
    M = np.array([[(1.0 - s) * LUMA[k] for k in range(3)] for _ in range(3)])
    return M + s * np.eye(3)


SEPIA = [[.393, .769, .189], [.349, .686, .168], [.272, .534, .131]]
YCBCR = [[.299, .587, .114], [-.168736, -.331264, .5], [.5, -.418688, -.081312]]
YCBCR_INV = [[1, 0, 1.402], [1, -.344136, -.714136], [1, 1.772, 0]]
YCBCR_INV_B = [-1.402 * 128, .344136 * 128 + .714136 * 128, -1.772 * 128]
# nine distinct mixed-sign coefficients, three distinct offsets: a transposed
# matrix or permuted offsets change the result
MIXED = [[0.5, -0.25, 0.75], [1.25, 0.125, -0.625], [-0.375, 0.875, 0.3125]]
MIXED_B = [10.0, -20.5, 33.25]
# the largest coefficients and offsets the format takes: accumulator width
WIDE = [[7.99, 7.99, 7.99], [-7.99, -7.99, -7.99], [7.99, -7.99, 7.99]]
WIDE_B = [2048.0, -2048.0, -2048.0]
WIDE2_B = [-2048.0, 2048.0, 2048.0]

# name -> (token, (q, qb) of the mirror, (M, b) of the float oracle)
CASES = {}


def _add(name, token, M, b, q=None):
    qq, qb = quantise(M, b)
    CASES[name] = (token, (qq if q is None else q, qb), (np.asarray(M, np.float64), np.asarray(b, np.float64)))


_add("identity", "colormatrix:1;0;0;0;1;0;0;0;1", np.eye(3), [0, 0, 0])
_add("swaprb", "swaprb", [[0, 0, 1], [0, 1, 0], [1, 0, 0]], [0, 0, 0])
_add("sepia", "sepia", SEPIA, [0, 0, 0])
for _s in (0.0, 0.5, 1.5, 2.0):
    _add(f"saturation:{_s}", f"saturation:{_s}", _sat_matrix(_s), [0, 0, 0], q=saturation_q(_s))
_add("ycbcr", "ycbcr", YCBCR, [0, 128, 128])
_add("ycbcr:inv", "ycbcr:inv", YCBCR_INV, YCBCR_INV_B)
_add("mixed", _token(MIXED, MIXED_B), MIXED, MIXED_B)
_add("wide", _token(WIDE, WIDE_B), WIDE, WIDE_B)
_add("wide2", _token(-np.asarray(WIDE), WIDE2_B), -np.asarray(WIDE), WIDE2_B)
NAMES = list(CASES)

CHAINS = ["invert,sepia,brightness:10", "sepia,gaussian5@constant",
          "contrast:1.7," + _token(MIXED, MIXED_B) + ",threshold:90,box3"]

EXTREMES = np.array([0, 1, 254, 255], np.uint8)


def images(rng, shape):
    """Uniform bytes; the byte extremes; constant channels (10, 100, 250)."""
    full = tuple(shape) + (3,)
    const = np.empty(full, np.uint8)
    const[...] = np.array([10, 100, 250], np.uint8)
    return [rng.integers(0, 256, size=full, dtype=np.uint8), rng.choice(EXTREMES, size=full), const]


def mirror(img, q, qb):
    """out_c = sat_u8((sum_k q[c][k] p_k + qb[c] + 2048) >> 12), >> = floor."""
    p = img.astype(np.int64)
    acc = np.einsum("ck,...k->...c", np.asarray(q, np.int64), p) + np.asarray(qb, np.int64) + 2048
    return np.clip(acc >> 12, 0, 255).astype(np.uint8)
