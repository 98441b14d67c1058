"""numpy mirror of the resize rule (csrc/include/stripe/resize.h), written from
its text, not from the C++: integer taps per axis, horizontal pass to 8.8 fixed
point, vertical pass to a byte.  Also the float64 reference: the same geometry
with real-valued weights and one rounding at the end.

taps(n_in, n_out, mode) -> (first, count, weights): weights is a list of
int64 arrays, one per output index.
"""
from fractions import Fraction

import numpy as np

ONE = 32768
MAX_FACTOR = 32


def resolve(n_in, n_out, mode):
    if mode != "auto":
        return mode
    return "area" if n_out < n_in else "bilinear" if n_out > n_in else "nearest"


def taps(n_in, n_out, mode, real=False):
    """Integer Q15 taps (real=False) or exact Fractions summing to 1 (real=True)."""
    mode = resolve(n_in, n_out, mode)
    first, count, weights = [], [], []
    for o in range(n_out):
        if mode == "nearest":
            f, w = ((2 * o + 1) * n_in) // (2 * n_out), [Fraction(1)]
            q = [ONE]
        elif mode == "bilinear":
            num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
            i0 = num // den  # python floors, also for negative num
            r = num - i0 * den
            w1 = (65536 * r + den) // (2 * den)
            a, b = min(max(i0, 0), n_in - 1), min(max(i0 + 1, 0), n_in - 1)
            if a == b:
                f, w, q = a, [Fraction(1)], [ONE]
            else:
                f, w, q = a, [1 - Fraction(r, den), Fraction(r, den)], [ONE - w1, w1]
        elif mode == "area":
            if n_out > n_in:
                raise ValueError("area cannot grow an axis")
            if n_in > MAX_FACTOR * n_out:
                raise ValueError("area factor above 32")
            c0, c1 = o * n_in, (o + 1) * n_in
            lo, hi = c0 // n_out, (c1 - 1) // n_out
            L = [min(c1, (i + 1) * n_out) - max(c0, i * n_out) for i in range(lo, hi + 1)]
            assert sum(L) == n_in and min(L) > 0
            f, w = lo, [Fraction(l, n_in) for l in L]
            q = [(ONE * l) // n_in for l in L]
            rem = [(ONE * l) % n_in for l in L]
            order = sorted(range(len(L)), key=lambda k: (-rem[k], k))
            for k in order[: ONE - sum(q)]:
                q[k] += 1
        else:
            raise ValueError(f"unknown mode {mode}")
        first.append(f)
        count.append(len(q))
        weights.append(w if real else np.array(q, dtype=np.int64))
    return np.array(first), np.array(count), weights


def _matrix(n_in, n_out, mode, real):
    f, c, w = taps(n_in, n_out, mode, real)
    M = np.zeros((n_out, n_in), dtype=np.float64 if real else np.int64)
    for o in range(n_out):
        M[o, f[o]:f[o] + c[o]] = [float(v) for v in w[o]] if real else w[o]
    return M


def resize(img, W2, H2, mode="auto"):
    """The rule, bit for bit: HxW or HxWxC uint8 -> H2xW2[xC] uint8."""
    a = img.astype(np.int64)
    Mx, My = _matrix(a.shape[1], W2, mode, False), _matrix(a.shape[0], H2, mode, False)
    h = (np.tensordot(Mx, a, axes=([1], [1])) + 64) >> 7  # (W2, H[, C])
    assert h.max(initial=0) <= 65280
    out = (np.tensordot(My, h, axes=([1], [1])) + (1 << 22)) >> 23  # (H2, W2[, C])
    assert out.max(initial=0) <= 255
    return out.astype(np.uint8)


def resize_real(img, W2, H2, mode="auto"):
    """Same geometry, real-valued weights, float64, not rounded."""
    a = img.astype(np.float64)
    Mx, My = _matrix(a.shape[1], W2, mode, True), _matrix(a.shape[0], H2, mode, True)
    h = np.tensordot(Mx, a, axes=([1], [1]))
    return np.tensordot(My, h, axes=([1], [1]))


def bound(Tx, Ty):
    """|out - real| <= 0.5 + 2^-9 + 127.5 (Tx + Ty) 2^-15 for the largest tap counts Tx, Ty."""
    return 0.5 + 2.0 ** -9 + 127.5 * (Tx + Ty) * 2.0 ** -15
