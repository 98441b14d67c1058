"""Test frames of the integral-image tests (shared by the CPU and the GPU file)."""
import numpy as np


def text_on_gradient(H, W):
    """Two levels of "ink" on a left-to-right illumination ramp: what a global threshold gets wrong."""
    yy, xx = np.mgrid[0:H, 0:W]
    paper = 60 + (xx * 180) // max(W - 1, 1)
    ink = ((yy // 2 + xx // 3) % 5 == 0) | ((yy % 7 == 3) & (xx % 4 < 2))
    return np.where(ink, paper // 3, paper).astype(np.uint8)


def cases(H, W, seed=0):
    """(name, frame) pairs for an H x W frame."""
    rng = np.random.default_rng(1000 * H + W + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = [(f"flat{v}", np.full((H, W), v, np.uint8)) for v in (0, 1, 127)]
    out.append(("all255", np.full((H, W), 255, np.uint8)))
    out.append(("random", rng.integers(0, 256, (H, W), dtype=np.uint8)))
    out.append(("ramp", ((xx * 3 + yy * 5) % 256).astype(np.uint8)))
    out.append(("checker", (((xx + yy) % 2) * 255).astype(np.uint8)))
    a = np.zeros((H, W), np.uint8)
    a[H // 2, W // 3] = 255
    out.append(("one_bright", a))
    out.append(("text", text_on_gradient(H, W)))
    return out


NAMES = [name for name, _ in cases(2, 2)]
