"""Deterministic saturated and structured test images.

Uniform noise checks tiling, borders and halos, but it almost never produces
the windows on which the packed 16-bit arithmetic of the kernels has the least
headroom (a saturated 5x5 window, a 0/255 alternation, gray values 0 and 254)
or a single pixel next to a tile seam.  `patterns(H, W, C)` yields
`(label, image)` for those: HxW uint8 for C = 1, HxWx3 for C = 3.  For C = 3
every pattern comes twice, the same in all channels ("/same") and with a phase
shift per channel ("/shift"), so that a channel mix-up shows.
"""
from __future__ import annotations

import numpy as np

UNIFORM = (0, 1, 127, 128, 254, 255)
EXTREMES = np.array([0, 1, 254, 255], np.uint8)
# wave-tile seams of a row, in bytes: every multiple of 992 (16 B x the 62
# output chunks of a k_sep / k_direct / k_rank wave) and of 1024 (gray k_sobel_rp)
SEAMS = (992, 1024)
MIN_GAP = 8  # impulses sharing a frame: further apart than any window (K <= 7)

HEIGHTS = (1, 2, 5, 13)  # 13: past the 4-row group, a remainder in 8- and 12-row bands
# row bytes on either side of the seams: 991 / 993 / 1025 / 2049 (gray), 993 / 1026 / 2049 (RGB)
WIDTHS = {1: (991, 993, 1025, 2049), 3: (331, 342, 683)}
TINY = ((1, 1), (2, 3), (3, 2), (5, 70))  # the first three are border only


def shapes(C):
    """(H, W) of the frames the device kernels are run on."""
    return [(h, w) for h in HEIGHTS for w in WIDTHS[C]] + list(TINY)


def host_shapes(C):
    """A subset for the host-side suites: the tiny frames, a 13-row frame and one row past a seam."""
    return list(TINY) + [(13, 70), (5, WIDTHS[C][1] if C == 1 else WIDTHS[C][0])]


def _checker(H, W, phase):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy + xx + phase) & 1) * 255).astype(np.uint8)


def _cols(H, W, phase):
    return np.broadcast_to((((np.arange(W) + phase) & 1) * 255).astype(np.uint8), (H, W)).copy()


def _rows(H, W, phase):
    return np.broadcast_to((((np.arange(H) + phase) & 1) * 255).astype(np.uint8)[:, None], (H, W)).copy()


def _half_lr(H, W, phase):
    # step edge at W / 2 (+ phase); odd phases swap the bright side
    img = np.zeros((H, W), np.uint8)
    img[:, min(W, W // 2 + phase):] = 255
    return img if phase % 2 == 0 else 255 - img


def _half_tb(H, W, phase):
    img = np.zeros((H, W), np.uint8)
    img[min(H, H // 2 + phase):, :] = 255
    return img if phase % 2 == 0 else 255 - img


def impulse_sites(H, W, C, seams=SEAMS):
    """(y, x, channel) of the impulses: corners, centre, and the pixel holding
    the last byte before / the first byte after every seam inside the row
    (`seams`: the seam periods in bytes)."""
    sites = [(H // 2, W // 2, 0), (0, 0, 1), (0, W - 1, 2), (H - 1, 0, 2), (H - 1, W - 1, 1)]
    k = 0
    for period in seams:
        for s in range(period, W * C, period):
            y = (3 + 4 * k) % H
            k += 1
            for b in (s - 1, s):
                sites.append((y, b // C, b % C))
    seen, out = set(), []
    for y, x, c in sites:
        if (y, x) not in seen:
            seen.add((y, x))
            out.append((y, x, c % C))
    return out


def _pack(sites):
    """Greedy split into frames whose impulses lie >= MIN_GAP apart (Chebyshev)."""
    frames = []
    for s in sites:
        for f in frames:
            if all(max(abs(s[0] - t[0]), abs(s[1] - t[1])) >= MIN_GAP for t in f):
                f.append(s)
                break
        else:
            frames.append([s])
    return frames


def _three(fn, H, W, shift):
    return np.stack([fn(H, W, c if shift else 0) for c in range(3)], axis=-1)


def patterns(H, W, C, seed=7, seams=SEAMS):
    assert C in (1, 3)
    rng = np.random.default_rng(seed)
    variants = (("", False),) if C == 1 else (("/same", False), ("/shift", True))
    for tag, shift in variants:
        for i, v in enumerate(UNIFORM):
            if C == 1:
                yield f"uniform{v}", np.full((H, W), v, np.uint8)
            else:
                vals = [UNIFORM[(i + 2 * c) % len(UNIFORM)] if shift else v for c in range(3)]
                yield f"uniform{v}{tag}", np.broadcast_to(np.array(vals, np.uint8), (H, W, 3)).copy()
        for name, fn, phases in (("checker", _checker, (0, 1)), ("colstripes", _cols, (0,)), ("rowstripes", _rows, (0,)),
                                 ("half_lr", _half_lr, (0,)), ("half_tb", _half_tb, (0,))):
            for ph in phases:
                def one(h, w, c, fn=fn, ph=ph):
                    return fn(h, w, ph + c)
                yield f"{name}{ph}{tag}", one(H, W, 0) if C == 1 else _three(one, H, W, shift)
        if C == 1 or shift:
            yield f"extremes{tag}", rng.choice(EXTREMES, size=(H, W) if C == 1 else (H, W, 3))
        else:
            yield f"extremes{tag}", np.repeat(rng.choice(EXTREMES, size=(H, W))[..., None], 3, axis=-1)
        for bg, fg, name in ((0, 255, "impulse255on0"), (255, 0, "impulse0on255")):
            for n, frame in enumerate(_pack(impulse_sites(H, W, C, seams))):
                img = np.full((H, W) if C == 1 else (H, W, 3), bg, np.uint8)
                for y, x, c in frame:
                    if C == 1:
                        img[y, x] = fg
                    elif shift:
                        img[y, x, c] = fg
                    else:
                        img[y, x, :] = fg
                yield f"{name}.{n}{tag}", img


def saturated(H, W, C):
    """The frames the fused forms run on: all-255, both checkerboards, the draw from {0, 1, 254, 255}."""
    keep = ("uniform255", "checker", "extremes")
    return [(l, im) for l, im in patterns(H, W, C) if l.startswith(keep)]
