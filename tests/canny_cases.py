"""Test frames of the canny tests (shared by the CPU and the GPU file): the
frames of integral_cases and their 5 x 5 box means (the smooth ones have real
weak edges), a disc and a ring (every gradient direction), step edges and
two-pixel bars at 0, 45, 90 and 135 degrees in both polarities (plateau ties),
and masks for the hysteresis stage alone."""
import numpy as np

import integral_cases as IC
import np_integral as NI

ANGLES = (0, 45, 90, 135)


def _across(H, W, angle):
    """The coordinate that grows across an edge of the given direction, centred on the frame."""
    yy, xx = np.mgrid[0:H, 0:W]
    if angle == 0:
        return yy - H // 2
    if angle == 90:
        return xx - W // 2
    if angle == 45:
        return (xx - W // 2) + (yy - H // 2)
    return (xx - W // 2) - (yy - H // 2)


def frames(H, W):
    """(name, frame) pairs for an H x W frame."""
    out = list(IC.cases(H, W))
    out += [("blur_" + name, NI.window(a, "box", 5)) for name, a in IC.cases(H, W)]
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = (2 * yy - (H - 1)) ** 2 + (2 * xx - (W - 1)) ** 2  # squared distance from the centre, in half pixels
    r = max(min(H, W) - 2, 1)
    out.append(("disc", np.where(d2 <= r * r, 220, 30).astype(np.uint8)))
    out.append(("ring", np.where((d2 <= r * r) & (d2 > (r * r) // 4), 200, 60).astype(np.uint8)))
    for angle in ANGLES:
        t = _across(H, W, angle)
        for pol, (lo, hi) in (("up", (40, 210)), ("down", (210, 40))):
            out.append((f"step{angle}{pol}", np.where(t >= 0, hi, lo).astype(np.uint8)))
            out.append((f"bar{angle}{pol}", np.where((t == 0) | (t == 1), hi, lo).astype(np.uint8)))
    return out


NAMES = [name for name, _ in frames(2, 2)]


def spiral_path(H, W):
    """The pixels (y, x) of a one-pixel-wide square spiral from (0, 0) inwards, arms one blank pixel apart."""
    seen = np.zeros((H, W), bool)
    y, x, d = 0, 0, 0
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))
    path = [(0, 0)]
    seen[0, 0] = True

    def free(yy, xx):
        return 0 <= yy < H and 0 <= xx < W and not seen[yy, xx]

    def can(dd):
        dy, dx = steps[dd]
        y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        ahead_clear = not (0 <= y2 < H and 0 <= x2 < W) or not seen[y2, x2]
        return free(y1, x1) and ahead_clear

    while True:
        if not can(d):
            d = (d + 1) % 4
            if not can(d):
                break
        y, x = y + steps[d][0], x + steps[d][1]
        seen[y, x] = True
        path.append((y, x))
    return path


def spiral(H, W, strong=True, gap=False):
    """(mask, path, gap index): value 100 along the spiral, 200 at its inner end if strong, one pixel removed from
    the middle of a straight run if gap."""
    path = spiral_path(H, W)
    a = np.zeros((H, W), np.uint8)
    for y, x in path:
        a[y, x] = 100
    if strong:
        a[path[-1]] = 200
    k = None
    if gap:
        k = len(path) // 2
        while not (path[k - 1][0] == path[k + 1][0] or path[k - 1][1] == path[k + 1][1]):
            k += 1  # not at a corner: the two ends must not touch diagonally
        a[path[k]] = 0
    return a, path, k


def staircase(H, W):
    """A diagonal of value 100 from a 200 pixel at (0, 0): one component under 8-connectivity, single pixels under 4."""
    a = np.zeros((H, W), np.uint8)
    n = min(H, W)
    a[np.arange(n), np.arange(n)] = 100
    a[0, 0] = 200
    return a
