"""Probability maps whose one border sits exactly at a capacity limit of the GPU box extraction (csrc/ctd_boxes.hip: BFB_CAP = 8192
contour points and BFB_HCAP = 4096 corner points per border, held in one workgroup's LDS), and at the edge of the round-join offset's
16-bit key range.  The counts are asserted independently of the kernel by tests/test_box_shapes.py; the GPU tests in
tests/test_ctd_boxes_gpu.py probe the caps with them.

A border of a filled w x h rectangle (w, h >= 3) has 2w + 2h - 4 points, and taking away a convex corner pixel replaces two unit steps
by one diagonal step: one point less.  A point is a corner unless its incoming and outgoing steps are equal (the kernel's rule); a
crenellated edge (every other pixel of the row taken away) turns at every point, so a band of width L with both long edges
crenellated has a corner at almost every one of its ~2L points while staying far under the point cap."""
from __future__ import annotations

import numpy as np

ON = np.float32(0.9)          # inside the shape: above every threshold used (0.3) and every box threshold (0.6, 0.7)
H, W = 160, 2200              # the map of the point / corner pages (one batch holds all of them; boxes clear of its frame)

# the point pages: a comb, a spine of SPINE = (y0, x0, h, w) with 2-pixel teeth hanging from it every 40 columns; its one border has
# 2 (w + h) - 4 points for the spine plus 2 t - 2 per tooth of length t: 4122 + 50 x 80 + 72 = 8194
SPINE = (56, 60, 4, 2059)
TEETH = [41] * 50 + [37]
BAND = (70, 16, 6)            # (y0, x0, h) of the crenellated band of the corner pages


def comb_points(cut: int, shift: int = 0) -> np.ndarray:
    """The comb with ``cut`` (1 or 2) convex corner pixels of its spine taken away: one border of 8194 - cut points (8193 or 8192).
    ``shift`` moves it right (a different map with the same border statistics)."""
    if cut not in (1, 2):
        raise ValueError(cut)
    y0, x0, h, w = SPINE
    x0 += shift
    m = np.zeros((H, W), np.float32)
    m[y0:y0 + h, x0:x0 + w] = ON
    for i, t in enumerate(TEETH):
        m[y0 + h:y0 + h + t, x0 + 2 + 40 * i:x0 + 4 + 40 * i] = ON
    m[y0, x0] = 0                                   # top-left corner of the spine
    if cut == 2:
        m[y0 + h - 1, x0 + w - 1] = 0               # bottom-right corner of the spine (no tooth there)
    return m


def band_corners(corners: int) -> np.ndarray:
    """A 6-pixel-high band with both long edges crenellated: one border with exactly ``corners`` (4096 or 4097) corner points and
    ~4100 points.  Width 2048 gives 4096; width 2047 gives 4094, and a one-pixel bump on the left side adds three."""
    if corners not in (4096, 4097):
        raise ValueError(corners)
    y0, x0, h = BAND
    L = 2048 if corners == 4096 else 2047
    m = np.zeros((H, W), np.float32)
    m[y0:y0 + h, x0:x0 + L] = ON
    m[y0, x0 + 1:x0 + L:2] = 0
    m[y0 + h - 1, x0 + 1:x0 + L:2] = 0
    if corners == 4097:
        m[y0 + 2, x0 - 1] = ON
    return m


def dots(step: int = 6, size: int = 4) -> np.ndarray:
    """size x size squares every ``step`` pixels: far more borders (~9900) than max_candidates (1000), most of
    them a box."""
    m = np.zeros((H, W), np.float32)
    for k in range(size):
        for j in range(size):
            m[1 + k:H - 1:step, 1 + j:W - 1:step] = ON
    return m


# the offset page: one square box; the round join reaches x1 + delta, delta = area * ratio / length = side * ratio / 4
OFF_HW = 512
OFF_BOX = (16, 495)           # first and last row / column of the square


def offset_page() -> np.ndarray:
    a, b = OFF_BOX
    m = np.zeros((OFF_HW, OFF_HW), np.float32)
    m[a:b + 1, a:b + 1] = ON
    return m


def offset_edge_ratio() -> float:
    """The unclip ratio at which the offset polygon's right / bottom edge reaches x = 32768, the first coordinate outside the
    kernel's 16-bit keys (the box of a pixel square is its pixel centres: side b - a, area side^2, length 4 side)."""
    a, b = OFF_BOX
    return (32768 - b) / ((b - a) / 4.0)


def contour_stats(bitmap: np.ndarray):
    """Per border of ``bitmap`` (through the test oracle's border following, on the tight crop around the set pixels plus a 1-pixel
    margin): (points, corners), corners by the kernel's rule (n >= 3: a point whose incoming and outgoing steps differ)."""
    from oracle.contours import find_contours_list

    ys, xs = np.nonzero(bitmap)
    crop = bitmap[max(ys.min() - 1, 0):ys.max() + 2, max(xs.min() - 1, 0):xs.max() + 2]
    out = []
    for c in find_contours_list(crop):
        p = c.reshape(-1, 2).astype(np.int64)
        n = len(p)
        if n < 3:
            out.append((n, n))
            continue
        straight = ((p - np.roll(p, 1, axis=0)) == (np.roll(p, -1, axis=0) - p)).all(axis=1)
        out.append((n, int((~straight).sum())))
    return out
