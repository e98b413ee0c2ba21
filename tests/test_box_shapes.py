"""The capacity-limit maps of tests/_box_shapes.py have the border statistics they claim, counted without the GPU kernel: total points
through the native host contour count, per-border points and corners through the test oracle's border following (oracle/contours.py)
with the kernel's corner rule.  The GPU tests that probe BFB_CAP / BFB_HCAP of csrc/ctd_boxes.hip rely on these counts."""
import numpy as np
import pytest

import _box_shapes as S


@pytest.mark.parametrize("cut,points", [(2, 8192), (1, 8193)])
@pytest.mark.parametrize("shift", [0, 9])
def test_comb_has_exactly_the_point_cap_or_one_more(cut, points, shift):
    from manga_image_translator_amd import hostglue as HG

    bm = S.comb_points(cut, shift) > 0.3
    assert HG.contour_count(bm) == (1, points)
    [(n, corners)] = S.contour_stats(bm)
    assert n == points and corners <= 4096


@pytest.mark.parametrize("corners", [4096, 4097])
def test_band_has_exactly_the_corner_cap_or_one_more(corners):
    from manga_image_translator_amd import hostglue as HG

    bm = S.band_corners(corners) > 0.3
    n_borders, n_points = HG.contour_count(bm)
    [(n, c)] = S.contour_stats(bm)
    assert n_borders == 1 and n_points == n <= 8192
    assert c == corners


def test_corner_rule_on_small_shapes():
    """The corner count itself: a filled rectangle turns at its four corners only, a crenellated edge at every point, and a contour of
    fewer than three points keeps all of them."""
    m = np.zeros((8, 12), np.uint8)
    m[2:6, 3:10] = 1
    assert S.contour_stats(m) == [(2 * 7 + 2 * 4 - 4, 4)]
    m[2, 4:10:2] = 0                      # crenellated top edge: (4, 2) (5, 3) (6, 2) (7, 3) (8, 2) (9, 3) all turn
    [(n, c)] = S.contour_stats(m)
    assert (n, c) == (18, 9)
    one = np.zeros((3, 3), np.uint8)
    one[1, 1] = 1
    assert S.contour_stats(one) == [(1, 1)]


def test_offset_page_reaches_the_key_range_at_the_edge_ratio():
    """Box of the offset page and the unclip ratio at which its round-join polygon touches x = 32768 (host arithmetic of the box)."""
    from manga_image_translator_amd import hostglue as HG

    page = S.offset_page()
    a, b = S.OFF_BOX
    boxes, scores = HG.boxes_from_bitmap(page, 0.3, S.OFF_HW, S.OFF_HW, unclip_ratio=1.0, min_sside=2.0)
    assert len(boxes) == 1 and scores[0] == pytest.approx(0.9, abs=1e-6)
    side = b - a
    r = S.offset_edge_ratio()
    assert b + side * r / 4 == pytest.approx(32768, abs=1e-6)
    assert HG.contour_count(page > 0.3) == (1, 4 * side)


def test_dots_page_has_more_borders_than_max_candidates():
    from manga_image_translator_amd import hostglue as HG

    n, _ = HG.contour_count(S.dots() > 0.3)
    assert n > 1000
