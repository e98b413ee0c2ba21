"""The detector filters (``det_filters``: rotate, border, invert, gamma around a detector, detection/common.py:12-64) — no GPU needed:

* ``det_filters.detect`` with the host statements against tests/golden/det_filters.npz, which holds what the reference's OWN
  ``CommonDetector.detect`` returned around the same stand-in network: five pages (96x160, 300x520 and 399x640 get the border, 400x400
  does not, 450x410), all eight combinations of rotate / invert / gamma, and the three auto-rotate outcomes.  Where the reference is
  present every case is run through it again and compared array by array;
* ``gamma_lut`` against the reference's statement applied to whole pages, the degenerate means included;
* ``plan`` at the 399 / 400 boundary;
* every refusal of the three C entries, with a fake pointer that is never dereferenced."""
import asyncio

import numpy as np
import pytest

from manga_image_translator_amd import det_filters as DF
from manga_image_translator_amd.textline import Quadrilateral

from _det_filters_cases import gen, golden

CASE_IDS = [c[0] for c in gen.CASES]


@pytest.fixture(scope="module")
def fixture():
    return golden()


def _run(case, quad_cls=Quadrilateral):
    name, h, w, rotate, invert, gamma, auto, kind = case
    net = gen.StubNet(quad_cls, kind, gen.with_mask(h, w, rotate, invert))
    page = gen.page(h, w)
    keep = page.copy()
    res = asyncio.run(DF.detect(net, page, *gen.DETECT_ARGS, invert, gamma, rotate, auto))
    assert np.array_equal(page, keep), "detect must leave the caller's page alone"
    assert all(a == gen.DETECT_ARGS + (False,) for a in net.args)
    return (net,) + tuple(res)


@pytest.mark.parametrize("case", gen.CASES, ids=CASE_IDS)
def test_detect_equals_the_reference_fixture(case, fixture):
    name = case[0]
    got = {}
    gen.pack(name, got, *_run(case))
    want = {k: v for k, v in fixture.items() if k.startswith(name + "/")}
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def test_fixture_covers_what_it_should(fixture):
    """The outcomes are asserted on the fixture, so a change of the generator cannot quietly lose one."""
    n = lambda name: int(fixture[name + "/n_pages"])
    for (h, w), r in (((96, 160), False), ((450, 410), True)):
        tag = f"p{h}x{w}_r{int(r)}"
        assert n(f"auto_v_{tag}") == 1 and n(f"auto_h_{tag}") == 2 and n(f"auto_none_{tag}") == 2
        assert len(fixture[f"auto_none_{tag}/pts"]) == 0 and len(fixture[f"auto_v_{tag}/pts"]) == 3
    # the quirk: a rotated, bordered 96 x 160 page comes back with masks of (160, 96) and negative ordinates
    assert tuple(fixture["p96x160_r1i0g0/raw_shape"]) == (160, 96) and fixture["p96x160_r1i0g0/pts"][..., 1].min() == -64
    assert tuple(fixture["p96x160_r0i0g0/page0_shape"]) == (400, 400, 3) and tuple(fixture["p400x400_r0i0g0/page0_shape"]) == (400, 400, 3)
    assert tuple(fixture["p399x640_r1i1g1/page0_shape"]) == (640, 640, 3) and tuple(fixture["p450x410_r1i0g0/page0_shape"]) == (410, 450, 3)
    # of seven lines: area 1 dropped everywhere; on the small page the far corner and the middle lie beyond both sizes and go as well
    assert len(fixture["p450x410_r0i0g0/pts"]) == 6 and len(fixture["p96x160_r0i0g0/pts"]) == 4
    assert fixture["p96x160_r0i0g0/pts"][..., 0].max() == 160                      # the line right of the page: kept, clipped to the width
    assert {bool(fixture[c[0] + "/has_mask"]) for c in gen.CASES} == {True, False}


def test_detect_equals_the_reference_run_again():
    """Where the reference is present: every case through its own detect, compared in full (not by digest)."""
    from oracle import ref_import

    if not ref_import.available():
        pytest.skip("the reference checkout is not on this machine")
    det, quad_cls = gen.reference_detector()
    for case in gen.CASES:
        rnet, rl, rraw, rmask = gen.reference_detect(det, quad_cls, case)
        net, l, raw, mask = _run(case)
        assert len(net.pages) == len(rnet.pages) and all(np.array_equal(a, b) for a, b in zip(net.pages, rnet.pages)), case[0]
        assert len(l) == len(rl) and all(np.array_equal(a.pts, b.pts) and a.prob == b.prob for a, b in zip(l, rl)), case[0]
        assert raw.shape == rraw.shape and np.array_equal(raw, rraw), case[0]
        assert (mask is None) == (rmask is None) and (mask is None or (mask.shape == rmask.shape and np.array_equal(mask, rmask))), case[0]


def test_undo_host_is_remove_border_then_remove_rotation(fixture):
    h, w = 96, 160
    net = gen.StubNet(Quadrilateral, "mixed", True)
    lines, raw, mask = net(DF.apply_host(gen.page(h, w), True, False, False))
    lines = [t for t in lines if t.area > 1]
    lines, raw, mask = DF.undo_host(lines, raw, mask, h, w, True)
    assert np.array_equal(np.array([t.pts for t in lines]), fixture["p96x160_r1i0g0/pts"])
    assert np.array_equal(gen.digest(raw), fixture["p96x160_r1i0g0/raw_sha"]) and mask.shape == (160, 96) and mask.flags.c_contiguous


def _reference_gamma(image):
    """_add_gamma_correction (detection/common.py:118-124) on a whole page, gray in the project's fixed-point form."""
    with np.errstate(all="ignore"):
        gray = DF.gray_u8(image)
        mean = np.mean(gray)
        gamma = np.log(0.5 * 255) / np.log(mean)
        return np.power(image, gamma).clip(0, 255).astype(np.uint8)


def _by_table(image):
    gray = DF.gray_u8(image)
    return DF.gamma_lut(int(gray.astype(np.int64).sum()), gray.size)[image]


@pytest.mark.parametrize("name", ["noise", "zeros", "ones", "inverted_border", "dark", "bright"])
def test_gamma_lut_equals_the_statement_on_whole_pages(name):
    rng = np.random.default_rng(5)
    if name == "zeros":
        page = np.zeros((64, 48, 3), np.uint8)
    elif name == "ones":
        page = np.full((400, 400, 3), 1, np.uint8)
        page[3, 5] = (8, 0, 1)     # the table has more than one entry to get right (its gray value is 1 as well: the mean stays 1)
        assert DF.gray_u8(page).min() == 1 == DF.gray_u8(page).max()
    elif name == "inverted_border":
        page = DF.apply_host(gen.page(96, 160), False, True, False)
        assert page.shape == (400, 400, 3) and page[399, 399, 0] == 255
    elif name == "dark":
        page = rng.integers(0, 3, (50, 70, 3)).astype(np.uint8)   # mean below 1: a negative exponent
    elif name == "bright":
        page = rng.integers(200, 256, (50, 70, 3)).astype(np.uint8)
    else:
        page = rng.integers(0, 256, (123, 77, 3)).astype(np.uint8)
    assert np.array_equal(_by_table(page), _reference_gamma(page))
    if min(page.shape[:2]) >= 400:     # no border gets in the way: the host statement itself
        assert np.array_equal(DF.apply_host(page, False, False, True), _reference_gamma(page))


def test_gamma_lut_degenerate_means():
    assert np.array_equal(DF.gamma_lut(0, 1000), np.ones(256, np.uint8))
    assert np.array_equal(DF.gamma_lut(1000, 1000), np.array([0, 1] + [255] * 254, np.uint8))
    mid = DF.gamma_lut(int(127.5 * 1000), 1000)        # mean 127.5: gamma 1, the identity up to the truncation of the power
    assert mid[0] == 0 and mid[255] in (254, 255) and np.all(np.abs(mid.astype(int) - np.arange(256)) <= 1)


def test_plan_at_the_boundary():
    assert DF.plan(399, 640, False) == (True, 640, 640, 640) and DF.plan(399, 640, True) == (True, 640, 640, 640)
    assert DF.plan(640, 399, False) == (True, 640, 640, 640)
    assert DF.plan(400, 400, False) == (False, 0, 400, 400)
    assert DF.plan(400, 1000, True) == (False, 0, 1000, 400) and DF.plan(400, 1000, False) == (False, 0, 400, 1000)
    assert DF.plan(96, 160, True) == (True, 400, 400, 400) and DF.plan(399, 399, False) == (True, 400, 400, 400)
    assert DF.plan(399, 401, True) == (True, 401, 401, 401)
    with pytest.raises(ValueError):
        DF.plan(0, 10, False)


def test_host_and_device_forms_refuse_the_wrong_input():
    with pytest.raises(ValueError):
        DF.apply_host(np.zeros((8, 8, 3), np.float32), False, False, False)
    with pytest.raises(ValueError):
        DF.apply_host(np.zeros((8, 8), np.uint8), False, False, False)
    import torch

    with pytest.raises(ValueError, match="device tensors"):
        DF.apply(torch.zeros(8, 8, 3, dtype=torch.uint8), True, False, False)
    with pytest.raises(ValueError):
        DF.apply(np.zeros((8, 8, 3), np.uint8), True, False, False)


def test_entries_refuse_bad_arguments_before_any_hip_call():
    from manga_image_translator_amd import lib

    L = lib.load()
    fake = 4096      # never dereferenced: every call below is refused by the argument checks
    err = lambda: L.mit_last_error()
    # mit_det_filter_gray_sum(pages, B, H, W, side, invert, sums, stream)
    assert L.mit_det_filter_gray_sum(None, 1, 8, 8, 0, 0, fake, None) != 0 and b"null pointer" in err()
    assert L.mit_det_filter_gray_sum(fake, 1, 8, 8, 0, 0, None, None) != 0 and b"null pointer" in err()
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert L.mit_det_filter_gray_sum(fake, B, H, W, 0, 0, fake, None) != 0 and b"must be positive" in err(), (B, H, W)
    assert L.mit_det_filter_gray_sum(fake, 1, 96, 160, 159, 0, fake, None) != 0 and b"smaller than the frame" in err()
    assert L.mit_det_filter_gray_sum(fake, 1, 96, 160, -1, 0, fake, None) != 0 and b"smaller than the frame" in err()
    assert L.mit_det_filter_gray_sum(fake, 1, 96, 160, 400, 0, fake + 4, None) != 0 and b"8-byte aligned" in err()
    assert L.mit_det_filter_gray_sum(fake, 1, 40000, 8, 0, 0, fake, None) != 0 and b"sides up to" in err()
    # mit_det_filter_apply(src, B, H, W, rotate, side, invert, lut, dst, stream): a null lut is no error, it means no gamma
    assert L.mit_det_filter_apply(None, 1, 8, 8, 1, 0, 0, None, fake, None) != 0 and b"null pointer" in err()
    assert L.mit_det_filter_apply(fake, 1, 8, 8, 1, 0, 0, None, None, None) != 0 and b"null pointer" in err()
    for B, H, W in ((0, 8, 8), (1, -3, 8), (1, 8, 0)):
        assert L.mit_det_filter_apply(fake, B, H, W, 0, 0, 0, None, 2 * fake, None) != 0 and b"must be positive" in err(), (B, H, W)
    assert L.mit_det_filter_apply(fake, 1, 401, 33, 1, 400, 0, None, 2 * fake, None) != 0 and b"smaller than the frame" in err()
    assert L.mit_det_filter_apply(fake, 1, 8, 8, 1, 0, 0, None, fake, None) != 0 and b"over its source" in err()
    assert L.mit_det_filter_apply(fake, 70000, 8, 8, 1, 0, 0, None, 2 * fake, None) != 0 and b"at most 65535" in err()
    # mit_det_unrotate_u8(maps, B, h, w, ch, cw, out, stream)
    assert L.mit_det_unrotate_u8(None, 1, 8, 8, 8, 8, fake, None) != 0 and b"null pointer" in err()
    assert L.mit_det_unrotate_u8(fake, 1, 8, 8, 8, 8, None, None) != 0 and b"null pointer" in err()
    for B, h, w, ch, cw in ((0, 8, 8, 8, 8), (1, 0, 8, 8, 8), (1, 8, -8, 8, 8), (1, 8, 8, 0, 8), (1, 8, 8, 8, -1)):
        assert L.mit_det_unrotate_u8(fake, B, h, w, ch, cw, 2 * fake, None) != 0 and b"must be positive" in err(), (B, h, w, ch, cw)
    assert L.mit_det_unrotate_u8(fake, 1, 8, 16, 9, 16, 2 * fake, None) != 0 and b"outside the map" in err()
    assert L.mit_det_unrotate_u8(fake, 1, 8, 16, 8, 17, 2 * fake, None) != 0 and b"outside the map" in err()
    assert L.mit_det_unrotate_u8(fake, 1, 8, 8, 8, 8, fake, None) != 0 and b"over its source" in err()
