"""The detector filters on the device (csrc/det_filters.hip, ``det_filters.apply`` / ``undo``, the plugins' ``detect``) against the
host statements (``det_filters.apply_host`` / ``undo_masks_host`` / ``detect`` around ``infer``), which tests/test_det_filters.py pins
to the reference's own ``CommonDetector.detect``.  Everything is bytes or integers: no tolerances.

Shapes for the 32-pixel tile: 37 x 53 (both sides off the tile), 64 x 64 (exact tiles), 96 x 160 (bordered to 400: 12.5 tiles), 401 x 33
(bordered to 401: one pixel into a 13th tile, a page narrower than two tiles); B = 1 and B = 3; every combination of the flags."""
import asyncio
import itertools
import warnings

import numpy as np
import pytest
import torch

from manga_image_translator_amd import det_filters as DF

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (64, 64), (96, 160), (401, 33)]
FLAGS = list(itertools.product((False, True), repeat=3))   # rotate, invert, gamma_correct


def _pages(B, h, w, seed=0):
    rng = np.random.default_rng(1000 * h + w + seed)
    pages = rng.integers(0, 256, (B, h, w, 3)).astype(np.uint8)
    if B > 1:
        pages[1] //= 4          # pages of one batch with different means: a table per page
    return pages


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gray_sums_are_exact(cuda, hw, B):
    pages = _pages(B, *hw)
    dev = torch.from_numpy(pages).to(cuda)
    for invert in (False, True):
        want = [int(DF.gray_u8(DF.apply_host(p, False, invert, False)).astype(np.int64).sum()) for p in pages]
        rot = [int(DF.gray_u8(DF.apply_host(p, True, invert, False)).astype(np.int64).sum()) for p in pages]
        assert want == rot                                   # the rotation does not change the sum
        assert DF.gray_sums(dev, invert) == want, (hw, B, invert)
    assert DF.gray_sums(dev[0], False) == [int(DF.gray_u8(DF.apply_host(pages[0], False, False, False)).astype(np.int64).sum())]


def test_gray_sum_needs_its_64_bits(cuda):
    """A white 4200 x 4200 page sums to 255 * 4200^2 = 4 498 200 000 > 2^32."""
    dev = torch.full((1, 4200, 4200, 3), 255, dtype=torch.uint8, device=cuda)
    assert DF.gray_sums(dev, False) == [255 * 4200 * 4200] and DF.gray_sums(dev, True) == [0]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_apply_equals_the_host_statement(cuda, hw, B):
    pages = _pages(B, *hw)
    dev = torch.from_numpy(pages).to(cuda)
    for rotate, invert, gamma in FLAGS:
        want = np.stack([DF.apply_host(p, rotate, invert, gamma) for p in pages])
        got = DF.apply(dev, rotate, invert, gamma)
        assert tuple(got.shape) == want.shape, (hw, B, rotate, invert, gamma)
        assert np.array_equal(got.cpu().numpy(), want), (hw, B, rotate, invert, gamma, int((got.cpu().numpy() != want).sum()))
    assert torch.equal(dev, torch.from_numpy(pages).to(cuda))                      # the source is left alone
    one = DF.apply(dev[0], True, True, True)                                        # [H,W,3] in, [fh,fw,3] out
    assert np.array_equal(one.cpu().numpy(), DF.apply_host(pages[0], True, True, True))


def test_apply_without_a_border(cuda):
    """Pages of 400 px and more: the frame is the page (turned), no border; nothing to do returns the page itself."""
    pages = _pages(2, 400, 431)
    dev = torch.from_numpy(pages).to(cuda)
    assert DF.apply(dev, False, False, False) is dev
    for rotate, invert, gamma in FLAGS[1:]:
        want = np.stack([DF.apply_host(p, rotate, invert, gamma) for p in pages])
        got = DF.apply(dev, rotate, invert, gamma).cpu().numpy()
        assert got.shape == want.shape == ((2, 431, 400, 3) if rotate else (2, 400, 431, 3)) and np.array_equal(got, want), (rotate, invert, gamma)


def test_apply_degenerate_gamma_tables(cuda):
    """mean 0 (a black page of 400 px: every byte becomes 1) and mean 1 ([0, 1, 255, ...])."""
    black = np.zeros((400, 400, 3), np.uint8)
    ones = np.full((400, 400, 3), 1, np.uint8)
    ones[7, 9] = (8, 0, 1)       # gray 1 as well
    for page in (black, ones):
        want = DF.apply_host(page, False, False, True)
        assert np.array_equal(DF.apply(torch.from_numpy(page).to(cuda), False, False, True).cpu().numpy(), want)
    assert (DF.apply_host(black, False, False, True) == 1).all() and tuple(DF.apply_host(ones, False, False, True)[7, 9]) == (255, 0, 1)


@pytest.mark.parametrize("B", [1, 3])
def test_unrotate_u8(cuda, B):
    rng = np.random.default_rng(3)
    for (h, w), (ch, cw) in (((400, 400), (96, 160)), ((53, 37), (53, 37)), ((64, 96), (64, 33)), ((70, 65), (1, 65))):
        maps = rng.integers(0, 256, (B, h, w)).astype(np.uint8)
        want = np.stack([np.rot90(m[:ch, :cw]) for m in maps])
        got = DF.unrotate_u8(torch.from_numpy(maps).to(cuda), ch, cw)
        assert tuple(got.shape) == (B, cw, ch) and np.array_equal(got.cpu().numpy(), want), ((h, w), (ch, cw))
    m = rng.integers(0, 256, (53, 37)).astype(np.uint8)
    assert np.array_equal(DF.unrotate_u8(torch.from_numpy(m).to(cuda), 53, 37).cpu().numpy(), np.rot90(m))


def test_undo_equals_the_host_statement(cuda):
    rng = np.random.default_rng(4)
    for (h, w), rotate in itertools.product([(96, 160), (300, 520), (399, 640), (400, 400), (450, 410)], (False, True)):
        p = DF.plan(h, w, rotate)
        raw, mask = rng.integers(0, 256, (2, p.fh, p.fw)).astype(np.uint8)
        for second in (mask, None):
            want = DF.undo_masks_host(raw, second, h, w, rotate)
            got = DF.undo(torch.from_numpy(raw).to(cuda), None if second is None else torch.from_numpy(second).to(cuda), h, w, rotate)
            for a, b in zip(got, want):
                assert (a is None) == (b is None)
                if b is not None:
                    assert tuple(a.shape) == b.shape and np.array_equal(a.cpu().numpy(), b), (h, w, rotate)
    assert DF.undo_masks_host(raw, None, 96, 160, True)[0].shape == (160, 96)      # the quirk: cropped by the unrotated sizes, then turned


# ---- the plugins -----------------------------------------------------------------------------------------------------------------

def _head_prob(h, w):
    """A trained head's shrink map for any map size: two horizontal lines and a vertical one at fixed fractions of the filtered frame —
    the far one lies in the border of a small page."""
    prob = np.zeros((h, w), np.float32)
    for x0, x1, y0, y1 in ((0.03, 0.30, 0.03, 0.08), (0.05, 0.10, 0.10, 0.22), (0.70, 0.92, 0.80, 0.86)):
        prob[int(y0 * h):int(y1 * h), int(x0 * w):int(x1 * w)] = 0.9
    return prob


@pytest.fixture(scope="module")
def detectors(cuda):
    """The ctd and the ``default`` plugin on seeded weights; their network calls get the stand-in shrink map laid over channel 0 of the
    line map.  The ``default`` plugin's mask stays the network's own; the ctd plugin's is a stand-in made from the page the network was
    given, which ``refine_mask`` then reads together with that page — both depend on the bytes of the filtered page."""
    from manga_image_translator_amd import ctd_schema as S, dbnet_schema, imgproc, plugins as P, synth

    run = asyncio.new_event_loop().run_until_complete
    g = S.CTD_GAIN
    ctd = P.HipComicTextDetector(weights={"ctd.yolo": synth.synth_state_dict(S.yolo_schema(), gain=g), "ctd.seg": synth.synth_state_dict(S.unet_head_schema(), gain=g),
                                          "ctd.det": synth.synth_state_dict(S.db_head_schema(), gain=g)})
    default = P.HipDefaultDetector(weights=synth.synth_state_dict(dbnet_schema.text_detection_schema(), gain=1.2))
    calls = {"ctd": [], "default": []}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        run(ctd.load("cuda"))
        run(default.load("cuda"))
    ctd_plain, db_plain = ctd.engine.forward, default.engine.forward

    def ctd_fwd(pages_u8, taps=None):
        calls["ctd"].append(tuple(pages_u8.shape))
        m8, lines, pad = ctd_plain(pages_u8, taps)
        lines[:, 0] = torch.from_numpy(_head_prob(*lines.shape[-2:])).to(lines.device)
        # seeded weights give an empty text mask: the stand-in is the dark pixels of the page the network was given, at the map's size
        dark = (pages_u8.amin(-1) < 128).to(torch.uint8) * 255
        m8 = imgproc.resize_u8(dark.contiguous(), (int(m8.shape[2]), int(m8.shape[1])))
        return m8, lines, pad

    def db_fwd(pages_u8, taps=None):
        calls["default"].append(tuple(pages_u8.shape))
        db, mask = db_plain(pages_u8, taps)
        db[:, 0] = torch.from_numpy(_head_prob(*db.shape[-2:])).to(db.device)
        return db, mask

    ctd.engine.forward, default.engine.forward = ctd_fwd, db_fwd
    yield {"ctd": ctd, "default": default, "calls": calls, "run": run}
    ctd.engine.forward, default.engine.forward = ctd_plain, db_plain
    run(ctd.unload())
    run(default.unload())


ARGS = (512, 0.5, 0.7, 1.5)     # detect_size, text_threshold, box_threshold, unclip_ratio (ctd ignores all four)


def _same(got, want, what):
    (gl, graw, gmask), (wl, wraw, wmask) = got, want
    assert len(gl) == len(wl) >= 1, what
    for a, b in zip(gl, wl):
        assert np.array_equal(np.asarray(a.pts), np.asarray(b.pts)) and a.prob == b.prob and type(a) is type(b), what
    assert isinstance(graw, np.ndarray) and graw.dtype == np.uint8 and graw.shape == wraw.shape and np.array_equal(graw, wraw), what
    assert (gmask is None) == (wmask is None) and (gmask is None or (gmask.shape == wmask.shape and np.array_equal(gmask, wmask))), what
    assert len(np.unique(wraw)) > 1, what            # a mask that says something


@pytest.mark.parametrize("hw", [(96, 160), (300, 520)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("which", ["ctd", "default"])
def test_plugin_detect_equals_the_host_statements_around_infer(detectors, which, hw):
    from manga_image_translator_amd import synth

    det, run = detectors[which], detectors["run"]
    page = synth.synth_page(21, *hw, n_boxes=3)[0]
    keep = page.copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = run(DF.detect(det.infer, page, *ARGS, True, True, True, False))       # invert, gamma_correct, rotate: all on
        got = run(det.detect(page, *ARGS, True, True, True, False))
    assert np.array_equal(page, keep)
    _same(got, want, (which, hw))
    side = max(max(hw), 400) if which == "ctd" else ARGS[0]     # the ctd engine is handed the bordered frame, DBNet's the frame at detect_size
    assert detectors["calls"][which][-2:] == [(1, side, side, 3)] * 2
    assert want[1].shape == {(96, 160): (160, 96), (300, 520): (520, 300)}[hw]     # cropped by the unrotated sizes, then turned


@pytest.mark.parametrize("which", ["ctd", "default"])
def test_plugin_detect_auto_rotate_runs_again(detectors, which):
    """Two of the three stand-in lines are horizontal: the vote is 'h' and the original page is run again, turned."""
    from manga_image_translator_amd import synth

    det, run, calls = detectors[which], detectors["run"], detectors["calls"][which]
    page = synth.synth_page(22, 450, 410, n_boxes=3)[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        n0 = len(calls)
        want = run(DF.detect(det.infer, page, *ARGS, False, True, False, True))
        n1 = len(calls)
        got = run(det.detect(page, *ARGS, False, True, False, True))
    # two network calls each way: the page, then the page turned (DBNet's engine sees both padded to its square)
    assert calls[n0:n1] == calls[n1:] == ([(1, 450, 410, 3), (1, 410, 450, 3)] if which == "ctd" else [(1, 512, 512, 3)] * 2)
    _same(got, want, which)
    # ctd's mask is page-sized; DBNet's is the network page without its padding (default.py:89-95), here 466 x 512 turned back
    assert got[1].shape == ((450, 410) if which == "ctd" else (512, 466))


def test_plugin_detect_before_load_and_bad_input(detectors):
    from manga_image_translator_amd import plugins as P

    det, run = detectors["default"], detectors["run"]
    with pytest.raises(ValueError, match="expected uint8 RGB"):
        run(det.detect(np.zeros((64, 64, 3), np.float32), *ARGS, False, False, False))
    fresh = P.HipDefaultDetector(weights={})
    with pytest.raises(Exception, match="without having loaded the model"):
        run(fresh.detect(np.zeros((64, 64, 3), np.uint8), *ARGS, False, False, False))
