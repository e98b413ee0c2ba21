"""The ``--ignore-bubble`` rules on the device (csrc/bubble.hip) against their host statements, byte for byte: ``mit_bubble_filter``
(``GpuMaskBackend.bubble_filter``) against ``mask_refinement.bubble_filter``, ``mit_bubble_crop_flags`` (``textline.bubble_crop_flags``)
against ``textline.is_ignore`` per crop, and the option carried through ``dispatch_device`` / ``dispatch_sync``, the ctc and 32px OCR
plugins and ``CoupledPageEngine.run``.  There are no tolerances: every comparison is ``np.array_equal``.  The host statements are
pinned to the reference by tests/test_mask_refinement.py and tests/test_ocr32_cpu.py.

Every group of cases also asserts ON THE ORACLE that both outcomes occur (something erased / rejected and something kept), so a kernel
that does nothing, or that clears everything, cannot pass."""
import asyncio
import types
import warnings

import numpy as np
import pytest
import torch
from scipy import ndimage as nd

from manga_image_translator_amd import mask_refinement as MR, textline as TL

pytestmark = pytest.mark.gpu

RED = (255, 0, 0)


@pytest.fixture(scope="module")
def be(cuda):
    return MR.GpuMaskBackend(cuda)


def _device(be, mask, page, level):
    out = be.bubble_filter(torch.from_numpy(mask).to(be.device), torch.from_numpy(page).to(be.device), level)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == mask.shape
    return out.cpu().numpy()


def _outcomes(mask, want):
    """(components the oracle erased, components it kept): the external contours of the dilated mask, looked up in the oracle's output."""
    H, W = mask.shape
    k = int(max(H, W) * 0.025)
    dil = MR.dilate(mask, np.ones((k, k), np.uint8)) if k > 0 else mask
    labels, n = nd.label(nd.binary_fill_holes(dil > 0), structure=np.ones((3, 3)))
    own = nd.maximum(want, labels, index=np.arange(1, n + 1)) if n else np.zeros(0)
    erased = int((np.asarray(own) == 0).sum())
    return erased, n - erased


def _check(be, mask, page, level):
    want = MR.bubble_filter(mask.copy(), page, level)
    got = _device(be, mask, page, level)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ at {mask.shape}, level {level}"
    return want


def _grey(shape, value):
    return np.full(shape + (3,), value, np.uint8)


# ---- random masks -----------------------------------------------------------------------------------------------------------

SIZES = ((37, 33), (96, 80), (200, 120), (256, 192))     # k = 0, 2 (even anchor), 5, 6
LEVELS = (1, 10, 40, 50)
_RANDOM = {}


def _random_case(H, W, density, level):
    key = (H, W, density, level)
    if key not in _RANDOM:
        rng = np.random.default_rng([H, W, int(density * 100), level])
        mask = np.where(rng.random((H, W)) < density, 255, 0).astype(np.uint8)
        if density > 0.1:                        # dense masks: knock windows out so that the dilated mask is several pieces with holes
            for _ in range(6):
                y, x = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
                mask[y:y + int(rng.integers(8, H // 2)), x:x + int(rng.integers(8, W // 2))] = 0
        g = rng.integers(0, 256, (H, W), dtype=np.uint8)
        g[:, :W // 3] = np.minimum(g[:, :W // 3], 100)       # a dark third: rectangles there see a dark frame
        page = np.repeat(g[..., None], 3, axis=2)
        for _ in range(3):                       # a few coloured pixels: clusters of 12 and single ones
            y, x = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 4))
            page[y:y + 3, x:x + 4] = RED
        for _ in range(5):
            page[int(rng.integers(0, H)), int(rng.integers(0, W))] = (0, 200, 30)
        want = MR.bubble_filter(mask.copy(), page, level)
        _RANDOM[key] = (mask, page, want, _outcomes(mask, want))
    return _RANDOM[key]


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("density", (0.02, 0.30))
@pytest.mark.parametrize("H,W", SIZES)
def test_random_masks(be, H, W, density, level):
    mask, page, want, _ = _random_case(H, W, density, level)
    got = _device(be, mask, page, level)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"


def test_the_random_set_decides_both_ways_at_every_level():
    for level in LEVELS:
        erased = kept = 0
        for H, W in SIZES:
            for density in (0.02, 0.30):
                e, k = _random_case(H, W, density, level)[3]
                erased, kept = erased + e, kept + k
        assert erased >= 1 and kept >= 1, (level, erased, kept)


def test_labelling_across_many_workgroups(be):
    """1024 x 768 (k = 25): a few hundred blobs, some of them long diagonal chains, one frame-hugging snake; 3072 workgroups label it."""
    H, W = 1024, 768
    rng = np.random.default_rng(77)
    mask = np.zeros((H, W), np.uint8)
    for _ in range(60):
        y, x = int(rng.integers(0, H - 40)), int(rng.integers(0, W - 40))
        mask[y:y + int(rng.integers(1, 40)), x:x + int(rng.integers(1, 40))] = 255
    for _ in range(6):                              # diagonal chains: roots far from most of their pixels
        y, x, n = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2)), int(rng.integers(100, 380))
        mask[y + np.arange(n), x + np.arange(n)] = 255
    mask[60:64, 60:700] = mask[60:900, 60:64] = mask[896:900, 60:700] = 255       # a C that encloses other blobs without closing
    g = rng.integers(0, 256, (H, W), dtype=np.uint8)
    g[H // 2:] //= 3
    page = np.repeat(g[..., None], 3, axis=2)
    for _ in range(4):
        y, x = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 4))
        page[y:y + 3, x:x + 4] = RED
    want = _check(be, mask, page, 10)
    erased, kept = _outcomes(mask, want)
    assert erased >= 1 and kept >= 1, (erased, kept)


# ---- constructed cases ------------------------------------------------------------------------------------------------------

def test_empty_and_full_masks(be):
    H, W = 96, 80
    rng = np.random.default_rng(5)
    page = np.repeat(rng.integers(0, 256, (H, W, 1), dtype=np.uint8), 3, axis=2)
    assert not _check(be, np.zeros((H, W), np.uint8), page, 10).any()
    full = np.full((H, W), 255, np.uint8)
    assert not _check(be, full, page, 10).any()                        # a half-bright frame: the one component goes
    assert _check(be, full, _grey((H, W), 30), 10).all()               # an all-dark frame (ratio 100): it stays
    assert _check(be, np.full((37, 33), 255, np.uint8), _grey((37, 33), 30), 50).all()


def test_ring_and_the_blob_in_its_hole_share_one_contour(be):
    H, W = 96, 80
    mask = np.zeros((H, W), np.uint8)
    mask[20:60, 20:60] = 255
    mask[24:56, 24:56] = 0
    mask[36:44, 36:44] = 255
    page = _grey((H, W), 30)
    want = _check(be, mask, page, 10)
    assert want[40, 40] and want[21, 21]                               # nothing coloured, interior: both stay
    page[30:33, 28:32] = RED                                           # 12 coloured pixels in the hole, outside the blob's own rectangle
    want = _check(be, mask, page, 10)
    assert not want.any()                                              # one external contour: both go


def test_diagonal_touch_is_one_component(be):
    H, W = 37, 33                                                      # k = 0
    mask = np.zeros((H, W), np.uint8)
    mask[5:10, 5:10] = mask[10:15, 10:15] = 255
    page = _grey((H, W), 30)
    page[5:8, 12:16] = RED                                             # inside the union's rectangle only
    assert not _check(be, mask, page, 10).any()
    mask[10:15, 10:15] = 0
    mask[11:16, 10:15] = 255                                           # one row further down: two components, neither sees the colour
    assert np.array_equal(_check(be, mask, page, 10), mask)


def test_a_hole_open_only_through_diagonal_gaps_is_filled(be):
    H, W = 37, 33
    mask = np.zeros((H, W), np.uint8)
    for i in range(13):                                                # a diamond outline drawn with diagonal steps only
        for y, x in ((16 - 12 + i, 16 - i), (16 - 12 + i, 16 + i), (16 + 12 - i, 16 - i), (16 + 12 - i, 16 + i)):
            mask[y, x] = 255
    mask[15:18, 15:18] = 255                                           # a blob inside, not touching
    page = _grey((H, W), 30)
    page[5:8, 8:12] = RED                                              # in the diamond's rectangle, far from the blob's
    assert not _check(be, mask, page, 10).any()                        # the blob lies in the filled diamond and goes with it
    mask[16, 4] = mask[16, 5] = 0                                      # now the inside is open by a real (4-connected) gap ...
    mask[17, 5] = mask[15, 5] = 0
    want = _check(be, mask, page, 10)
    assert want[16, 16] and not want[4, 16]                            # ... and the blob is a contour of its own, which stays


def test_corner_and_edge_components_count_the_frame(be):
    H, W = 96, 80
    mask = np.zeros((H, W), np.uint8)
    mask[0:6, 0:6] = mask[40:50, 0:3] = mask[90:96, 30:70] = mask[50:56, 40:46] = 255
    rng = np.random.default_rng(9)
    page = np.repeat(rng.integers(0, 256, (H, W, 1), dtype=np.uint8), 3, axis=2)
    outcomes = set()
    for level in (1, 2, 3, 10):
        want = _check(be, mask, page, level)
        outcomes |= {(level, bool(want[2, 2]), bool(want[45, 1]), bool(want[93, 50]), bool(want[53, 43]))}
    assert len({o[1:] for o in outcomes}) >= 2                         # the small frame counts make the levels differ
    assert all(o[4] for o in outcomes)                                 # the interior component never sees the frame


def test_overlapping_rectangles_are_judged_separately(be):
    H, W = 37, 33
    mask = np.zeros((H, W), np.uint8)
    mask[5:25, 5:7] = mask[23:25, 5:25] = 255                          # an L ...
    mask[8:12, 12:16] = 255                                            # ... and a blob inside the L's rectangle
    page = _grey((H, W), 30)
    page[15:18, 18:22] = RED                                           # in the L's rectangle, outside the blob's
    want = _check(be, mask, page, 10)
    assert not want[10, 5] and want[9, 13]
    page[15:18, 18:22] = 30
    page[9:12, 13:17] = RED                                            # in both
    assert not _check(be, mask, page, 10).any()


@pytest.mark.parametrize("extra,erased", [(None, False), ((12, 12), True), ((12, 15), True), ((15, 12), True), ((15, 15), True),
                                          ((12, 16), False), ((16, 12), False), ((9, 12), False), ((12, 9), False)])
def test_ten_against_eleven_coloured_pixels_and_the_extra_row_and_column(be, extra, erased):
    """Blob [10:15, 10:15] (k = 0): its rectangle is rows / columns 10..15, one more than it covers to the right and below."""
    H, W = 37, 33
    mask = np.zeros((H, W), np.uint8)
    mask[10:15, 10:15] = 255
    page = _grey((H, W), 30)
    page[10:12, 10:15] = RED                                           # exactly 10
    if extra is not None:
        if extra == (12, 12):
            page[12, 12] = (0, 0, 255)
        else:
            page[extra] = RED
    want = _check(be, mask, page, 10)
    assert bool(want[12, 12]) != erased


def test_frame_brightness_at_the_ends_of_the_interval(be):
    H, W, level = 96, 80, 10
    total = (H * W - (H - 4) * (W - 4)) * 3
    lo, hi = MR.bubble_interval(total, level)
    assert 0 < lo < hi < total
    frame = [(y, x) for y in range(H) for x in range(W) if y < 2 or y >= H - 2 or x < 2 or x >= W - 2]
    mask = np.full((H, W), 255, np.uint8)                              # one component, its rectangle the page
    for dark, erased in ((lo - 1, False), (lo, True), (hi, True), (hi + 1, False)):
        page = _grey((H, W), 50)
        page[10:80, 10:70] = 240                                       # bright, but not in the frame
        bright = total - dark
        for y, x in frame[:bright // 3]:
            page[y, x] = 200
        if bright % 3:
            page[frame[bright // 3]][:bright % 3] = 200                # one pixel bright in one or two channels (coloured, but alone)
        want = _check(be, mask, page, level)
        assert (not want.any()) == erased, (dark, lo, hi)


# ---- the crop test ----------------------------------------------------------------------------------------------------------

def _dark_frame(crop, dark):
    """``dark`` elements of the crop's frame made dark, each in a place the slices count once (widths of 4 and more)."""
    h, w = crop.shape[:2]
    frame = [(y, x) for y in range(h) for x in range(w) if y < 2 or y >= h - 2 or x < 2 or x >= w - 2]
    for y, x in frame[:dark // 3]:
        crop[y, x] = 90
    if dark % 3:
        crop[frame[dark // 3]][:dark % 3] = 90


def _crop_chunk(rng, n, h, level, pad_value=0):
    """A chunk of n lines whose crops cover the rule's branches.  Widths 2 and 3 first: a clean one, a noisy one, and for each width a
    crop whose dark pixels lie where two column slices overlap, as many as reach the interval only when counted twice.  Then widths 4
    and 5 and random ones, in turn: clean bubbles (kept), noise (rejected), 10 and 11 coloured pixels, frames with exactly lo - 1, lo,
    hi and hi + 1 dark elements."""
    widths = ([2, 3, 2, 3, 4, 5] + [int(v) for v in rng.integers(6, 200, n)])[:n] if n > 1 else [int(rng.integers(6, 200))]
    wp = max(widths) + 7
    region = np.full((n, h, wp, 3), pad_value, np.uint8)
    for j, w in enumerate(widths):
        lo, hi = MR.bubble_interval(TL.crop_frame_total(h, w), level)
        crop = np.repeat(rng.integers(200, 256, (h, w, 1), dtype=np.uint8), 3, axis=2)       # a clean bubble
        kind = j if j < 4 and n > 1 else 4 + j % 8
        if kind == 1 or kind == 5 or n == 1:
            crop = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)                           # noise
        elif kind in (2, 3):
            p = -(-lo // 6)                                                                  # pixels: 3p elements, 6p when counted twice
            assert 3 * p < lo <= 6 * p <= hi and p <= h - 4
            crop[2:2 + p, 1 if w == 3 else 0] = 90                                           # w == 2: either column; w == 3: the middle one
        elif kind in (6, 7) and w >= 6:
            crop[5:7, 0:5] = RED                                                             # 10 coloured ...
            if kind == 7:
                crop[h - 1, w - 1] = RED                                                     # ... and the 11th in the last corner
        elif kind in (8, 9, 10, 11) and w >= 4:
            _dark_frame(crop, {8: lo - 1, 9: lo, 10: hi, 11: hi + 1}[kind])
        region[j, :, :w] = crop
    return region, widths


@pytest.mark.parametrize("h,n,pad_value", [(32, 1, 0), (48, 1, 0), (32, 70, 0), (48, 70, 0), (32, 70, 255), (48, 70, 255)])
def test_crop_flags_equal_is_ignore_per_crop(cuda, h, n, pad_value):
    level = 10
    rng = np.random.default_rng([h, n, pad_value])
    region, widths = _crop_chunk(rng, n, h, level, pad_value)
    want_flags = np.array([TL.is_ignore(region[j, :, :w], level) for j, w in enumerate(widths)], np.uint8)
    want = region.copy()
    want[want_flags.astype(bool)] = 0
    if n > 1:                                                          # the oracle decides both ways, and as the recipe intends
        assert want_flags[:6].tolist() == [0, 1, 1, 1, 0, 1] and 0 < want_flags.sum() < n
        by_kind = {k: {int(want_flags[j]) for j in range(6, n) if 4 + j % 8 == k and widths[j] >= 6} for k in range(4, 12)}
        assert by_kind[4] == {0} and by_kind[5] == {1} and by_kind[6] == {0} and by_kind[7] == {1}, by_kind
        assert by_kind[8] == {0} and by_kind[9] == {1} and by_kind[10] == {1} and by_kind[11] == {0}, by_kind
    dev = torch.from_numpy(region).to(cuda)
    flags = TL.bubble_crop_flags(dev, widths, level)
    assert np.array_equal(flags.cpu().numpy(), want_flags), (flags.cpu().numpy().tolist(), want_flags.tolist())
    assert np.array_equal(dev.cpu().numpy(), want)
    with pytest.raises(ValueError):
        TL.bubble_crop_flags(dev, [w + 1000 for w in widths], level)   # a width beyond the chunk never reaches the kernel


# ---- the option through dispatch, the OCR plugins and the coupled engine ------------------------------------------------------

def _page_with_three_lines(H=256, W=192):
    rng = np.random.default_rng(21)
    page = np.repeat(rng.integers(180, 256, (H, W, 1), dtype=np.uint8), 3, axis=2)
    page[:, :50] //= 3                                                 # a dark band down the left: the frame is mixed
    mask = np.zeros((H, W), np.uint8)
    quads = []
    for y0, x0, x1 in ((30, 20, 150), (110, 40, 170), (200, 10, 120)):
        quads.append(np.array([[x0, y0], [x1, y0], [x1, y0 + 24], [x0, y0 + 24]], np.float64))
        for x in range(x0 + 6, x1 - 10, 14):
            mask[y0 + 5:y0 + 19, x:x + 9] = 255
            page[y0 + 5:y0 + 19, x:x + 9] = 20
    page[112:116, 60:64] = RED                                         # 16 coloured pixels on the second line
    regions = [types.SimpleNamespace(lines=[q]) for q in quads]
    return page, mask, regions


def test_dispatch_device_and_dispatch_sync_carry_the_bubble_stage(cuda, be):
    page, mask, regions = _page_with_three_lines()
    pd, md = torch.from_numpy(page).to(cuda), torch.from_numpy(mask).to(cuda)
    plain = MR.dispatch_device(regions, pd, md.clone(), backend=be, ignore_bubble=0)
    assert plain.is_cuda and plain.any()
    want = MR.bubble_filter(plain.cpu().numpy(), page, 10)
    got = MR.dispatch_device(regions, pd, md.clone(), backend=be, ignore_bubble=10)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    host = MR.dispatch_sync(regions, page, mask.copy(), ignore_bubble=10, backend=be, device_result=False)
    assert isinstance(host, np.ndarray) and np.array_equal(host, want)
    assert not np.array_equal(want, plain.cpu().numpy())
    # a backend whose tail runs on the host keeps the numpy stage: same bytes, as a device tensor when asked for one
    host_tail = MR.GpuMaskBackend(cuda, gpu_tail=False)
    again = MR.dispatch_sync(regions, page, mask.copy(), ignore_bubble=10, backend=host_tail, device_result=True)
    assert again.is_cuda and np.array_equal(again.cpu().numpy(), want)


def _bubble_page(H, W, boxes):
    """Every other line is bright writing on a plain dark ground — its frame is all dark, outside 10..90 %, and it is kept (a clean
    WHITE bubble would not be: the rectification's black border beyond the box's last row and column makes a quarter of its frame
    dark) —, the others lie on noise (rejected)."""
    rng = np.random.default_rng(44)
    page = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    for k, b in enumerate(boxes):
        if k % 2 == 0:
            x0, y0, x1, y1 = int(b[0, 0]), int(b[0, 1]), int(b[2, 0]), int(b[2, 1])
            page[max(y0 - 4, 0):y1 + 5, max(x0 - 4, 0):x1 + 5] = 20
            page[y0 + 6:y1 - 5:3, x0 + 6:x1 - 5] = 250
    return page


def _boxes():
    out = []
    for k, (x, y, w, h) in enumerate(((10, 10, 120, 28), (150, 12, 30, 150), (12, 60, 100, 30), (200, 20, 28, 120), (20, 120, 110, 26),
                                      (30, 180, 200, 32))):
        out.append(np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]]))
    return out


def _forced_reject(monkeypatch, flags):
    """``textline.rectified_chunks`` with the device path replaced by the host rule (``plugins._bubble_reject``) whenever a caller asks
    for the option: what the plugins did before the crop test moved to the device."""
    from manga_image_translator_amd import plugins as P

    plain = TL.rectified_chunks

    def forced(page_u8, quads, directions, height, extra=0, reject=None, rectify_fn=None, ignore_bubble=0):
        rule = P._bubble_reject(ignore_bubble)
        if reject is None and rule is not None:
            reject = lambda crop: flags.append(bool(rule(crop))) or flags[-1]
        return plain(page_u8, quads, directions, height, extra, reject, rectify_fn, 0)

    monkeypatch.setattr(TL, "rectified_chunks", forced)


def _results(lines):
    return [(tuple(map(tuple, np.asarray(q.pts).tolist())), q.text, float(q.prob), q.fg_r, q.fg_g, q.fg_b, q.bg_r, q.bg_g, q.bg_b) for q in lines]


def test_ocr_plugins_judge_crops_on_the_device(cuda, monkeypatch):
    import _ocr32_oracle as O
    from manga_image_translator_amd import ocr_ctc_schema as S, plugins as P, synth

    run = lambda c: asyncio.new_event_loop().run_until_complete(c)
    D = 64
    boxes = _boxes()
    page = _bubble_page(256, 320, boxes)
    cfg = types.SimpleNamespace(prob=0.0, ignore_bubble=10)
    ctc_dict = ["<PAD>", "<S>", "</S>", "<SP>"] + [chr(0x3041 + i) for i in range(D - 4)]
    plugins = [(P.HipModel48pxCTCOCR(weights=synth.synth_state_dict(S.ocr_ctc_schema(D), gain=S.CTC_GAIN), dictionary=ctc_dict), {}),
               (P.HipModel32pxOCR(weights=O.weights(D, 0), dictionary=O.dictionary(D)), {"max_seq_length": 12})]
    for ocr, kw in plugins:
        run(ocr.load("cuda"))
        mk = lambda: [P._RefQuadrilateral(b.copy(), "", 1.0) for b in boxes]
        got = _results(run(ocr._infer(page, mk(), cfg, **kw)))
        off = _results(run(ocr._infer(page, mk(), types.SimpleNamespace(prob=0.0, ignore_bubble=0), **kw)))
        flags = []
        with monkeypatch.context() as m:
            _forced_reject(m, flags)
            want = _results(run(ocr._infer(page, mk(), cfg, **kw)))
        run(ocr.unload())
        assert len(flags) == len(boxes) and 0 < sum(flags) < len(flags), flags       # the oracle rejects some lines and keeps some
        assert got == want, type(ocr).__name__
        assert got != off, type(ocr).__name__                                         # and the option changes what is read


def _coupled_pages(H=256, W=192):
    """Two small pages of three speech bubbles each (dark glyph blocks on white, like ``synth.synth_page`` at a size whose lines are
    tall enough to carry glyphs), and the boxes.  Page 0 has 12 coloured pixels in its first bubble: that contour goes."""
    layouts = (((16, 14, 150, 26), (20, 70, 28, 150), (80, 120, 96, 28)), ((30, 20, 120, 24), (140, 70, 30, 140), (14, 110, 100, 26)))
    pages, quads = [], []
    for k, boxes in enumerate(layouts):
        rng = np.random.default_rng(60 + k)
        page = np.clip(rng.normal(235.0, 5.0, (H, W, 1)), 0, 255).astype(np.uint8).repeat(3, axis=2)
        page[:, :3] = 20                                               # a panel border on the page's edge: the frame is not all bright
        qs = []
        for x, y, w, h in boxes:
            page[y:y + h, x:x + w] = 250
            for yy in range(y + 4, y + h - 8, 9):
                for xx in range(x + 4, x + w - 8, 9):
                    page[yy:yy + 6, xx:xx + 6] = 15
            qs.append([[x, y], [x + w, y], [x + w, y + h], [x, y + h]])
        pages.append(page)
        quads.append(np.asarray(qs, np.int64))
    x, y = layouts[0][0][:2]
    pages[0][y + 1:y + 4, x + 12:x + 16] = RED
    return np.stack(pages), quads


def test_coupled_engine_runs_the_bubble_stage(cuda):
    from manga_image_translator_amd import coupled, ctd as CTD, pipeline, plugins as P

    H, W, T, D = 256, 192, 4, 211
    weights = pipeline.synthetic_weights(dict_size=D)
    dictionary = ["<PAD>", "<S>", "</S>", "<SP>"] + [chr(0x4E00 + i) for i in range(D - 4)]
    pages, quads = _coupled_pages(H, W)
    nh, nw, dw, dh = CTD.CtdEngine.letterbox_geometry(H, W)
    heads = [coupled.synthetic_head_outputs(pages[b], quads[b], (CTD.INPUT_SIZE - dh, CTD.INPUT_SIZE - dw)) for b in range(2)]
    inj = {"prob": torch.from_numpy(np.stack([h[0] for h in heads])).to(cuda), "mask": torch.from_numpy(np.stack([h[1] for h in heads])).to(cuda)}
    pages_dev = torch.from_numpy(pages).to(cuda)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        eng = coupled.CoupledPageEngine(weights, dictionary, device=cuda, ctd_mb=2, lama_mb=2, host_workers=2)
        kw = dict(max_seq_length=T, suppress_eos=True, prob_threshold=0.0, inject=inj, inpainting_size=256)
        plain = eng.run(pages_dev, **kw)
        res = eng.run(pages_dev, ignore_bubble=10, **kw)
        torch.cuda.synchronize()
        assert plain.mask[0].any() and plain.mask[1].any()
        want = np.stack([MR.bubble_filter(plain.mask[b].cpu().numpy(), pages[b], 10) for b in range(2)])
        outcomes = [_outcomes(plain.mask[b].cpu().numpy(), want[b]) for b in range(2)]
        assert np.array_equal(res.mask.cpu().numpy(), want)
        assert sum(o[0] for o in outcomes) >= 1 and sum(o[1] for o in outcomes) >= 1, outcomes
        painted = P.inpaint_pages(eng.lama, pages_dev, torch.from_numpy(want).to(cuda), 256, None, eng.lama_mb)
        torch.cuda.synchronize()
        assert torch.equal(res.inpainted, painted)
        eng.close()
