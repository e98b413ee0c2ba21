"""The two host-side facts the ``--ignore-bubble`` kernels (csrc/bubble.hip) rest on, and the entries' argument checks — no GPU needed:

* ``mask_refinement.bubble_interval`` is the integer form of ``ignore_bubble <= round(v / total, 6) * 100 <= 100 - ignore_bubble``:
  compared with a scan of that very expression over every count v, for the frame totals of the OCR crops and of two page sizes;
* the kernels' integer colour rule ``sum_c (1000 c - G)^2 > 10^8``, ``G = 299 r + 587 g + 114 b``, decides every RGB triple the way the
  reference's float64 statement does (``np.dot(img, [0.299, 0.587, 0.114])``, squared distance > 100), and no triple meets the threshold
  exactly — so no float ordering of the statement could decide differently;
* ``mit_bubble_filter`` / ``mit_bubble_crop_flags`` refuse bad arguments before any HIP call, and the workspace size is negative for
  shapes the stage does not take."""
import numpy as np
import pytest

from manga_image_translator_amd import mask_refinement as MR, textline as TL

LEVELS = (1, 5, 10, 25, 49, 50)
CROP_TOTALS = sorted({TL.crop_frame_total(h, w) for h in (32, 48) for w in (2, 3, 4, 5, 37, 512)})
PAGE_TOTALS = [(2048 * 1456 - 2044 * 1452) * 3, (96 * 80 - 92 * 76) * 3]


def test_crop_frame_total_is_the_summed_size_of_is_ignores_slices():
    for h in (32, 48):
        for w in (2, 3, 4, 5, 37, 512):
            d = np.zeros((h, w, 3), bool)
            slices = [d[0:2, 0:w], d[h - 2:h, 0:w], d[2:h - 2, 0:2], d[2:h - 2, w - 2:w]]
            assert TL.crop_frame_total(h, w) == sum(s.size for s in slices), (h, w)


@pytest.mark.parametrize("total", CROP_TOTALS + PAGE_TOTALS)
def test_bubble_interval_equals_a_scan_of_the_python_expression(total):
    for level in LEVELS:
        hit = [v for v in range(total + 1) if level <= round(v / total, 6) * 100 <= 100 - level]
        lo, hi = MR.bubble_interval(total, level)
        if hit:
            assert (lo, hi) == (hit[0], hit[-1]) and len(hit) == hi - lo + 1, (total, level, lo, hi)
        else:
            assert lo > hi, (total, level, lo, hi)
    with pytest.raises(ValueError):
        MR.bubble_interval(0, 10)


def test_bubble_interval_agrees_with_is_ignore_on_crops_at_the_interval_ends():
    """The same interval seen through ``textline.is_ignore`` itself: grey crops (no colour) whose frame holds exactly lo - 1, lo, hi and
    hi + 1 dark elements."""
    h, w = 32, 37
    total = TL.crop_frame_total(h, w)
    for level in (1, 10, 50):
        lo, hi = MR.bubble_interval(total, level)
        for dark, want in ((lo - 1, False), (lo, True), (hi, True), (hi + 1, False)):
            if not 0 <= dark <= total or lo > hi:
                continue
            crop = np.full((h, w, 3), 200, np.uint8)
            frame = [(y, x) for y in range(h) for x in range(w) if y < 2 or y >= h - 2 or x < 2 or x >= w - 2]   # each counted once (w >= 4)
            assert 3 * len(frame) == total
            n = dark // 3                       # whole dark pixels, then the rest one channel at a time
            for y, x in frame[:n]:
                crop[y, x] = 100
            if dark - 3 * n:
                crop[frame[n]][:dark - 3 * n] = 100
            got = TL.is_ignore(crop, level)
            coloured = int((np.sum((crop - np.dot(crop[..., :3], [0.299, 0.587, 0.114])[..., None]) ** 2, axis=-1) > 100).sum())
            assert got == (want or coloured > 10), (level, dark, lo, hi)


def _float_rule(rgb):
    img = rgb.astype(np.uint8)
    gray = np.dot(img[..., :3], [0.299, 0.587, 0.114])[..., np.newaxis]
    return np.sum((img - gray) ** 2, axis=-1)


def _int_rule(rgb):
    c = rgb.astype(np.int64)
    G = 299 * c[..., 0] + 587 * c[..., 1] + 114 * c[..., 2]
    return ((1000 * c - G[..., None]) ** 2).sum(-1)


def test_integer_colour_rule_equals_the_float64_statement_on_every_colour():
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    disagreements = on_threshold = coloured = 0
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], axis=-1)
        s = _int_rule(rgb)
        disagreements += int(((s > 10 ** 8) != (_float_rule(rgb) > 100)).sum())
        on_threshold += int((s == 10 ** 8).sum())
        coloured += int((s > 10 ** 8).sum())
    assert disagreements == 0 and on_threshold == 0
    assert 0 < coloured < 256 ** 3          # both outcomes occur


def test_bubble_entries_refuse_bad_arguments_before_any_hip_call():
    from manga_image_translator_amd import lib

    L = lib.load()
    fake = 4096      # never dereferenced: every call below is refused by the argument checks
    need = L.mit_bubble_filter_workspace_bytes(40, 80)
    assert need >= 8 * 40 * 80 * 4
    for H, W in ((0, 80), (40, 0), (-1, 80), (3, 80), (40, 3), (1 << 16, 1 << 16)):
        assert L.mit_bubble_filter_workspace_bytes(H, W) < 0, (H, W)
    ok = dict(mask=fake, page=fake, H=40, W=80, k=2, lo=10, hi=20, out=fake, ws=fake, ws_bytes=need)

    def filt(**kw):
        a = {**ok, **kw}
        return L.mit_bubble_filter(a["mask"], a["page"], a["H"], a["W"], a["k"], a["lo"], a["hi"], a["out"], a["ws"], a["ws_bytes"], None)

    for name in ("mask", "page", "out", "ws"):
        assert filt(**{name: None}) != 0 and b"null pointer" in L.mit_last_error(), name
    for kw in ({"H": 0}, {"W": 0}, {"H": -4}):
        assert filt(**kw) != 0 and b"must be positive" in L.mit_last_error(), kw
    for kw in ({"H": 3}, {"W": 3}, {"H": 1 << 16, "W": 1 << 16}):
        assert filt(**kw) != 0 and b"bad shape" in L.mit_last_error(), kw
    for kw in ({"k": -1}, {"k": 81}):
        assert filt(**kw) != 0 and b"dilation size" in L.mit_last_error(), kw
    assert filt(ws_bytes=need - 1) != 0 and b"workspace" in L.mit_last_error()
    assert filt(ws=fake + 2) != 0 and b"aligned" in L.mit_last_error()

    assert L.mit_bubble_crop_flags(None, 1, 32, 40, fake, fake, None) != 0 and b"null pointer" in L.mit_last_error()
    assert L.mit_bubble_crop_flags(fake, 1, 32, 40, None, fake, None) != 0 and b"null pointer" in L.mit_last_error()
    assert L.mit_bubble_crop_flags(fake, 1, 32, 40, fake, None, None) != 0 and b"null pointer" in L.mit_last_error()
    for n, h, wp in ((0, 32, 40), (1, 0, 40), (1, 32, 0), (-1, 32, 40)):
        assert L.mit_bubble_crop_flags(fake, n, h, wp, fake, fake, None) != 0 and b"must be positive" in L.mit_last_error(), (n, h, wp)
    for n, h, wp in ((1, 3, 40), (1, 32, 1)):
        assert L.mit_bubble_crop_flags(fake, n, h, wp, fake, fake, None) != 0 and b"bad shape" in L.mit_last_error(), (n, h, wp)
    assert L.mit_bubble_crop_flags(fake, 1, 1 << 15, 1 << 15, fake, fake, None) != 0 and b"too large" in L.mit_last_error()


def test_the_host_chunk_path_of_rectified_chunks_judges_with_is_ignore():
    """``rectified_chunks(ignore_bubble=...)`` on a chunk a host ``rectify_fn`` made (no device involved): the rows ``is_ignore``
    rejects are zeroed, the others are untouched, exactly as with ``reject=`` set to that rule."""
    import torch

    rng = np.random.default_rng(3)
    quads = [TL.Quadrilateral(np.array([[10, 10 + 40 * i], [10 + 60 + 9 * i, 10 + 40 * i], [10 + 60 + 9 * i, 40 + 40 * i], [10, 40 + 40 * i]]))
             for i in range(6)]
    page = torch.zeros(1, 300, 200, 3, dtype=torch.uint8)

    def fake_rectify(page_u8, qs, dirs, idx, records, wp):
        region = np.zeros((len(idx), 32, wp, 3), np.uint8)
        for j, i in enumerate(idx):
            w = int(records["dw"][j])
            region[j, :, :w] = 230 if i % 2 else rng.integers(0, 256, (32, w, 3))     # clean bubble / noise: kept / rejected
        return torch.from_numpy(region)

    runs = {}
    for key, kw in (("flag", dict(ignore_bubble=10)), ("rule", dict(reject=lambda c: TL.is_ignore(c, 10))), ("off", dict())):
        rng = np.random.default_rng(3)
        runs[key] = [r.numpy().copy() for _, _, r in TL.rectified_chunks(page, quads, ["h"] * 6, 32, rectify_fn=fake_rectify, **kw)]
    assert all(np.array_equal(a, b) for a, b in zip(runs["flag"], runs["rule"]))
    zeroed = sum(int(not a[j].any()) for a in runs["flag"] for j in range(len(a)))
    assert 0 < zeroed < 6 and all(b[j].any() for b in runs["off"] for j in range(len(b)))
