"""Small synthetic pages for the DBNet coupled / serving tests, with the maps a trained DBNet head would give for them.

``synth.synth_page`` scales its text boxes with the page, and at 320 x 200 they are a few pixels high: below what the detector's
representer keeps at ``detect_size`` 256.  These pages carry two boxes sized for that geometry — one horizontal line, one vertical —
with the glyph blobs of ``synth_page`` inside, on its background."""
import numpy as np


def small_page(index: int, H: int, W: int):
    """-> (page u8 [H,W,3], quads int64 [2,4,2]): boxes of 0.6 x 0.11 and 0.17 x 0.40 of the page's (short, long) side."""
    from manga_image_translator_amd import synth

    page = synth.synth_page(index, H, W, n_boxes=0)[0]
    rng = np.random.default_rng(900 + index)
    S, L = min(H, W), max(H, W)
    # the page is cut into two bands along its long side: one box in each, so they never touch
    sizes = [(int(0.6 * S), int(0.11 * L)), (int(0.17 * S), int(0.40 * L))]       # (along the short side, along the long side)
    quads = np.zeros((2, 4, 2), np.int64)
    for b, (s, l) in enumerate(sizes):
        lo, hi = (8, L // 2 - l - 8) if b == 0 else (L // 2 + 8, L - l - 8)
        pl = int(rng.integers(lo, hi + 1))
        ps = int(rng.integers(8, S - s - 8 + 1))
        x0, y0, bw, bh = (ps, pl, s, l) if H >= W else (pl, ps, l, s)
        page[y0:y0 + bh, x0:x0 + bw] = 250
        g = 4
        for yy in range(y0 + 2, y0 + bh - g - 1, g + 2):
            for xx in range(x0 + 2, x0 + bw - g - 1, g + 2):
                if rng.random() < 0.7:
                    page[yy:yy + g, xx:xx + g] = int(rng.integers(0, 40))
        quads[b] = [[x0, y0], [x0 + bw, y0], [x0 + bw, y0 + bh], [x0, y0 + bh]]
    return page, quads


def head_maps(page, quads, detect_size: int):
    """What a trained DBNet would emit for ``page`` at ``detect_size`` (``coupled.synthetic_head_outputs`` at the network's map size, on
    the zero-padded canvas the network sees): (prob f32 [h,w], mask f32 [h/2,w/2]) with h, w the padded network page.  The helper's
    shrink is solved for an unclip ratio of 1.5: call the detector with that."""
    from manga_image_translator_amd import coupled

    H, W = page.shape[:2]
    r = detect_size / max(H, W)
    th, tw = int(round(H * r)), int(round(W * r))
    h, w = th + (256 - th % 256) % 256, tw + (256 - tw % 256) % 256
    prob = np.zeros((h, w), np.float32)
    prob[:th, :tw] = coupled.synthetic_head_outputs(page, quads, (th, tw))[0]
    mask = np.zeros((h // 2, w // 2), np.float32)
    mask[:th // 2, :tw // 2] = coupled.synthetic_head_outputs(page, quads, (th // 2, tw // 2))[1].astype(np.float32) / np.float32(255)
    return prob, mask
