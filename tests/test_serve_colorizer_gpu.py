"""A worker in "config" mode serves ``colorizer.colorizer = mc2``: the page is colorized first (seeded synthetic weights, loaded by the
first request that names the colorizer) and the colorized image, at the network's size, is the page of every later stage — exactly
what calling the colorizer plugin and then ``translate`` on its output returns.  Seeded weights detect nothing, so every request brings
the text lines and the raw text mask a trained detector would give, in the frame of the page the detector sees: the colorized one
(182 x 128 for a 300 x 212 page at size 128), as in tests/test_serve_stages_gpu.py."""
import asyncio

import numpy as np
import pytest

import _mc2_oracle as O
from tests._dbnet_pages import small_page

pytestmark = pytest.mark.gpu

D, H, W, SIZE, SIGMA = 211, 300, 212, 128, 30
CH, CW = 182, 128          # Mc2Engine.plan(300, 212, 128, 30): the colorized frame


def _same_page(got, want):
    assert set(got) == set(want)
    for k in ("mask_raw", "mask", "inpainted"):
        assert got[k].dtype == want[k].dtype == np.uint8 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert got["textlines"] == want["textlines"]


def _lines(index, h, w):
    """Text lines and the raw mask a trained detector would give for an h x w page."""
    from manga_image_translator_amd import coupled, imgproc

    page, quads = small_page(index, h, w)
    raw = imgproc.resize_u8_host(coupled.synthetic_head_outputs(page, quads, (h // 2, w // 2))[1], (w, h))
    assert raw.any()
    return {"textlines": np.asarray(quads).tolist(), "mask_raw": raw}


def test_a_colorization_request_equals_the_plugin_then_translate(cuda):
    from PIL import Image

    from manga_image_translator_amd import mc2, plugins as P, serve

    assert mc2.Mc2Engine.plan(H, W, SIZE, SIGMA)[2] == (CH, CW)
    page = O.synth_color_page(61, H, W)
    shared = {"detector": {"detector": "default", "detection_size": 256}, "inpainter": {"inpainter": "lama_large", "inpainting_size": 256},
              "ocr": {"max_seq_length": 6, "suppress_eos": True, "prob": 0.0}}
    col = {"colorizer": {"colorizer": "mc2", "colorization_size": SIZE, "denoise_sigma": SIGMA}}
    small, big = _lines(70, CH, CW), _lines(71, H, W)
    st = serve.DenseStages({"dict_size": D, "stages": "config"})
    loop = asyncio.new_event_loop()
    run = lambda c, t=300: loop.run_until_complete(asyncio.wait_for(c, t))   # noqa: E731
    try:
        # "none", and no section at all: today's result, and no colorizer is loaded
        plain = run(st.translate(page, {**shared, **big}))
        none = run(st.translate(page, {**shared, **big, "colorizer": {"colorizer": "none", "colorization_size": SIZE}}))
        _same_page(none, plain)
        assert st.col is None and st.last_colorizer == "none" and plain["inpainted"].shape == (H, W, 3)
        # mc2: colorize -> detect -> ... in the colorized frame
        got = run(st.translate(page, {**shared, **col, **small}))
        assert type(st.col) is P.HipMangaColorizer and st.col.precision == "fp32" and st.last_colorizer == "mc2"
        assert run(st.device_info())["last_colorizer"] == "mc2"
        colorized = np.asarray(run(st.col.infer(Image.fromarray(page), SIZE, denoise_sigma=SIGMA, text_regions=None)))
        assert colorized.shape == (CH, CW, 3) and colorized.dtype == np.uint8
        want = run(st.translate(colorized, {**shared, **small}))
        _same_page(got, want)
        assert len(want["textlines"]) >= 1 and want["mask"].any() and not np.array_equal(want["inpainted"], colorized)
        assert got["inpainted"].shape == (CH, CW, 3) and np.array_equal(got["mask_raw"], small["mask_raw"])
        assert st.last_colorizer == "none"                                        # (the last request was the uncolorized one)
        # a batch of two such pages: the page loop, with the reason; the coupled engine is not built for it
        res = run(st.translate_batch([page, page.copy()], {**shared, **col, "per_page": [small, small]}, batch_size=2), 600)
        assert st.last_batch_plan == [([0], "colorizer"), ([1], "colorizer")] and st.pages_looped == 2 and st.pages_batched == 0
        assert st._coupled is None and st.last_colorizer == "mc2"
        for r in res:
            _same_page(r, got)
    finally:
        if st._coupled is not None:
            st._coupled[1].close()
        loop.close()
