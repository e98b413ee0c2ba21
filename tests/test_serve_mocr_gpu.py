"""A worker in "config" mode serves ``ocr.ocr = "mocr"``: the manga-ocr plugin is loaded at first use (seeded weights: the 48px model
and pipeline.mocr_synthetic's stand-in of the model directory), the page takes the page loop, and the text, prob and colours of every
line are the ones the plugin gives when it is called directly on the same page and lines.  Seeded weights detect nothing, so the page
brings its text lines and raw text mask (as in tests/test_serve_stages_gpu.py)."""
import asyncio

import numpy as np
import pytest

from tests._dbnet_pages import small_page

pytestmark = pytest.mark.gpu

D, H, W = 211, 320, 200


def test_a_config_mode_worker_serves_mocr(cuda):
    from manga_image_translator_amd import coupled, imgproc, plugins as P, serve
    from manga_image_translator_amd.textline import Quadrilateral

    page, quads = small_page(71, H, W)
    raw = imgproc.resize_u8_host(coupled.synthetic_head_outputs(page, quads, (H // 2, W // 2))[1], (W, H))
    cfg = {"detector": {"detector": "default", "detection_size": 256}, "inpainter": {"inpainter": "lama_large", "inpainting_size": 256},
           "ocr": {"ocr": "mocr", "use_mocr_merge": False}, "textlines": np.asarray(quads).tolist(), "mask_raw": raw}
    eng = serve.DenseStages({"dict_size": D, "stages": "config"})
    loop = asyncio.new_event_loop()
    try:
        got = loop.run_until_complete(asyncio.wait_for(eng.translate_batch([page], cfg, batch_size=2), 600))[0]
        assert eng.last_stage_keys == ("default", "mocr", "lama_large") and type(eng.ocr) is P.HipModelMangaOCR
        assert eng.pages_looped == 1 and eng.last_batch_plan == [([0], "ocr.ocr = mocr is not in the coupled engine")]
        lines = [Quadrilateral(np.asarray(p, dtype=np.int64), "", 1.0) for p in cfg["textlines"]]
        want = loop.run_until_complete(asyncio.wait_for(eng.ocr.infer(page, lines, None, False), 300))
        assert len(want) == len(lines) >= 2                          # the plugin returns every line, as the reference does
        want = [l for l in want if l.text.strip()]
        assert len(want) >= 1 and len(got["textlines"]) == len(want)
        for a, b in zip(got["textlines"], want):
            assert a["pts"] == np.asarray(b.pts).tolist() and a["text"] == b.text
            assert a["fg"] == [b.fg_r, b.fg_g, b.fg_b] and a["bg"] == [b.bg_r, b.bg_g, b.bg_b]
            assert abs(a["prob"] - float(b.prob)) <= 1e-6
        print("mocr lines:", [(a["text"], a["prob"], a["fg"], a["bg"]) for a in got["textlines"]])
        assert all(all(0x3042 <= ord(ch) < 0x3042 + 91 for ch in a["text"]) for a in got["textlines"])   # text from the mocr vocabulary
        with pytest.raises(ValueError, match="use_mocr_merge"):
            loop.run_until_complete(asyncio.wait_for(eng.translate(page, {**cfg, "ocr": {"ocr": "mocr", "use_mocr_merge": True}}), 300))
    finally:
        if eng._coupled is not None:
            eng._coupled[1].close()
        loop.close()
