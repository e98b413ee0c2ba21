"""A worker in "config" mode serves the stages the request names: ``detector.detector = default`` + ``inpainter.inpainter = lama_large``
load the DBNet detector and the 18-block LaMa (seeded weights), and a batch request goes through ONE coupled run over those engines
whose pages equal the page loop's (``translate``).  Seeded weights detect nothing, so every page brings the text lines and the raw text
mask a trained detector would give, as in tests/test_serve_batch_gpu.py (whose page comparison, with its 1e-4 on ``prob`` for decoder
batches of different row counts, is the one used here)."""
import asyncio

import numpy as np
import pytest

from tests._dbnet_pages import small_page

pytestmark = pytest.mark.gpu

D, H, W = 211, 320, 200


def _same_page(got, want):
    assert set(got) == set(want)
    for k in ("mask_raw", "mask", "inpainted"):
        assert got[k].dtype == want[k].dtype == np.uint8 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert len(got["textlines"]) == len(want["textlines"])
    for a, b in zip(got["textlines"], want["textlines"]):
        assert a["pts"] == b["pts"] and a["text"] == b["text"] and a["fg"] == b["fg"] and a["bg"] == b["bg"]
        assert abs(a["prob"] - b["prob"]) <= 1e-4, (a["prob"], b["prob"])


def test_config_mode_batch_equals_the_page_loop_on_the_named_stages(cuda):
    from manga_image_translator_amd import coupled, imgproc, plugins as P, serve

    pages, per_page = [], []
    for i in range(3):
        page, quads = small_page(70 + i, H, W)
        raw = imgproc.resize_u8_host(coupled.synthetic_head_outputs(page, quads, (H // 2, W // 2))[1], (W, H))
        assert raw.any()
        pages.append(page)
        per_page.append({"textlines": np.asarray(quads).tolist(), "mask_raw": raw})
    shared = {"detector": {"detector": "default", "detection_size": 256}, "inpainter": {"inpainter": "lama_large", "inpainting_size": 256},
              "ocr": {"max_seq_length": 6, "suppress_eos": True, "prob": 0.0}}
    eng = serve.DenseStages({"dict_size": D, "stages": "config"})
    loop = asyncio.new_event_loop()
    try:
        got = loop.run_until_complete(asyncio.wait_for(eng.translate_batch(pages, {**shared, "per_page": per_page}, batch_size=3), 600))
        assert eng.last_stage_keys == ("default", "48px", "lama_large")
        assert eng.pages_batched == 3 and eng.pages_looped == 0 and eng.last_batch_plan == [([0, 1, 2], "")]
        assert type(eng.det) is P.HipDefaultDetector and type(eng.ocr) is P.HipModel48pxOCR and type(eng.inp) is P.HipLamaLargeInpainter
        assert eng.inp.engine.n_blocks == 18 and eng._coupled[1].dbnet
        for i in range(3):
            want = loop.run_until_complete(asyncio.wait_for(eng.translate(pages[i], {**shared, **per_page[i]}), 300))
            _same_page(got[i], want)
            assert len(want["textlines"]) >= 1 and want["mask"].any() and not np.array_equal(want["inpainted"], pages[i])
            assert np.array_equal(got[i]["mask_raw"], per_page[i]["mask_raw"])
        assert eng.pages_batched == 3 and eng.pages_looped == 0          # translate itself counts nothing
        assert set(eng._plugins) == {("detector", "default"), ("ocr", "48px"), ("inpainter", "lama_large")}    # nothing else was loaded
        info = loop.run_until_complete(eng.device_info())
        assert info["stages"] == "config" and info["last_stage_keys"] == ("default", "48px", "lama_large")
    finally:
        if eng._coupled is not None:
            eng._coupled[1].close()
        loop.close()
