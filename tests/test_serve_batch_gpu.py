"""A batch request is served as a batch: ``DenseStages.translate_batch(images, cfg, n)[i]`` equals ``translate(images[i], cfg_i)`` —
text-line geometry, text, colours, raw mask, mask and inpainted page identical; ``prob`` within the 1e-4 the decoder's K-cut FFN form
allows when the number of decoder rows differs — in process and through a pool worker; the ``pages_batched`` / ``pages_looped``
counters say which pages went through one ``CoupledPageEngine.run`` and which took the page loop."""
import asyncio
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 128
OCR = {"max_seq_length": 8, "suppress_eos": True, "prob": 0.0}


def _page_request(index, H, W, lines=5):
    """A synthetic page with the text lines and the raw text mask a trained detector head would give for it (seeded weights detect
    nothing): (page, per_page entry)."""
    from manga_image_translator_amd import coupled, imgproc, synth

    page, quads, _ = synth.synth_page(index, H, W, n_boxes=lines, disjoint=True)
    _, head = coupled.synthetic_head_outputs(page, quads, (H // 2, W // 2))
    raw = imgproc.resize_u8_host(head, (W, H))
    assert raw.any()
    return page, {"textlines": np.asarray(quads).tolist(), "mask_raw": raw}


def _same_page(got, want):
    assert set(got) == set(want)
    for k in ("mask_raw", "mask", "inpainted"):
        assert got[k].dtype == want[k].dtype == np.uint8 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert len(got["textlines"]) == len(want["textlines"])
    for a, b in zip(got["textlines"], want["textlines"]):
        assert a["pts"] == b["pts"] and a["text"] == b["text"] and a["fg"] == b["fg"] and a["bg"] == b["bg"]
        assert abs(a["prob"] - b["prob"]) <= 1e-4, (a["prob"], b["prob"])


@pytest.fixture(scope="module")
def stages(cuda):
    from manga_image_translator_amd import serve

    eng = serve.DenseStages({"dict_size": D})
    loop = asyncio.new_event_loop()
    loop.run_until_complete(eng._load())
    yield eng, loop
    if eng._coupled is not None:
        eng._coupled[1].close()
    loop.close()


def test_batch_request_equals_page_by_page(stages):
    """4 + 4 pages of two sizes (two coupled runs), one of them without text lines, and a ninth page of a third size."""
    eng, loop = stages
    reqs = [_page_request(i, 512, 384) for i in range(4)] + [_page_request(10 + i, 384, 512) for i in range(4)] + [_page_request(20, 256, 320, 3)]
    order = [0, 4, 1, 5, 8, 2, 6, 3, 7]                       # the sizes interleaved: results must come back in request order
    pages = [reqs[i][0] for i in order]
    per_page = [reqs[i][1] for i in order]
    per_page[3] = {"textlines": []}                            # a page without text lines: untouched, zero mask
    cfg = {"ocr": OCR, "inpainter": {"inpainting_size": 512}, "per_page": per_page}
    shared = {k: v for k, v in cfg.items() if k != "per_page"}
    b0, l0 = eng.pages_batched, eng.pages_looped
    got = loop.run_until_complete(asyncio.wait_for(eng.translate_batch(pages, cfg, batch_size=4), 600))
    # the split is stated here, not read from the code under test: two groups of four, the ninth page alone in its size group
    assert eng.pages_batched - b0 == 8 and eng.pages_looped - l0 == 1
    assert len(got) == 9
    n_lines = 0
    for i in range(9):
        want = loop.run_until_complete(asyncio.wait_for(eng.translate(pages[i], {**shared, **per_page[i]}), 300))
        _same_page(got[i], want)
        n_lines += len(want["textlines"])
    assert eng.pages_batched - b0 == 8 and eng.pages_looped - l0 == 1      # translate itself counts nothing
    assert n_lines >= 8                                                      # the OCR had lines to read
    assert np.array_equal(got[3]["inpainted"], pages[3]) and not got[3]["mask"].any() and got[3]["textlines"] == []
    assert got[0]["mask"].any() and not np.array_equal(got[0]["inpainted"], pages[0])
    assert np.array_equal(got[0]["mask_raw"], per_page[0]["mask_raw"])
    info = loop.run_until_complete(eng.device_info())
    assert info["pages_batched"] == eng.pages_batched and info["pages_looped"] == eng.pages_looped


def test_inpainting_size_and_odd_page_size_batched_equal_single(stages):
    """``inpainting_size`` smaller than the page and a page size that is no multiple of 8: the batch takes the plugin's resize /
    composite legs for the whole group and returns the bytes the plugin returns page by page.  One page brings its final mask."""
    eng, loop = stages
    reqs = [_page_request(30 + i, 378, 250, 4) for i in range(3)]
    pages = [p for p, _ in reqs]
    per_page = [pp for _, pp in reqs]
    given = np.zeros((378, 250), np.uint8)
    given[100:160, 40:200] = 255
    per_page[2] = {"textlines": per_page[2]["textlines"], "mask": given}
    cfg = {"ocr": OCR, "inpainter": {"inpainting_size": 192}, "mask_dilation_offset": 10, "kernel_size": 5, "per_page": per_page}
    shared = {k: v for k, v in cfg.items() if k != "per_page"}
    b0, l0 = eng.pages_batched, eng.pages_looped
    got = loop.run_until_complete(asyncio.wait_for(eng.translate_batch(pages, cfg, batch_size=3), 600))
    assert eng.pages_batched - b0 == 3 and eng.pages_looped - l0 == 0
    for i in range(3):
        _same_page(got[i], loop.run_until_complete(asyncio.wait_for(eng.translate(pages[i], {**shared, **per_page[i]}), 300)))
    assert np.array_equal(got[2]["mask"], given) and not np.array_equal(got[2]["inpainted"], pages[2])
    assert got[0]["mask"].any()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_worker_serves_sent_batch_as_a_batch(cuda):
    """One pool worker: ``sent_batch`` returns what ``sent`` returns page by page, and the worker's counters move by the batch size."""
    from manga_image_translator_amd import serve

    reqs = [_page_request(40 + i, 512, 384) for i in range(3)]
    pages = [p for p, _ in reqs]
    per_page = [pp for _, pp in reqs]
    shared = {"ocr": OCR, "inpainter": {"inpainting_size": 512}}
    pool = serve.WorkerPool(gpus=["0"], base_port=_port(), worker_args=["--dict-size", str(D)])
    pool.start(timeout=600)
    try:
        w, = pool.executors.list
        i0 = asyncio.run(asyncio.wait_for(w.sent(None, None, method="device_info"), 120))
        assert i0["pages_batched"] == 0 and i0["pages_looped"] == 0
        got = asyncio.run(asyncio.wait_for(w.sent_batch(pages, {**shared, "per_page": per_page}, batch_size=3), 600))
        i1 = asyncio.run(asyncio.wait_for(w.sent(None, None, method="device_info"), 120))
        assert i1["pages_batched"] == 3 and i1["pages_looped"] == 0
        single = [asyncio.run(asyncio.wait_for(w.sent(pages[i], {**shared, **per_page[i]}), 300)) for i in range(3)]
        looped = asyncio.run(asyncio.wait_for(w.sent_batch(pages, {**shared, "per_page": per_page}, batch_size=1), 600))
        i2 = asyncio.run(asyncio.wait_for(w.sent(None, None, method="device_info"), 120))
        assert i2["pages_batched"] == 3 and i2["pages_looped"] == 3
    finally:
        pool.stop()
    assert len(got) == len(looped) == 3
    for i in range(3):
        _same_page(got[i], single[i])
        _same_page(looped[i], single[i])
    assert sum(len(r["textlines"]) for r in got) >= 3 and got[0]["mask"].any()
