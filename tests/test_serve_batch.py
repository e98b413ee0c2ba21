"""``DenseStages.translate_batch`` without a GPU: how a batch request is cut into coupled runs and looped pages, that results come
back in request order, the ``per_page`` overlay and its checks (MIT_SERVE_ENGINE stub: tests/_serve_batch_stub.py keeps the planning
code and replaces the engines)."""
import asyncio

import numpy as np
import pytest

from manga_image_translator_amd import serve


def _page(h, w, v):
    return np.full((h, w, 3), v, np.uint8)


@pytest.fixture
def stages(monkeypatch):
    monkeypatch.setenv("MIT_SERVE_ENGINE", "tests._serve_batch_stub:make")
    eng = serve._make_engine({})
    assert isinstance(eng, serve.DenseStages)
    return eng


def test_plan_groups_pages_of_equal_size_up_to_batch_size():
    shapes = [(64, 48)] * 3 + [(32, 32)] + [(64, 48)] * 2 + [(32, 32)] + [(16, 16)]
    plan = serve.DenseStages.plan_batches(shapes, [None] * 8, 4)
    assert plan == [([0, 1, 2, 4], ""), ([3, 6], ""), ([5], "alone in its size group"), ([7], "alone in its size group")]
    assert serve.DenseStages.plan_batches(shapes, [None] * 8, 1) == [([i], "batch_size <= 1") for i in range(8)]
    why = [None, "webtoon strip (rearranged detection)"] + [None] * 6
    plan = serve.DenseStages.plan_batches(shapes, why, 16)
    assert plan == [([0, 2, 4, 5], ""), ([1], why[1]), ([3, 6], ""), ([7], "alone in its size group")]
    assert serve.DenseStages.plan_batches([], [], 4) == []


def test_results_come_back_in_request_order(stages):
    pages = [_page(64, 48, 10), _page(32, 32, 20), _page(64, 48, 30), _page(16, 24, 40), _page(32, 32, 50), _page(64, 48, 60)]
    out = asyncio.run(stages.translate_batch(pages, {"ocr": {"max_seq_length": 8}, "inpainter": {"inpainting_size": 512}}, batch_size=2))
    # coupled runs add 1, the loop adds 2 (the stub's marks): pages 0+2 and 1+4 are batched, 3 (own size) and 5 (left over) looped
    assert [int(r["inpainted"][0, 0, 0]) - int(p[0, 0, 0]) for r, p in zip(out, pages)] == [1, 1, 1, 2, 1, 2]
    assert all(r["inpainted"].shape == p.shape for r, p in zip(out, pages))
    assert [c[0] for c in stages.fake.calls] == [(2, 64, 48, 3), (2, 32, 32, 3)]
    kw = stages.fake.calls[0][1]
    assert kw["max_seq_length"] == 8 and kw["inpainting_size"] == 512 and kw["prob_threshold"] == 0.2 and kw["mask_dilation_offset"] == 20
    assert stages.pages_batched == 4 and stages.pages_looped == 2
    assert [e[1] for e in stages.last_batch_plan] == ["", "", "alone in its size group", "alone in its size group"]
    info = asyncio.run(stages.device_info())
    assert info["pages_batched"] == 4 and info["pages_looped"] == 2
    assert set(out[0]) == set(out[3])      # a batched page's dict has the keys translate returns


def test_batch_size_one_is_the_page_loop(stages):
    pages = [_page(32, 32, 1), _page(32, 32, 2), _page(32, 32, 3)]
    for bs in (1, 0):
        out = asyncio.run(stages.translate_batch(pages, {"kernel_size": 5}, batch_size=bs))
        assert [int(r["inpainted"][0, 0, 0]) for r in out] == [3, 4, 5]
    assert not stages.fake.calls and len(stages.loop_calls) == 6 and stages.loop_calls[0][1] == {"kernel_size": 5}
    assert stages.pages_batched == 0 and stages.pages_looped == 6


def test_per_page_overlay_and_its_checks(stages):
    pages = [_page(32, 40, 1), _page(32, 40, 2), _page(8, 8, 3)]
    raw = np.zeros((32, 40), np.uint8)
    raw[3:9, 4:20] = 255
    quads = [[[4, 3], [20, 3], [20, 9], [4, 9]]]
    cfg = {"kernel_size": 3, "per_page": [{"textlines": quads, "mask_raw": raw}, {}, {"mask": np.ones((8, 8), np.uint8)}]}
    out = asyncio.run(stages.translate_batch(pages, cfg, batch_size=4))
    (shape, kw), = stages.fake.calls
    assert shape == (2, 32, 40, 3) and kw["textlines"] == [quads, None] and kw["mask"] == [None, None]
    assert kw["mask_raw"][0] is raw and kw["mask_raw"][1] is None
    assert np.array_equal(out[0]["mask_raw"], raw) and not out[1]["mask_raw"].any()
    # the looped page got the shared config with ITS overlay, and no per_page list
    (_, c2), = stages.loop_calls
    assert c2["kernel_size"] == 3 and "per_page" not in c2 and np.array_equal(c2["mask"], np.ones((8, 8), np.uint8))
    assert serve.DenseStages.page_configs(None, 2) == [{}, {}]
    with pytest.raises(ValueError, match="one entry per image"):
        asyncio.run(stages.translate_batch(pages, {"per_page": [{}, {}]}, batch_size=4))
    with pytest.raises(ValueError, match="only textlines, mask, mask_raw"):
        asyncio.run(stages.translate_batch(pages, {"per_page": [{}, {"kernel_size": 5}, {}]}, batch_size=4))
    with pytest.raises(ValueError, match="mask must be 32x40"):
        asyncio.run(stages.translate_batch(pages[:2], {"per_page": [{"mask": np.zeros((3, 3), np.uint8)}, {}]}, batch_size=4))


def test_pages_the_coupled_engine_does_not_take(stages):
    """A webtoon strip (the detector rearranges it) and ``ocr.ignore_bubble`` go through ``translate`` and say so."""
    strip = _page(4000, 300, 7)
    pages = [strip, strip.copy(), _page(32, 32, 1), _page(32, 32, 2)]
    asyncio.run(stages.translate_batch(pages, None, batch_size=4))
    assert stages.last_batch_plan == [([0], "webtoon strip (rearranged detection)"), ([1], "webtoon strip (rearranged detection)"), ([2, 3], "")]
    asyncio.run(stages.translate_batch(pages[2:], {"ocr": {"ignore_bubble": 5}}, batch_size=4))
    assert all("ignore_bubble" in why for _, why in stages.last_batch_plan)
    assert stages.pages_batched == 2 and stages.pages_looped == 4
