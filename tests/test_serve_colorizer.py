"""Colorization requests on the serving worker (``serve.colorizer_options``, ``DenseStages`` in config mode), without a GPU: the option
mapping and its refusal, the fixed mode, ``stage_keys`` untouched, the batch planning reason, and — on stub stages like those of
tests/test_serve_det_filters.py — the order colorize -> upscale -> detect with the colorized page handed on."""
import asyncio
import types

import numpy as np
import pytest
import torch

from manga_image_translator_amd import serve

from _serve_batch_stub import FakeCoupled


def test_colorizer_options_defaults_dicts_and_objects():
    assert serve.colorizer_options(None) == serve.colorizer_options({}) == ("none", 576, 30)
    assert serve.colorizer_options({"colorizer": None}) == serve.colorizer_options({"colorizer": {}}) == ("none", 576, 30)
    # ColorizerConfig as a front server posts it (config.py:301-307), as a dict or as an object with an enum member
    assert serve.colorizer_options({"colorizer": {"colorization_size": 576, "denoise_sigma": 30, "colorizer": "none"}}) == ("none", 576, 30)
    assert serve.colorizer_options({"colorizer": {"colorizer": "mc2"}}) == ("mc2", 576, 30)
    assert serve.colorizer_options({"colorizer": {"colorizer": "mc2", "colorization_size": 128, "denoise_sigma": 12.5}}) == ("mc2", 128, 12.5)
    assert serve.colorizer_options({"colorizer": {"colorizer": "mc2", "colorization_size": -1, "denoise_sigma": -1}}) == ("mc2", -1, -1)
    enum = lambda v: types.SimpleNamespace(value=v)   # noqa: E731
    obj = types.SimpleNamespace(colorizer=types.SimpleNamespace(colorizer=enum("mc2"), colorization_size=256, denoise_sigma=25))
    assert serve.colorizer_options(obj) == ("mc2", 256, 25)
    key, size, sigma = serve.colorizer_options(types.SimpleNamespace(colorizer=types.SimpleNamespace(colorizer=enum("none"))))
    assert (key, size, sigma) == ("none", 576, 30) and isinstance(size, int)


@pytest.mark.parametrize("key", ["mc1", "sd", "MC2", ""])
def test_an_unknown_colorizer_is_refused_with_the_key_and_the_supported_set(key):
    with pytest.raises(ValueError) as e:
        serve.colorizer_options({"colorizer": {"colorizer": key}})
    msg = str(e.value)
    assert "colorizer.colorizer" in msg and repr(key) in msg and "none" in msg and "mc2" in msg
    assert serve.SUPPORTED_COLORIZER_KEYS == ("none", "mc2")


def test_stage_keys_and_their_tables_are_unchanged_by_a_colorizer_section():
    assert serve.stage_keys({"colorizer": {"colorizer": "mc2"}}) == serve.stage_keys(None) == ("default", "48px", "lama_large")
    assert serve.stage_keys({"colorizer": {"colorizer": "sd"}, "ocr": {"ocr": "32px"}}) == ("default", "32px", "lama_large")   # not its business
    assert list(serve.SUPPORTED_STAGE_KEYS) == [("detector", "detector"), ("ocr", "ocr"), ("inpainter", "inpainter")]
    assert serve.DEFAULT_STAGE_KEYS == ("default", "48px", "lama_large")


class _Det:
    def __init__(self, log):
        self.log = log

    async def infer(self, page, *args):
        self.log.append(("detect", page.copy()))
        return [], np.zeros(page.shape[:2], np.uint8), None


class _Engine:
    """A recording stand-in for ``Mc2Engine`` / ``EsrganEngine`` on the CPU."""
    device = torch.device("cpu")

    def __init__(self, log):
        self.log = log

    def forward(self, pages, size, sigma):           # "colorized": half the size, a constant that encodes the arguments
        self.log.append(("colorize", tuple(pages.shape), size, sigma))
        B, H, W, _ = pages.shape
        return torch.full((B, H // 2, W // 2, 3), 100 + int(sigma), dtype=torch.uint8)

    def upscale(self, pages, ratio):
        self.log.append(("upscale", tuple(pages.shape), ratio, int(pages[0, 0, 0, 0])))
        return pages.repeat_interleave(int(ratio), 1).repeat_interleave(int(ratio), 2) + 1


class _Stages(serve.DenseStages):
    """The real ``translate`` / ``translate_batch`` around recording stages; no text is found, so OCR and inpainting never run."""

    def __init__(self, params=None):
        super().__init__(params)
        self.log = []
        self.det, self.ocr, self.inp, self.device_name, self.fake = _Det(self.log), None, None, "stub", FakeCoupled()
        self.col_loads = 0

    async def _load(self):
        self._loaded = True

    async def _load_colorizer(self):
        if self.col is None:
            self.col_loads += 1
            self.col = types.SimpleNamespace(engine=_Engine(self.log))
        return self.col

    async def _load_upscaler(self):
        if self.up is None:
            self.up = types.SimpleNamespace(engine=_Engine(self.log))
        return self.up

    def _coupled_engine(self):
        return self.fake


def _page(h, w, v=3):
    return np.full((h, w, 3), v, np.uint8)


def test_translate_colorizes_first_and_hands_the_colorized_page_on():
    st = _Stages({"stages": "config"})
    assert st.last_colorizer is None and st.col is None
    cfg = {"colorizer": {"colorizer": "mc2", "colorization_size": 128, "denoise_sigma": 30}}
    res = asyncio.run(st.translate(_page(64, 80), cfg))
    assert [e[0] for e in st.log] == ["colorize", "detect"] and st.log[0] == ("colorize", (1, 64, 80, 3), 128, 30.0)
    assert st.log[1][1].shape == (32, 40, 3) and bool((st.log[1][1] == 130).all())            # the detector saw the colorized page
    assert res["inpainted"].shape == (32, 40, 3) and bool((res["inpainted"] == 130).all())       # and so did everything after it
    assert res["mask_raw"].shape == res["mask"].shape == (32, 40)
    assert st.last_colorizer == "mc2" and st.col_loads == 1
    # request-supplied masks are in the colorized frame
    with pytest.raises(ValueError, match="mask must be 32x40"):
        asyncio.run(st.translate(_page(64, 80), {**cfg, "mask": np.zeros((64, 80), np.uint8)}))
    with pytest.raises(ValueError, match="mask_raw must be 32x40"):
        asyncio.run(st.translate(_page(64, 80), {**cfg, "mask_raw": np.zeros((64, 80), np.uint8)}))
    assert st.col_loads == 1                                                                     # loaded once, by the first request
    # with upscaling: colorize -> upscale -> detect, the upscaler fed the colorized page; revert returns to the request's own size
    st.log.clear()
    asyncio.run(st.translate(_page(64, 80), {**cfg, "upscale": {"upscale_ratio": 2}}))
    assert [e[0] for e in st.log] == ["colorize", "upscale", "detect"]
    assert st.log[1] == ("upscale", (1, 32, 40, 3), 2, 130) and st.log[2][1].shape == (64, 80, 3) and bool((st.log[2][1] == 131).all())
    # a request without the section, or with "none", is served as before: no colorizer call
    st.log.clear()
    for c in (None, {"colorizer": {"colorizer": "none", "colorization_size": 128}}):
        res = asyncio.run(st.translate(_page(64, 80, 9), c))
        assert st.last_colorizer == "none" and bool((res["inpainted"] == 9).all()) and res["inpainted"].shape == (64, 80, 3)
    assert [e[0] for e in st.log] == ["detect", "detect"]
    assert asyncio.run(st.device_info())["last_colorizer"] == "none"
    with pytest.raises(ValueError, match="colorizer.colorizer = 'sd'"):
        asyncio.run(st.translate(_page(64, 80), {"colorizer": {"colorizer": "sd"}}))


def test_fixed_mode_ignores_the_section():
    st = _Stages({})
    assert st.stages == "fixed"
    for key in ("mc2", "sd"):                                    # as it ignores every stage name, supported or not
        res = asyncio.run(st.translate(_page(64, 80, 5), {"colorizer": {"colorizer": key, "colorization_size": 128}}))
        assert res["inpainted"].shape == (64, 80, 3) and st.last_colorizer == "none"
    assert [e[0] for e in st.log] == ["detect", "detect"] and st.col is None
    assert st._loop_reason(_page(64, 80), {"colorizer": {"colorizer": "mc2"}}) is None


def test_a_colorization_page_takes_the_page_loop_with_its_reason():
    st = _Stages({"stages": "config"})
    cfg = {"colorizer": {"colorizer": "mc2", "colorization_size": 128}}
    assert st._loop_reason(_page(64, 80), cfg) == "colorizer"
    assert st._loop_reason(_page(64, 80), {**cfg, "upscale": {"upscale_ratio": 2}}) == "colorizer"     # named first: it runs first
    assert st._loop_reason(_page(64, 80), {"colorizer": {"colorizer": "none"}}) is None
    res = asyncio.run(st.translate_batch([_page(64, 80, 1), _page(64, 80, 2)], cfg, batch_size=2))
    assert st.last_batch_plan == [([0], "colorizer"), ([1], "colorizer")] and st.pages_looped == 2 and st.pages_batched == 0
    assert not st.fake.calls and [e[0] for e in st.log] == ["colorize", "detect"] * 2            # the coupled engine is not touched
    assert all(r["inpainted"].shape == (32, 40, 3) for r in res) and st.last_colorizer == "mc2"
    asyncio.run(st.translate_batch([_page(64, 80, 1), _page(64, 80, 2)], None, batch_size=2))
    assert st.last_batch_plan == [([0, 1], "")] and st.pages_batched == 2
    with pytest.raises(ValueError, match="colorizer.colorizer = 'sd'"):
        asyncio.run(st.translate_batch([_page(64, 80)], {"colorizer": {"colorizer": "sd"}}, batch_size=2))
