"""The serving worker's ``detector_filters`` parameter (``DenseStages(params={"detector_filters": True})``, ``--detector-filters``,
``MIT_SERVE_DETECTOR_FILTERS=1``), without a GPU, on stub stages: off, nothing changes; on (config mode only), the four options of
``CommonDetector.detect`` are accepted, ``translate`` calls the plugin's ``detect``, and a batch page with an option set or a side
under 400 px takes the page loop with the reason "detector filters"."""
import asyncio

import numpy as np
import pytest

from manga_image_translator_amd import serve

from _serve_batch_stub import FakeCoupled

OPTIONS = ["det_rotate", "det_auto_rotate", "det_invert", "det_gamma_correct"]


class _Det:
    """Records which of ``infer`` / ``detect`` the worker calls, with what; finds no text."""

    def __init__(self):
        self.calls = []

    async def infer(self, page, *args):
        self.calls.append(("infer", page.shape, args))
        return [], np.zeros(page.shape[:2], np.uint8), None

    async def detect(self, page, *args):
        self.calls.append(("detect", page.shape, args))
        return [], np.zeros(page.shape[:2], np.uint8), None


class _Stages(serve.DenseStages):
    """The real ``translate`` and ``translate_batch`` around a recording detector; no text is found, so OCR and inpainting never run."""

    def __init__(self, params=None):
        super().__init__(params)
        self.det, self.ocr, self.inp, self.device_name, self.fake = _Det(), None, None, "stub", FakeCoupled()

    async def _load(self):
        self._loaded = True

    def _coupled_engine(self):
        return self.fake


def _page(h, w, v=3):
    return np.full((h, w, 3), v, np.uint8)


@pytest.mark.parametrize("opt", OPTIONS)
def test_flag_off_the_refusal_is_unchanged(opt, monkeypatch):
    monkeypatch.delenv("MIT_SERVE_DETECTOR_FILTERS", raising=False)
    with pytest.raises(ValueError, match=f"detector.{opt} is set"):
        serve.stage_keys({"detector": {opt: True}})
    with pytest.raises(ValueError, match=f"detector.{opt} is set"):
        serve.stage_keys({"detector": {opt: True}}, detector_filters=False)
    st = _Stages({"stages": "config"})
    assert st.detector_filters is False
    with pytest.raises(ValueError, match=f"detector.{opt} is set"):
        asyncio.run(st.translate(_page(64, 64), {"detector": {opt: True}}))
    assert st.det.calls == []


def test_flag_off_translate_calls_infer_and_small_pages_batch(monkeypatch):
    monkeypatch.delenv("MIT_SERVE_DETECTOR_FILTERS", raising=False)
    st = _Stages({"stages": "config"})
    asyncio.run(st.translate(_page(64, 80), {"detector": {"detection_size": 1536}}))
    assert st.det.calls == [("infer", (64, 80, 3), (1536, 0.5, 0.7, 2.3))]
    asyncio.run(st.translate_batch([_page(64, 80), _page(64, 80)], None, batch_size=2))
    assert st.last_batch_plan == [([0, 1], "")]


@pytest.mark.parametrize("opt", OPTIONS)
def test_flag_on_accepts_the_options(opt):
    assert serve.stage_keys({"detector": {"detector": "ctd", opt: True}}, detector_filters=True) == ("ctd", "48px", "lama_large")
    with pytest.raises(ValueError, match="detector.detector = 'craft'"):     # the other refusals stay
        serve.stage_keys({"detector": {"detector": "craft", opt: True}}, detector_filters=True)


def test_detector_filter_options_are_in_detects_order():
    assert serve.detector_filter_options(None) == serve.detector_filter_options({"detector": {}}) == (False, False, False, False)
    for k, opt in enumerate(("det_invert", "det_gamma_correct", "det_rotate", "det_auto_rotate")):
        assert serve.detector_filter_options({"detector": {opt: True}}) == tuple(i == k for i in range(4))


def test_flag_on_translate_calls_detect_with_the_request_s_options():
    st = _Stages({"stages": "config", "detector_filters": True})
    cfg = {"detector": {"detector": "default", "detection_size": 1536, "unclip_ratio": 2.0, "det_invert": True, "det_auto_rotate": True}}
    res = asyncio.run(st.translate(_page(450, 410), cfg))
    # detect(image, detect_size, text_threshold, box_threshold, unclip_ratio, invert, gamma_correct, rotate, auto_rotate)
    assert st.det.calls == [("detect", (450, 410, 3), (1536, 0.5, 0.7, 2.0, True, False, False, True))]
    assert res["mask_raw"].shape == (450, 410) and st.last_stage_keys == ("default", "48px", "lama_large")
    # no option set: still detect — the border for a page under 400 px comes with it
    asyncio.run(st.translate(_page(96, 160), None))
    assert st.det.calls[-1] == ("detect", (96, 160, 3), (2048, 0.5, 0.7, 2.3, False, False, False, False))


def test_flag_on_batch_pages_take_the_loop_with_the_reason():
    st = _Stages({"stages": "config", "detector_filters": True})
    big = [_page(400, 400, 1), _page(400, 400, 2)]
    asyncio.run(st.translate_batch(big, None, batch_size=2))                       # nothing set, no small side: one coupled run
    assert st.last_batch_plan == [([0, 1], "")] and st.det.calls == []
    for opt in OPTIONS:
        asyncio.run(st.translate_batch(big, {"detector": {opt: True}}, batch_size=2))
        assert st.last_batch_plan == [([0], "detector filters"), ([1], "detector filters")], opt
    assert [c[0] for c in st.det.calls] == ["detect"] * 8
    asyncio.run(st.translate_batch([_page(399, 640), _page(399, 640), _page(640, 399)], None, batch_size=4))   # a side under 400 px
    assert st.last_batch_plan == [([i], "detector filters") for i in range(3)]


def test_fixed_mode_refuses_the_flag(monkeypatch):
    monkeypatch.delenv("MIT_SERVE_STAGES", raising=False)
    with pytest.raises(ValueError, match="detector_filters needs stages='config'"):
        serve.DenseStages({"detector_filters": True})
    with pytest.raises(ValueError, match="detector_filters needs stages='config'"):
        serve.DenseStages({"stages": "fixed", "detector_filters": True})
    monkeypatch.setenv("MIT_SERVE_DETECTOR_FILTERS", "1")
    with pytest.raises(ValueError, match="detector_filters needs stages='config'"):
        serve.DenseStages({})
    assert serve.DenseStages({"stages": "config"}).detector_filters is True
    assert serve.DenseStages({"stages": "fixed", "detector_filters": False}).detector_filters is False    # an explicit parameter wins
    monkeypatch.setenv("MIT_SERVE_DETECTOR_FILTERS", "0")
    assert serve.DenseStages({"stages": "config"}).detector_filters is False


def test_worker_command_line_carries_the_flag(monkeypatch):
    seen = {}
    monkeypatch.setattr(serve, "make_worker", lambda params: seen.update(params) or (_ for _ in ()).throw(SystemExit(0)))
    with pytest.raises(SystemExit):
        serve._main(["worker", "--stages", "config", "--detector-filters"])
    assert seen["detector_filters"] is True and seen["stages"] == "config"
    with pytest.raises(SystemExit):
        serve._main(["worker"])
    assert seen["detector_filters"] is None
